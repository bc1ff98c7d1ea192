"""The voice-activity and end-of-turn rule of encode sessions opened with voice= (models/stream_sessions.py: EncodeSessions), on the
host: the config, the per-session state, the scan over log-mel frames, and the report a caller reads.  The pool's kernel
(dmel_voice_items) is held to scan() bit for bit; only voice_items(), the launch at the end, needs a GPU.

The detector reads what every step's STFT launch already leaves on the device: the log-mel frames of the session, at the codec's
rate, whatever the session's wire is.  A single level per frame (the mean of log-mel over the bands) does not work: a 20-harmonic
burst at 0.1 peak amplitude over -60 dBFS noise moves that mean by about 1 nat only.  So the rule keeps a noise floor PER BAND and
counts the bands that stand out of it -- the same burst lifts 24 to 62 bands, the noise at most 2.

State of a session: STATE_INTS + n_mels 4-byte words -- floor[b], one fp32 per band, then eight int32: state (0 silence, 1 speech),
run, seen, start, end, starts, active_frames, and one reserved word kept at 0.  A zeroed row is the fresh state: seen == 0 makes
the rule initialise it (the floors from the first frame, start = end = -1).

Per frame f = seen with log-mel column L[b], in frame order:

    1. for every band b of [0, n_mels):   fl = L[b]                                   where seen == 0, else
                                          fl = floor[b] + c * (L[b] - floor[b]),      c = fall         where L[b] < floor[b]
                                                                                      c = rise         else where state == 0
                                                                                      c = rise_speech  else
       (subtract, multiply, add: three fp32 operations, each rounded -- no fused multiply-add);
       floor[b] = min_level where fl < min_level, else fl
    2. exceed[b] = L[b] > min_level and (L[b] - floor[b]) > threshold                 (an fp32 subtract, the UPDATED floor)
    3. count = the bands of [band_lo, band_hi) with exceed (an integer: no order of reduction matters);  active = count >= min_bands
    4. run = run + 1 where active != (state == 1), else 0
    5. state == 0 and run >= attack_frames:       state = 1, start = f - run + 1, starts += 1, run = 0
       else state == 1 and run >= release_frames: state = 0, end = f - run + 1, run = 0
    6. seen += 1, active_frames += active;  flags[f] = active | state << 1 (the state AFTER the frame), counts[f] = count, uint8 both
       (n_mels <= 128 is the STFT's limit already)

The floor falls fast (fall) and rises slowly (rise), slower still while speech is on (rise_speech), so that it sits on the noise
between the harmonics and the syllables; a band that lies at or under min_level -- the clamp of the log, log(1e-5) = -11.5, digital
silence -- never exceeds.  start / end are the first frame of the run that switched the state, so they precede the switch by
attack_frames - 1 / release_frames - 1 frames.

THE DEFAULTS ARE NOT TUNED ON SPEECH: no speech corpus was at hand.  They are checked on synthetic clips only (white noise at -60,
-40 and -30 dBFS and digital silence, a harmonic burst over it: tests/test_voice_cpu.py), and a deployment should set its own.
The frame counter is an int32: 2^31 frames are 265 days at 93.75 frames per second (hop 256 at 24 kHz); nothing checks for the
overflow.  NaN input is outside the contract."""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib

STATE_INTS = 8                                         # int32 words behind the floors of a state row
MAX_MELS = 128                                         # what dmel_voice_items takes (the STFT's own limit)
MAX_RUN = 1 << 20                                      # attack_frames and release_frames
TABLE_WORDS = 12                                       # 4-byte words of table scratch per slot of dmel_voice_items
I_STATE, I_RUN, I_SEEN, I_START, I_END, I_STARTS, I_ACTIVE, I_RESERVED = range(STATE_INTS)


@dataclasses.dataclass(frozen=True)
class VoiceConfig:
    """Plain values; see the module for what each does.  threshold and min_level are in nats of log-magnitude (the codec's log-mel);
    bands: None for all bands, or (lo, hi) for the window [lo, hi) that is counted (the floors of all bands are kept either way).
    The defaults are not tuned on speech."""
    threshold: float = 1.5
    min_level: float = -10.0
    fall: float = 0.1
    rise: float = 0.02
    rise_speech: float = 0.002
    bands: Optional[Tuple[int, int]] = None
    min_bands: int = 4
    attack_frames: int = 3
    release_frames: int = 47                           # about 0.5 s at hop 256 / 24 kHz

    def __post_init__(self):
        for name in ("threshold", "min_level", "fall", "rise", "rise_speech"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"{name} must be a finite number, got {v!r}")
            object.__setattr__(self, name, float(v))
        if not self.threshold > 0:
            raise ValueError(f"threshold must be > 0, got {self.threshold}")
        for name in ("fall", "rise"):
            if not 0 < getattr(self, name) <= 1:
                raise ValueError(f"{name} must lie in (0, 1], got {getattr(self, name)}")
        if not 0 <= self.rise_speech <= 1:
            raise ValueError(f"rise_speech must lie in [0, 1], got {self.rise_speech}")
        if self.bands is not None:
            b = self.bands
            if (not isinstance(b, (tuple, list)) or len(b) != 2 or any(isinstance(x, bool) or not isinstance(x, int) for x in b)
                    or not 0 <= b[0] < b[1] <= MAX_MELS):
                raise ValueError(f"bands must be None or (lo, hi) with 0 <= lo < hi <= n_mels, got {b!r}")
            object.__setattr__(self, "bands", (b[0], b[1]))
        for name, top in (("min_bands", MAX_MELS), ("attack_frames", MAX_RUN), ("release_frames", MAX_RUN)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= top:
                raise ValueError(f"{name} must be an integer in [1, {top}], got {v!r}")

    def window(self, n_mels: int) -> Tuple[int, int]:
        """the counted bands [lo, hi) in a transform of n_mels bands; ValueError where the config does not fit it"""
        if isinstance(n_mels, bool) or not isinstance(n_mels, int) or not 1 <= n_mels <= MAX_MELS:
            raise ValueError(f"n_mels must be an integer in [1, {MAX_MELS}], got {n_mels!r}")
        lo, hi = (0, n_mels) if self.bands is None else self.bands
        if not 0 <= lo < hi <= n_mels:
            raise ValueError(f"bands [{lo}, {hi}) are not a window of the {n_mels} mel bands")
        if not 1 <= self.min_bands <= hi - lo:
            raise ValueError(f"min_bands = {self.min_bands} must lie in [1, {hi - lo}], the width of the band window")
        return lo, hi

    def fparams(self) -> Tuple[float, ...]:
        """(threshold, min_level, fall, rise, rise_speech): a row of dmel_voice_items' fparams (rounded to fp32 there and in scan)"""
        return (self.threshold, self.min_level, self.fall, self.rise, self.rise_speech)

    def iparams(self, n_mels: int) -> Tuple[int, ...]:
        """(band_lo, band_hi, min_bands, attack_frames, release_frames): a row of dmel_voice_items' iparams"""
        lo, hi = self.window(n_mels)
        return (lo, hi, self.min_bands, self.attack_frames, self.release_frames)

    def as_dict(self) -> dict:
        """plain values (a snapshot's meta)"""
        d = dataclasses.asdict(self)
        d["bands"] = None if self.bands is None else list(self.bands)
        return d

    @classmethod
    def from_dict(cls, d) -> "VoiceConfig":
        d = dict(d)
        if d.get("bands") is not None:
            d["bands"] = tuple(d["bands"])
        return cls(**d)


def as_config(voice) -> Optional[VoiceConfig]:
    """what open(voice=) takes: None / False -> None, True -> the defaults, a VoiceConfig -> itself"""
    if voice is None or voice is False:
        return None
    if voice is True:
        return VoiceConfig()
    if isinstance(voice, VoiceConfig):
        return voice
    raise ValueError(f"voice must be None, a bool or a VoiceConfig, got {type(voice).__name__}")


def fresh_state(n_mels: int) -> torch.Tensor:
    """(n_mels + 8,) int32 zeros: the state of a session that has seen no frame"""
    return torch.zeros(n_mels + STATE_INTS, dtype=torch.int32)


def _check_state(state: torch.Tensor, n_mels: int) -> None:
    if state.dtype != torch.int32 or tuple(state.shape) != (n_mels + STATE_INTS,) or state.device.type != "cpu":
        raise ValueError(f"state must be a CPU int32 tensor of {n_mels} + {STATE_INTS} words, got {tuple(state.shape)} {state.dtype}")


def scan(mel: torch.Tensor, config: VoiceConfig, state: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """mel: (n_mels, T) CPU fp32 log-mel frames, T >= 0; state: what an earlier call returned (None: fresh) -> (state after the
    frames, flags (T,) uint8, counts (T,) uint8).  `state` is not modified.  Any split of the frames gives the bits of one call."""
    if mel.ndim != 2 or mel.dtype != torch.float32 or mel.device.type != "cpu":
        raise ValueError(f"mel must be a CPU fp32 tensor (n_mels, T), got {tuple(mel.shape)} {mel.dtype} on {mel.device}")
    n_mels, T = int(mel.shape[0]), int(mel.shape[1])
    lo, hi, min_bands, attack, release = config.iparams(n_mels)
    thr, min_level, fall, rise, rise_speech = (np.float32(v) for v in config.fparams())
    if state is None:
        state = fresh_state(n_mels)
    _check_state(state, n_mels)
    words = state.clone().numpy()
    if T == 0:                                                               # as an idle slot of the launch: the row is not touched
        return torch.from_numpy(words), torch.zeros(0, dtype=torch.uint8), torch.zeros(0, dtype=torch.uint8)
    floor = words[:n_mels].view(np.float32).copy()
    st, run, seen, start, end, starts, act_frames, _ = (int(v) for v in words[n_mels:])
    if seen == 0:
        start = end = -1
    x = np.ascontiguousarray(mel.numpy().T)                                  # (T, n_mels): a frame is a row
    flags, counts = np.zeros(T, dtype=np.uint8), np.zeros(T, dtype=np.uint8)
    for t in range(T):
        L = x[t]
        if seen == 0:
            fl = L.copy()
        else:
            c = np.where(L < floor, fall, rise if st == 0 else rise_speech).astype(np.float32)
            d = L - floor
            p = c * d
            fl = floor + p                                                   # three fp32 operations, each rounded
        floor = np.where(fl < min_level, min_level, fl).astype(np.float32)
        exceed = (L > min_level) & ((L - floor) > thr)
        count = int(np.count_nonzero(exceed[lo:hi]))
        active = 1 if count >= min_bands else 0
        run = run + 1 if active != (1 if st == 1 else 0) else 0
        if st == 0 and run >= attack:
            st, start, starts, run = 1, seen - run + 1, starts + 1, 0
        elif st == 1 and run >= release:
            st, end, run = 0, seen - run + 1, 0
        seen += 1
        act_frames += active
        flags[t], counts[t] = active | st << 1, count
    words[:n_mels] = floor.view(np.int32)
    words[n_mels:] = (st, run, seen, start, end, starts, act_frames, 0)
    return torch.from_numpy(words), torch.from_numpy(flags), torch.from_numpy(counts)


@dataclasses.dataclass(frozen=True)
class VoiceReport:
    """What a caller reads of a session's detector, built from its eight integers.  Frames are frames of the codec's transform
    (hop samples at the codec's rate each): samples(frame) and seconds(frame) convert.

        speaking         the state after the newest frame
        frames           frames seen
        speech_start     the first frame of the newest speech segment (None: none yet)
        speech_end       the first frame of the silence that ended the newest finished segment (None: none yet)
        starts           speech segments begun
        active_frames    frames whose band count reached min_bands
        silence_frames   0 while speaking, else the frames since speech_end (since frame 0 where nothing has ended yet)
        end_of_turn      starts > 0 and not speaking: the speaker has spoken and has stopped
    """
    speaking: bool
    frames: int
    speech_start: Optional[int]
    speech_end: Optional[int]
    starts: int
    active_frames: int
    hop: int = 256
    sample_rate: int = 24000

    @property
    def silence_frames(self) -> int:
        return 0 if self.speaking else self.frames - (self.speech_end or 0)

    @property
    def end_of_turn(self) -> bool:
        return self.starts > 0 and not self.speaking

    def samples(self, frame: int) -> int:
        """the first sample of `frame`'s hop, at the codec's rate"""
        return int(frame) * self.hop

    def seconds(self, frame: int) -> float:
        return self.samples(frame) / self.sample_rate


def report(state: torch.Tensor, hop: int = 256, sample_rate: int = 24000) -> VoiceReport:
    """the report of a state row (its last 8 words are read; any device -- one copy to the host)"""
    st, run, seen, start, end, starts, act_frames, _ = (int(v) for v in state[-STATE_INTS:].tolist())
    return VoiceReport(speaking=st == 1, frames=seen, speech_start=None if start < 0 or seen == 0 else start,
                       speech_end=None if end < 0 or seen == 0 else end, starts=starts, active_frames=act_frames, hop=int(hop),
                       sample_rate=int(sample_rate))


# ---------------------------------------------------------------------------------------------------- the launch
def voice_items(mel: torch.Tensor, n_frames: Sequence[int], configs: Sequence[Optional[VoiceConfig]], state: torch.Tensor,
                flags: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None, table: Optional[torch.Tensor] = None) -> None:
    """all slots of a step in ONE launch (dmel_voice_items).  mel: (S, n_mels, tmax) fp32 CUDA with contiguous frames; n_frames[s]
    <= tmax frames of slot s are scanned (0: the slot is idle, its rows are not touched, configs[s] may be None); state: (S, n_mels + 8)
    int32, contiguous, updated in place; flags / counts: (S, pitch) uint8, contiguous, pitch >= every n_frames[s], bytes behind a
    row's frames are not written.  table: int32 device scratch of 12 * S words a caller that scans every step keeps (default:
    allocated here).  Runs on the current stream."""
    _lib.require_cuda(mel, "mel")
    if mel.ndim != 3 or mel.dtype != torch.float32 or (mel.shape[2] > 1 and mel.stride(2) != 1):
        raise ValueError(f"mel must be an fp32 tensor (S, n_mels, frames) with contiguous frames, got {tuple(mel.shape)} {mel.dtype}")
    S, n_mels, tmax = (int(v) for v in mel.shape)
    dev = mel.device
    if len(n_frames) != S or len(configs) != S:
        raise ValueError(f"{S} slots need {S} frame counts and configs, got {len(n_frames)} and {len(configs)}")
    if state.dtype != torch.int32 or tuple(state.shape) != (S, n_mels + STATE_INTS) or not state.is_contiguous() or state.device != dev:
        raise ValueError(f"state must be a contiguous int32 tensor ({S}, {n_mels + STATE_INTS}) on {dev}")
    pitch = 0
    for t, name in ((flags, "flags"), (counts, "counts")):
        if t is None:
            continue
        if t.dtype != torch.uint8 or t.ndim != 2 or t.shape[0] != S or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be a contiguous uint8 tensor ({S}, pitch) on {dev}")
        if pitch and t.shape[1] != pitch:
            raise ValueError("flags and counts must have one pitch")
        pitch = int(t.shape[1])
    fp, ip = [], []
    for s in range(S):
        n = int(n_frames[s])
        if n > tmax:
            raise ValueError(f"slot {s}: {n} frames exceed the {tmax} of mel")
        if n and configs[s] is None:
            raise ValueError(f"slot {s} has {n} frames and no config")
        cfg = configs[s] if n else None
        fp += cfg.fparams() if cfg else (0.0,) * 5
        ip += cfg.iparams(n_mels) if cfg else (0,) * 5
    if flags is None and counts is None:
        pitch = tmax
    if table is None:
        table = torch.empty(TABLE_WORDS * S, dtype=torch.int32, device=dev)
    elif table.dtype != torch.int32 or table.numel() < TABLE_WORDS * S or table.device != dev or not table.is_contiguous():
        raise ValueError(f"table must hold {TABLE_WORDS * S} contiguous int32 on {dev}")
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dmel_voice_items(mel.data_ptr(), mel.stride(0), mel.stride(1), n_mels, S, (C.c_int64 * S)(*[int(n) for n in n_frames]),
                                               (C.c_float * (5 * S))(*fp), (C.c_int32 * (5 * S))(*ip), state.data_ptr(),
                                               _lib.ptr(flags), _lib.ptr(counts), pitch, table.data_ptr(), _lib.stream_ptr()),
                   "voice_items")
