"""The noise suppression rule of encode sessions opened with denoise= (models/stream_sessions.py: EncodeSessions), on the host: the
config, the per-session state, the scan over samples, and the report a caller reads.  The pool's kernel (dmel_denoise_items) is held
to scan() bit for bit; only denoise_items(), the launch at the end, needs a GPU.

What it is: a single-channel spectral-gain suppressor of STATIONARY noise -- a learnt and slowly tracked noise power per bin, a
decision-directed a-priori SNR, a Wiener gain with a floor -- on the session's samples at the codec's rate, as f32, behind the
convert, downmix, resample, conceal, echo and DTMF launches and in front of the leveller.  It is the first option with a delay.

Framing.  N = frame_samples, a power of two in 64 .. 1024 (default 512: 21.3 ms at 24 kHz), hop H = N / 2, window
w[i] = sin(pi (i + 0.5) / N) for analysis and for synthesis (the shifted squares sum to 1).  Frame k = 0, 1, ... covers the stream
positions [(k - 1) H, (k + 1) H); positions below 0 read as 0.  Frame k is computed when sample (k + 1) H - 1 has arrived and completes
the suppressed signal y on [(k - 1) H, k H): its first half plus the second half of frame k - 1 (the overlap tail).  The hop that
frame 0 completes lies in front of the stream and is zeros.

Delay.  out[p] = y[p - N], the first N outputs are 0, the length is kept: while the input hop [(k + 1) H, (k + 2) H) streams in, the
hop frame k completed streams out, sample for sample, so the samples are re-written in place and the session's timeline does not
move.  DenoiseConfig.delay(rate) reports the N samples.  THE LAST N INPUT SAMPLES OF A STREAM ARE NOT EMITTED; a caller who wants
them pushes N zeros behind them.

The constant table (transform_table(), TRANSFORM_WORDS = 3072 fp32 words, computed in float64 and rounded once):

    [0, 2048)      S[k] = sin(pi k / 2048):                 w[i] = S[(2 i + 1) (1024 / N)]
    [2048, 2560)   C[k] = cos(2 pi k / 1024), k < 512       the twiddle of angle 2 pi j / M is k = j (1024 / M):
    [2560, 3072)   Z[k] = sin(2 pi k / 1024), k < 512       forward  wr = C[k], wi = -Z[k];   inverse  wr = C[k], wi = Z[k]

Every fp32 operation below is rounded on its own: no fused multiply-add, the division is the IEEE one.

Transform.  Radix-2, complex, N points, in place on (re, im).  The complex product (tr, ti) = (wr, wi) * (br, bi) is
tr = wr br - wi bi, ti = wr bi + wi br: four products, one difference, one sum.
  forward (decimation in frequency; natural order in, bit-reversed out: bin b ends at index rev(b), the log2 N bits of b reversed):
    re[i] = x[i] * w[i], im[i] = 0;  for h = N/2, N/4, .., 1, for every a with (a mod 2h) < h, b = a + h, j = a mod 2h, M = 2h:
        u = x[a] + x[b];  d = x[a] - x[b];  x[a] = u;  x[b] = w_fwd(j, M) * d
  inverse (decimation in time; bit-reversed in, natural out), for h = 1, 2, .., N/2, a, b, j, M as above:
        t = w_inv(j, M) * x[b];  u = x[a] + t;  d = x[a] - t;  x[a] = u;  x[b] = d
    v[i] = (re[i] * (1 / N)) * w[i]          (the scale is exact; the imaginary part is dropped)

Per frame, with the fp32 parameters alpha, oma = fp32(1 - alpha), track, track_ratio, creep, floor_gain, eps and the integer
learn_frames; P[b] = re re + im im of bin b = 0 .. H (two products, one sum), and P[b] < TINY = 1e-30 counts as 0 (squares of very
quiet inputs are subnormal; the clamp keeps them out of every quotient):

    power_in = SUM(P).  SUM(v) over b = 0 .. H: 64 partials, partial l = ((v[l] + v[l + 64]) + v[l + 128]) + ..., ascending, then the
    xor tree t = 32, 16, .., 1: partial[l] = partial[l] + partial[l ^ t]; the sum is partial 0.
    power_in == 0 (digital silence): Nz, prev, learned and the sums keep their values, power_out = 0, and v = 0.
    otherwise, per bin:
        learned < learn_frames:  d = P - Nz;  d = d / fp32(learned + 1);  Nz = Nz + d          (the running mean of the first frames)
        else:                    Nz = Nz * creep;  t = track_ratio * Nz;
                                 P < t:  d = P - Nz;  d = track * d;  Nz = Nz + d               (one rate in both directions)
        den = max(Nz, eps);  post = P / den;  e = max(post - 1, 0)
        prio = alpha * prev + oma * e                                                           (two products, one sum)
        G = prio / (1 + prio);  G = max(G, floor_gain);  g2 = G * G;  prev = g2 * post;  Q = g2 * P
        bin b is scaled at index rev(b): (re, im) = (G re, G im); for 0 < b < H index rev(N - b) gets (G re, -(G im))
      power_out = SUM(Q);  learned += 1 while below learn_frames;  sum_in += power_in;  sum_out += power_out
    hop[i] = frames == 0 ? 0 : tail[i] + v[i];   tail[i] = v[H + i]   (i < H);   frames += 1;  raw[0 .. H) = raw[H .. N)

The creep lets a floor that jumped up be re-learnt within seconds; tracking only where P < track_ratio * Nz keeps tones that arrive
abruptly out of the noise estimate, while a sound that fades in over seconds is learnt as noise.

State of a session: STATE_WORDS = 3092 4-byte words, the same layout for every N (an N below 1024 uses the front of each part):

    header, HEADER_WORDS = 16:   0 frames int32   1 fill int32 (samples of the open hop)   2 learned int32   3 sum_in fp32
                                 4 sum_out fp32   5 nz_sum fp32 = SUM(Nz), written by every call with samples   6 .. 15 kept at 0
    O_RAW  = 16    raw[1024]     the last whole hop at [0, H), the open hop's samples at [H, H + fill)
    O_TAIL = 1040  tail[512]     O_HOP = 1552  hop[512]      O_NZ = 2064  Nz[513]      O_PREV = 2577  prev[513]      (2 words unused)

A zeroed row is the fresh state.  THE DEFAULTS ARE CHECKED ON SYNTHETIC SIGNALS ONLY (tests/test_denoise_cpu.py); no conformance is
claimed.  NaN and infinite input are outside the contract.  Not served: transient or non-stationary noise, comfort noise, a residual
echo suppressor driven by the canceller, learned suppressors, delay compensation of the reports of other options."""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib

MIN_FRAME, MAX_FRAME = 64, 1024
MAX_HOP = MAX_FRAME // 2
HEADER_WORDS = 16
O_RAW = HEADER_WORDS
O_TAIL = O_RAW + MAX_FRAME
O_HOP = O_TAIL + MAX_HOP
O_NZ = O_HOP + MAX_HOP
O_PREV = O_NZ + MAX_HOP + 1
STATE_WORDS = (O_PREV + MAX_HOP + 1 + 3) // 4 * 4      # 3092
TABLE_WORDS = 16                                       # 4-byte words of table scratch per slot of dmel_denoise_items
TRANSFORM_WORDS = 2 * MAX_FRAME + MAX_FRAME            # the constant table: S, C, Z
T_COS, T_SIN = 2 * MAX_FRAME, 2 * MAX_FRAME + MAX_HOP
TINY = 1e-30
I_FRAMES, I_FILL, I_LEARNED, I_SUM_IN, I_SUM_OUT, I_NZ_SUM = range(6)
_FLOATS = ("alpha", "track", "track_ratio", "creep", "floor_gain", "eps")


@dataclasses.dataclass(frozen=True)
class DenoiseConfig:
    """Plain values; see the module for what each does.  The defaults are checked on synthetic signals only."""
    frame_samples: int = 512
    alpha: float = 0.96                                # decision-directed smoothing of the a-priori SNR, in [0, 1)
    track: float = 0.05                                # rate of the noise tracker, in (0, 1]
    track_ratio: float = 6.0                           # bins below this multiple of the noise power are tracked, >= 1
    creep: float = 1.002                               # growth of the noise power per frame, in [1, 2]
    floor_gain: float = 0.126                          # -18 dB: the least gain of a bin, in (0, 1]
    eps: float = 1e-20                                 # the least noise power a quotient divides by
    learn_frames: int = 16                             # frames (not silent) whose mean power starts the noise estimate, 1 .. 4096

    def __post_init__(self):
        n = self.frame_samples
        if isinstance(n, bool) or not isinstance(n, int) or not MIN_FRAME <= n <= MAX_FRAME or n & (n - 1):
            raise ValueError(f"frame_samples must be a power of two in [{MIN_FRAME}, {MAX_FRAME}], got {n!r}")
        k = self.learn_frames
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= 4096:
            raise ValueError(f"learn_frames must be an integer in [1, 4096], got {k!r}")
        for name in _FLOATS:
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"{name} must be a finite number, got {v!r}")
            object.__setattr__(self, name, float(v))
        if not 0.0 <= self.alpha < 1.0:
            raise ValueError(f"alpha must be in [0, 1), got {self.alpha!r}")
        if not 0.0 < self.track <= 1.0:
            raise ValueError(f"track must be in (0, 1], got {self.track!r}")
        if not 1.0 <= self.track_ratio <= 1e6:
            raise ValueError(f"track_ratio must be in [1, 1e6], got {self.track_ratio!r}")
        if not 1.0 <= self.creep <= 2.0:
            raise ValueError(f"creep must be in [1, 2], got {self.creep!r}")
        if not 1e-6 <= self.floor_gain <= 1.0:
            raise ValueError(f"floor_gain must be in [1e-6, 1], got {self.floor_gain!r}")
        if not TINY <= self.eps <= 1.0:
            raise ValueError(f"eps must be in [{TINY}, 1], got {self.eps!r}")

    @property
    def hop(self) -> int:
        return self.frame_samples // 2

    def delay(self, sample_rate: int = 24000) -> float:
        """the delay of the output against the input in seconds at `sample_rate`: frame_samples samples"""
        if isinstance(sample_rate, bool) or not isinstance(sample_rate, int) or sample_rate <= 0:
            raise ValueError(f"sample_rate must be a positive integer, got {sample_rate!r}")
        return self.frame_samples / sample_rate

    def fparams(self) -> Tuple[float, ...]:
        """(alpha, oma, track, track_ratio, creep, floor_gain, eps, 1 / N) as the fp32 values scan and dmel_denoise_items compute with"""
        return _fparams(self)

    def as_dict(self) -> dict:
        """plain values (a snapshot's meta)"""
        return dataclasses.asdict(self)

    @classmethod
    def from_dict(cls, d) -> "DenoiseConfig":
        return cls(**dict(d))


@functools.lru_cache(maxsize=64)
def _fparams(config: DenoiseConfig) -> Tuple[float, ...]:
    return tuple(float(np.float32(v)) for v in (config.alpha, 1.0 - config.alpha, config.track, config.track_ratio, config.creep,
                                                config.floor_gain, config.eps, 1.0 / config.frame_samples))


def as_config(denoise) -> Optional[DenoiseConfig]:
    """what open(denoise=) takes: None / False -> None, True -> the defaults, a DenoiseConfig -> itself"""
    if denoise is None or denoise is False:
        return None
    if denoise is True:
        return DenoiseConfig()
    if isinstance(denoise, DenoiseConfig):
        return denoise
    raise ValueError(f"denoise must be None, a bool or a DenoiseConfig, got {type(denoise).__name__}")


def fresh_state() -> torch.Tensor:
    """(STATE_WORDS,) int32 zeros: the state of a session that has seen no sample"""
    return torch.zeros(STATE_WORDS, dtype=torch.int32)


@functools.lru_cache(maxsize=1)
def _table() -> np.ndarray:
    k = np.arange(2 * MAX_FRAME, dtype=np.float64)
    j = np.arange(MAX_HOP, dtype=np.float64)
    t = np.concatenate([np.sin(np.pi * k / (2 * MAX_FRAME)), np.cos(2 * np.pi * j / MAX_FRAME), np.sin(2 * np.pi * j / MAX_FRAME)])
    t = t.astype(np.float32)
    t.setflags(write=False)
    return t


def transform_table() -> torch.Tensor:
    """(TRANSFORM_WORDS,) fp32 on the host: the window and twiddle table every N strides through"""
    return torch.from_numpy(_table().copy())


@functools.lru_cache(maxsize=8)
def _plan(N: int):
    """(window (N,), rev (N,), the (cos, sin) of the forward stages h = N/2 .. 1, each (h,)) of an N-point frame"""
    t, r = _table(), MAX_FRAME // N
    win = t[(2 * np.arange(N) + 1) * r]
    bits = N.bit_length() - 1
    rev = np.zeros(N, dtype=np.int64)
    for b in range(bits):
        rev |= ((np.arange(N) >> b) & 1) << (bits - 1 - b)
    tw = {}
    h = N // 2
    while h >= 1:
        k = np.arange(h) * (MAX_FRAME // (2 * h))
        tw[h] = (t[T_COS + k], t[T_SIN + k])
        h //= 2
    return win, rev, tw


def _forward(re: np.ndarray, im: np.ndarray, tw) -> Tuple[np.ndarray, np.ndarray]:
    N = re.shape[0]
    h = N // 2
    while h >= 1:
        c, z = tw[h]
        wi = -z
        r2, i2 = re.reshape(-1, 2, h), im.reshape(-1, 2, h)
        ur, ui = r2[:, 0] + r2[:, 1], i2[:, 0] + i2[:, 1]
        dr, di = r2[:, 0] - r2[:, 1], i2[:, 0] - i2[:, 1]
        tr, ti = c * dr - wi * di, c * di + wi * dr
        re, im = np.stack([ur, tr], 1).reshape(N), np.stack([ui, ti], 1).reshape(N)
        h //= 2
    return re, im


def _inverse(re: np.ndarray, im: np.ndarray, tw) -> np.ndarray:
    N = re.shape[0]
    h = 1
    while h < N:
        c, z = tw[h]
        r2, i2 = re.reshape(-1, 2, h), im.reshape(-1, 2, h)
        tr, ti = c * r2[:, 1] - z * i2[:, 1], c * i2[:, 1] + z * r2[:, 1]
        re = np.stack([r2[:, 0] + tr, r2[:, 0] - tr], 1).reshape(N)
        im = np.stack([i2[:, 0] + ti, i2[:, 0] - ti], 1).reshape(N)
        h *= 2
    return re


_XOR = [np.arange(64) ^ t for t in (32, 16, 8, 4, 2, 1)]


def _sum(v: np.ndarray) -> np.float32:
    """SUM of the module: lane-strided partials in ascending index, then the xor tree"""
    n = v.shape[0]
    rows = np.zeros((n + 63) // 64 * 64, dtype=np.float32)
    rows[:n] = v
    rows = rows.reshape(-1, 64)
    p = np.zeros(64, dtype=np.float32)
    for r in rows:
        p = p + r
    for idx in _XOR:
        p = p + p[idx]
    return np.float32(p[0])


def _check_state(state: torch.Tensor) -> None:
    if state.dtype != torch.int32 or tuple(state.shape) != (STATE_WORDS,) or state.device.type != "cpu":
        raise ValueError(f"state must be a CPU int32 tensor of {STATE_WORDS} words, got {tuple(state.shape)} {state.dtype}")


def scan(samples, config: DenoiseConfig, state: Optional[torch.Tensor] = None,
         sample_rate: int = 24000) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """samples: (n,) fp32 on the host (a numpy array or a CPU tensor), n >= 0; state: what an earlier call returned (None: fresh)
    -> (out (n,) fp32: the suppressed samples, delayed by frame_samples, state after the samples, power_in (F,) fp32, power_out (F,)
    fp32) over the F frames the samples completed.  Neither `samples` nor `state` is modified.  Any split of the samples gives the
    bits of one call.  sample_rate does not enter the rule (frame_samples is in samples)."""
    x = samples.numpy() if isinstance(samples, torch.Tensor) else np.asarray(samples)
    if x.ndim != 1 or x.dtype != np.float32:
        raise ValueError(f"samples must be a 1-D fp32 array on the host, got {x.shape} {x.dtype}")
    N, H, learn = config.frame_samples, config.hop, config.learn_frames
    alpha, oma, track, ratio, creep, floor, eps, rN = (np.float32(v) for v in config.fparams())
    if state is None:
        state = fresh_state()
    _check_state(state)
    words = state.clone().numpy()
    fl = words.view(np.float32)
    n = int(x.shape[0])
    y = np.empty(n, dtype=np.float32)
    if n == 0:                                                               # as an idle slot of the launch: the row is not touched
        return torch.from_numpy(y), torch.from_numpy(words), torch.zeros(0), torch.zeros(0)
    frames, fill, learned = (int(words[k]) for k in (I_FRAMES, I_FILL, I_LEARNED))
    if not 0 <= fill < H:
        raise ValueError(f"the state's open hop holds {fill} samples, which is no part of a hop of {H}")
    sum_in, sum_out = np.float32(fl[I_SUM_IN]), np.float32(fl[I_SUM_OUT])
    raw, tail, hop = fl[O_RAW:O_RAW + N], fl[O_TAIL:O_TAIL + H], fl[O_HOP:O_HOP + H]          # views: updated in place
    nz, prev = fl[O_NZ:O_NZ + H + 1], fl[O_PREV:O_PREV + H + 1]
    win, rev, tw = _plan(N)
    own, mirror = rev[:H + 1], rev[N - np.arange(1, H)]
    one, zero, tiny = np.float32(1.0), np.float32(0.0), np.float32(TINY)
    pin, pout = [], []
    at = 0
    with np.errstate(under="ignore"):
        while at < n:
            m = min(H - fill, n - at)
            raw[H + fill:H + fill + m] = x[at:at + m]
            y[at:at + m] = hop[fill:fill + m]
            at, fill = at + m, fill + m
            if fill < H:
                break
            re, im = _forward(raw * win, np.zeros(N, dtype=np.float32), tw)
            br, bi = re[own], im[own]
            P = br * br + bi * bi
            P = np.where(P < tiny, zero, P)
            p_in = _sum(P)
            if p_in == 0:
                p_out, v = zero, np.zeros(N, dtype=np.float32)
            else:
                if learned < learn:
                    d = P - nz
                    d = d / np.float32(learned + 1)
                    nz[:] = nz + d
                    learned += 1
                else:
                    z = nz * creep
                    t = ratio * z
                    d = P - z
                    d = track * d
                    nz[:] = np.where(P < t, z + d, z)
                post = P / np.maximum(nz, eps)
                e = np.maximum(post - one, zero)
                prio = alpha * prev + oma * e
                G = np.maximum(prio / (one + prio), floor)
                g2 = G * G
                prev[:] = g2 * post
                p_out = _sum(g2 * P)
                gr, gi = G * br, G * bi
                re, im = np.empty(N, dtype=np.float32), np.empty(N, dtype=np.float32)
                re[own], im[own] = gr, gi
                re[mirror], im[mirror] = gr[1:H], -gi[1:H]
                v = (_inverse(re, im, tw) * rN) * win
                sum_in, sum_out = sum_in + p_in, sum_out + p_out
            hop[:] = tail + v[:H] if frames else zero
            tail[:] = v[H:]
            raw[:H] = raw[H:].copy()
            frames, fill = frames + 1, 0
            pin.append(p_in), pout.append(p_out)
    fl[I_SUM_IN], fl[I_SUM_OUT], fl[I_NZ_SUM] = sum_in, sum_out, _sum(nz)
    words[I_FRAMES], words[I_FILL], words[I_LEARNED] = frames, fill, learned
    return (torch.from_numpy(y), torch.from_numpy(words), torch.from_numpy(np.array(pin, dtype=np.float32)),
            torch.from_numpy(np.array(pout, dtype=np.float32)))


@dataclasses.dataclass(frozen=True)
class DenoiseReport:
    """What a caller reads of a session's suppressor, built from the header of its state row.

        frames, total_samples   whole frames computed; samples seen, the open hop's included
        learned, learning       frames that entered the initial noise estimate; whether it is still being formed
        power_in, power_out     the sums over all frames of the spectral power in front of and behind the gain
        attenuation_db          10 log10(power_in / power_out) (0 where either is 0)
        noise_power             SUM(Nz) at the last frame: the noise estimate over the bins, in the units of power_in per frame
        delay_samples           frame_samples: out[p] = y[p - delay_samples]
    """
    frames: int
    total_samples: int
    learned: int
    learning: bool
    power_in: float
    power_out: float
    attenuation_db: float
    noise_power: float
    delay_samples: int = 512
    sample_rate: int = 24000

    def seconds(self, k: int) -> float:
        """when frame k was computed: at its last sample"""
        return (int(k) + 1) * (self.delay_samples // 2) / self.sample_rate


def report(row: torch.Tensor, frame_samples: int = 512, sample_rate: int = 24000, learn_frames: int = 16) -> DenoiseReport:
    """the report of a state row or of its header (any device -- one copy to the host)"""
    head = row[:HEADER_WORDS].cpu()
    w, f = [int(v) for v in head.tolist()], [float(v) for v in head.view(torch.float32).tolist()]
    pi, po = f[I_SUM_IN], f[I_SUM_OUT]
    return DenoiseReport(frames=w[I_FRAMES], total_samples=w[I_FRAMES] * (int(frame_samples) // 2) + w[I_FILL], learned=w[I_LEARNED],
                         learning=w[I_LEARNED] < int(learn_frames), power_in=pi, power_out=po,
                         attenuation_db=10.0 * math.log10(pi / po) if pi > 0 and po > 0 else 0.0, noise_power=f[I_NZ_SUM],
                         delay_samples=int(frame_samples), sample_rate=int(sample_rate))


# ---------------------------------------------------------------------------------------------------- the launch
def max_frames(n_new: int, frame_samples: int) -> int:
    """the most frames n_new samples can complete, whatever the open hop holds: what a row of power_in / power_out must take"""
    hop = int(frame_samples) // 2
    return (int(n_new) + hop - 1) // hop


def denoise_items(samples: torch.Tensor, first: Sequence[int], n_new: Sequence[int], configs: Sequence[Optional[DenoiseConfig]],
                  state: torch.Tensor, power_in: torch.Tensor, power_out: torch.Tensor, transform: torch.Tensor,
                  table: Optional[torch.Tensor] = None) -> None:
    """all slots of a step in ONE launch (dmel_denoise_items).  samples: (S, width) fp32 CUDA with contiguous columns; slot s
    re-writes IN PLACE the n_new[s] samples at columns [first[s], first[s] + n_new[s]) of its row (0: the slot is idle, its rows are
    not touched, configs[s] may be None); no other column is written.  state: (S, STATE_WORDS) int32, contiguous, updated in place;
    power_in / power_out: (S, pitch) fp32, contiguous, pitch >= max_frames(n_new[s], N) for every s; the words behind the frames a
    row completed are not written.  transform: transform_table() on the device.  table: int32 device scratch of 16 * S words a
    caller that denoises every step keeps (default: allocated here).  Runs on the current stream."""
    _lib.require_cuda(samples, "samples")
    if samples.ndim != 2 or samples.dtype != torch.float32 or (samples.shape[1] > 1 and samples.stride(1) != 1):
        raise ValueError(f"samples must be an fp32 tensor (S, width) with contiguous columns, got {tuple(samples.shape)} {samples.dtype}")
    S, width = (int(v) for v in samples.shape)
    dev = samples.device
    if len(first) != S or len(n_new) != S or len(configs) != S:
        raise ValueError(f"{S} slots need {S} offsets, counts and configs, got {len(first)}, {len(n_new)} and {len(configs)}")
    if state.dtype != torch.int32 or tuple(state.shape) != (S, STATE_WORDS) or not state.is_contiguous() or state.device != dev:
        raise ValueError(f"state must be a contiguous int32 tensor ({S}, {STATE_WORDS}) on {dev}")
    for t, name in ((power_in, "power_in"), (power_out, "power_out")):
        if t.dtype != torch.float32 or t.ndim != 2 or t.shape[0] != S or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be a contiguous fp32 tensor ({S}, pitch) on {dev}")
    if power_in.shape[1] != power_out.shape[1]:
        raise ValueError("power_in and power_out must have one pitch")
    if transform.dtype != torch.float32 or tuple(transform.shape) != (TRANSFORM_WORDS,) or not transform.is_contiguous() or transform.device != dev:
        raise ValueError(f"transform must be transform_table() on {dev}: ({TRANSFORM_WORDS},) fp32")
    frames, learn, fp = [], [], []
    for s in range(S):
        n, f = int(n_new[s]), int(first[s])
        if n < 0 or (n and not 0 <= f <= width - n):
            raise ValueError(f"slot {s}: columns [{f}, {f + n}) are no part of a row of {width} samples")
        if n and configs[s] is None:
            raise ValueError(f"slot {s} has {n} samples and no config")
        cfg = configs[s] if n else None
        frames.append(cfg.frame_samples if cfg else 0)
        learn.append(cfg.learn_frames if cfg else 0)
        fp += cfg.fparams() if cfg else (0.0,) * 8
    if table is None:
        table = torch.empty(TABLE_WORDS * S, dtype=torch.int32, device=dev)
    elif table.dtype != torch.int32 or table.numel() < TABLE_WORDS * S or table.device != dev or not table.is_contiguous():
        raise ValueError(f"table must hold {TABLE_WORDS * S} contiguous int32 on {dev}")
    I64, I32 = C.c_int64 * S, C.c_int32 * S
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dmel_denoise_items(samples.data_ptr(), samples.stride(0), S, I64(*[int(v) for v in first]),
                                                 I64(*[int(v) for v in n_new]), I32(*frames), I32(*learn), (C.c_float * (8 * S))(*fp),
                                                 state.data_ptr(), power_in.data_ptr(), power_out.data_ptr(), int(power_in.shape[1]),
                                                 transform.data_ptr(), table.data_ptr(), _lib.stream_ptr()),
                   "denoise_items")
