"""Pools of independent live sessions served by ONE streaming step: EncodeSessions (VQGAN.encode_sessions, below) and DecodeSessions
(VQGAN.decode_sessions, at the end of the file).

StreamingEncoder(batch=B) is B streams in lockstep: one schedule, one origin, one (prev, next) row.  Microphones do not behave like that:
they start, stall and hang up on their own.  EncodeSessions keeps one EncodeSchedule, one origin and one sample tail PER SLOT and hands
the kernels one row per slot (dmel_stft_window_items_f32, dmel_wavenet_stream_step_items), so that any subset of the slots advances, each
by its own number of samples, in one STFT launch and one encoder launch.  Sessions whose sound cards do not run at the codec's rate
declare their own rate when they open; all of them, whatever their rates, are converted by one resample launch per step
(utils/resample.py: SessionResampler, dmel_resample_window_items_f32).  Sessions whose wire carries 16-bit PCM declare that too
(open(sample_format="s16")), and so do sessions whose wire is telephony's G.711 (open(sample_format="ulaw" | "alaw"), 8-bit codes,
usually at 8 kHz): the conversion is folded into the per-slot copy a pool makes anyway, one launch for all slots of a step
(utils/pcm.py, dmel_pcm_convert_items)."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Iterable, List, Mapping, Optional, Tuple

import torch

from .. import _lib
from ..utils import conceal as conceal_rule
from ..utils import crossfade, pcm
from ..utils import dtmf as dtmf_rule
from ..utils import echo as echo_rule
from ..utils import denoise as denoise_rule
from ..utils import level as level_rule
from ..utils import pace as pace_rule
from ..utils import shape as shape_rule
from ..utils import tones as tone_rule
from ..utils import voice as voice_rule
from .stream_park import ParkingPool, plain
from .stream_schedule import (DecodeGeometry, DecodeSchedule, EarlyDecodeSchedule, EncodeGeometry, EncodeSchedule, decode_capacity,
                              decode_live_window, decode_rebase, encode_live_window, encode_need_from, resample_max_outputs, session_rows)

_WIRE_DTYPES = {dt for name, (_, dt) in pcm.FORMATS.items() if name != "f32"}     # torch.int16, torch.uint8


class EncodeSessions(ParkingPool):
    """`slots` independent incremental encodes, each with the ids of encode() on its own finished clip.

        slot = pool.open()                                   # a free slot, fresh state; open(sample_rate=48000): a session at that rate;
                                                             # open(sample_format="s16", channels=2): stereo 16-bit frames (n, 2)
        ids = pool.push({slot: audio_1d, ...}, final=())     # one step for any subset of the open slots -> {slot: ids (G, m) int32}
        ids = pool.close(slot)                               # = push({slot: empty}, final=(slot,))[slot]

    Every named slot gets its own number of samples (0 is allowed, more than `max_push_samples` is refused); slots that are not named are
    idle in the step.  A slot in `final` ends with these samples: the step returns its remaining tokens, computed with the true end of
    its signal (reflection, zero padding, the floor of T // 4), and frees the slot.  The lookahead of StreamingEncoder applies per slot.

    Per step: one STFT launch over the new frames of all slots, one encoder step over the new columns of every level of all slots, and
    ONE quantiser call over all slots with new tokens, whatever the lengths of their feature windows and whether they end or go on: the
    windows are right-padded into one batch and passed with their lengths (quantizer.encode(z, lengths=): every layer sees each item's
    own end -- the depthwise k = 7 convolutions of the ConvNeXt blocks pad each item with its own zeros -- so a final slot's window,
    which ends at the true end of its signal, may sit in a longer batch).  A step whose windows all have one length -- the steady state
    of equal pushes -- makes the plain call, quantizer.encode(z), as it always did.

    State: buffers of (slots * G, C, cap) laid out like StreamingEncoder's, `cap` fixed at construction from `max_push_samples`; each slot
    has its own origin (the absolute frame in column 0 of ITS rows), its own s0 and sample tail; re-basing shifts one slot's columns
    only.  Memory grows neither with the length of a stream nor with the number of sessions served over time.

    Sample rates belong to SESSIONS, not to the pool: `sample_rates` declares the rates sessions may arrive at, open(sample_rate=r)
    starts one.  Such a slot takes its pushes in samples of ITS rate (max_push_samples bounds them in those samples) and its ids are
    the bits of encode(clip, len, sample_rate=r).  All slots of a step that need converting go through ONE resample launch, which
    writes straight behind each slot's carried sample tail; the STFT launch and the encoder step follow unchanged.  The rows and the
    capacity are sized from the most codec-rate samples one push can release over the declared rates (resample_max_outputs).  The
    constructor's own `sample_rate` only names the codec's rate, as before: a pool has no rate of its own.

    The sample format belongs to a session as well and sizes nothing: open(sample_format="s16") starts a session whose pushes are
    torch.int16 (16-bit signed PCM, in samples of its own rate as before) and whose ids are the bits of the same session opened as "f32"
    and fed pcm.float() / 32768 -- of encode(from_pcm16(clip), len[, sample_rate=r]).  In a step that names at least one s16 slot, ALL
    named slots with samples go through ONE dmel_pcm_convert_items launch (f32 slots as plain copies) that writes exactly where the
    per-slot copies of the float path write: behind the slot's sample tail, or behind its tail in the SessionResampler's rows; the
    resample launch, the STFT launch and the encoder step follow unchanged.  A step without an s16 slot takes the float path as it was.
    A push whose dtype does not match its slot's format is a ValueError.  open(sample_format="ulaw" | "alaw") starts a G.711 session
    the same way: its pushes are torch.uint8 codes, its ids the bits of the same session opened as "f32" and fed
    from_g711(clip, law) -- of encode(from_g711(clip, law), len, sample_rate=r); the one convert launch of the step decodes them
    (the companding rule of utils/pcm.py).  Out of scope: the lockstep StreamingEncoder and whole-clip encode() (callers have
    utils.pcm.from_pcm16 / from_g711), other formats (s24, s32, u8), dither.

    The channel count belongs to a session too and sizes nothing (the codec is mono): open(channels=c), 1 < c <= 8, starts a session
    whose pushes are contiguous INTERLEAVED frames (n, c) in the dtype of its format, n <= max_push_samples frames at its own rate.
    Its ids are the bits of the same session opened mono "f32" and fed the downmix of the channel rule of utils/pcm.py -- of
    encode(pcm.downmix(clip, format), len[, sample_rate=r]): every channel to f32 by its format's rule, the fp32 sum in channel order,
    one IEEE division by c (numpy.mean over the channel-first array, what librosa's to_mono computes).  open(channels=c, channel=k)
    encodes channel k alone: two sessions pushed the same stereo tensor with channel=0 and channel=1 are the two parties of a call
    recording.  A step that names at least one slot with a non-f32 format OR more than one channel takes the path above: ONE convert
    launch for all named slots with samples (dmel_pcm_convert_items_ch), the downmix inside it.  A step of mono f32 slots keeps the
    float path with no convert launch.  A 1-D or (1, n) push to a slot with channels, or an (n, c) push to a mono slot, is a
    ValueError.  Not served: weights, channel maps, more than 8 channels, planar (channel-first) pushes, the lockstep
    StreamingEncoder and whole-clip encode() (callers have utils.pcm.downmix).

    A session is not tied to its slot: snapshot(slots) gathers everything the named sessions own -- the live window of mel, of every
    level's history, of the skip sums and of the features (stream_schedule.encode_live_window: what a re-base in front of the next
    push would keep), the sample tail, the resampler tail, the counters -- with ONE dmel_stream_pack_items launch into one blob;
    drop(slot) frees a slot without flushing it; park(slots) is both; restore(snapshots) continues the sessions in free slots of
    this or another pool of the same codec (other slots, max_push_samples and capacity are fine) with ONE launch, each window at
    column 0 of its zeroed rows.  The ids of a parked and restored session are the bits of the uninterrupted one.  Refused with
    ValueError, no slot taken: the other kind, another geometry, width or depth, a rate the pool did not declare, a window or a
    tail that does not fit, an unknown format version.  Equal weights are the caller's contract (models/stream_park.py).

    A listening session can be asked what every conversational loop asks on each step -- is this person speaking, have they
    stopped, did they start while we talk -- without audio or mel reaching the host: a pool built with voice=True also serves
    sessions opened with open(voice=True | VoiceConfig), each with a detector of its own on the log-mel frames the STFT launch
    writes anyway (the rule, its state and its untuned defaults: utils/voice.py, which is also the host reference the pool is
    tested against bit for bit).  After the STFT launch of a step, ONE dmel_voice_items launch serves every named slot with
    detection that received frames, reading the step's temporary mel where it lies; a step without such a slot launches what it
    did.  The state is one row of n_mels + 8 words per slot (`voice`), zeroed with the slot's other rows, and travels with
    snapshot / restore as one more segment; push() returns what it returns and never syncs.  voice() -> {slot: VoiceReport} for
    every slot with detection that is open or ended in the most recent push, from ONE device-to-host copy of that table, the only
    sync and only when asked; voice_frames(slot) -> (flags, counts), device uint8 views of the frames of the slot's last push
    (flags: active | speaking << 1 after the frame; counts: the bands that stood out).  The detector sees the codec-rate mel, so
    rate, format and channels of the wire need nothing.  A pool built without voice=True allocates and launches exactly what it
    did, refuses open(voice=) and a snapshot that carries a detector; a session without detection in a voice pool snapshots to
    the bytes it always did.

    A session on a phone line can also be asked which keys its caller pressed: a pool built with dtmf=True serves sessions opened
    with open(dtmf=True | DtmfConfig), each with a DTMF detector of its own on the samples the step leaves in the slot's row anyway --
    at the codec's rate, as f32, behind the convert, downmix and resample launches, whatever the wire was (the rule, its state
    row and its caveats: utils/dtmf.py, which is also the host reference the pool is tested against bit for bit).  In front of
    the STFT launch of a step (which re-bases the sample rows), ONE dmel_dtmf_items launch serves every named slot with a detector
    that gained samples, over exactly the columns it gained, the resampler's flush of a final push included; a step without such
    a slot launches what it did.  The state is one row of 128 words per slot (`dtmf`: the open block's filter state, the debounce
    counters and a ring of the last 32 events), zeroed with the slot's other rows, and travels with snapshot / restore as one
    more segment; push() returns what it returns and never syncs.  dtmf() -> {slot: DtmfReport} for every slot with a detector that
    is open or ended in the most recent push, from ONE device-to-host copy of that table, the only sync and only when asked;
    dtmf_blocks(slot) -> (decided, pressed), device uint8 views of the blocks the slot's last push completed (key + 1, 0: none).
    Voice and DTMF are independent options of one pool.  A pool built without dtmf=True allocates and launches exactly what it
    did, refuses open(dtmf=) and a snapshot that carries a detector; a session without one snapshots to the bytes it always did.

    The wire delivers whatever level it likes -- a PSTN caller at -35 dBFS, a hot headset at -3 dBFS -- and the encoder was trained
    on clips peak-normalised to 0.95.  A pool built with level=True serves sessions opened with open(level=True | LevelConfig), each
    with an input leveller of its own: a causal block AGC with a meter and zero added latency on the same codec-rate samples (the
    rule, its state row and its caveats: utils/level.py, which is also the host reference the pool is tested against bit for bit).
    Unlike the detectors it CHANGES the samples the encoder sees.  Behind the DTMF launch of a step -- the detector reads the samples
    as received: a pool's DTMF reports do not change with level -- and in front of the STFT launch, ONE dmel_level_items launch
    re-writes in place exactly the columns every named slot with a leveller gained; a step without such a slot launches what it
    did.  The voice detector sees the levelled mel.  Contract: the ids of a levelled session are the bits of encode(y, len) with
    y = level.scan(x, config, sample_rate=codec rate)[0] and x the session's clip at the codec's rate (resample(from_wire(clip), r,
    codec rate)), however the audio was cut into pushes; the other sessions of the pool keep the bits of encode() of their clips.
    The state is one row of 16 words per slot (`level`), zeroed with the slot's other rows, and travels with snapshot / restore as
    one more segment; push() returns what it returns and never syncs.  levels() -> {slot: LevelReport} (gain, envelope, peaks,
    clamped samples, held blocks) for every slot with a leveller that is open or ended in the most recent push, from ONE
    device-to-host copy of that table, the only sync and only when asked; level_blocks(slot) -> (peaks, gains), device fp32 views
    of the blocks the slot's last push completed.  A pool built without level=True allocates and launches exactly what it did,
    refuses open(level=) and a snapshot that carries a leveller; a session without one snapshots to the bytes it always did.  Not
    served: look-ahead limiting, RMS or loudness (LUFS) metering, the lockstep StreamingEncoder and whole-clip encode() (callers
    have level.scan / level.level_items), output gain on decode pools, a DTMF detector that reads levelled samples.

    What the agent says into the line comes back through the hybrid or the speakerphone: its own keys are read by dtmf(), its own
    speech trips the voice detector, the leveller locks onto it.  A pool built with echo=True serves sessions opened with
    open(echo=True | EchoConfig), each with an echo canceller of its own: a block NLMS adaptive FIR of up to 2048 taps with zero
    added latency on the same codec-rate samples (the rule, its state row and its caveats: utils/echo.py, which is also the host
    reference the pool is tested against bit for bit).  push(audio, final, far={slot: (m,) f32 device tensor}) hands such a slot
    the far-end samples at the codec's rate -- naturally the codec-rate f32 audio of the decode session on the same call -- which
    have their own counter and may run up to far_room_samples ahead of the samples the slot had before the push; a slot may
    get far samples with an empty audio push, or audio with no far samples.  In front of the DTMF and leveller launches of a step, ONE dmel_echo_items
    launch appends every named slot's far samples to its history and re-writes in place exactly the columns the slot gained: the
    order of a step is convert, resample, echo, DTMF, level, STFT, so the DTMF detector and the leveller of an echo session see
    the cancelled samples; sessions without a canceller see what they saw, and a step without far or new samples for such a slot
    launches what it did.  Contract: the ids of an echo session are the bits of encode(e, len) with e = echo.scan(x, far,
    config)[0] over its codec-rate clip x, however both streams were cut (every far sample pushed no later than the sample that
    needs it); with a leveller as well, of encode(level.scan(e, ...)[0]); its DTMF report is dtmf.scan's over e.  The state is
    one row of 68112 words per slot (`echo`: counters and meters, the taps, the open block, a ring of far samples), zeroed with
    the slot's other rows; its first 2576 words and the live part of the ring travel with snapshot / restore as up to three more
    segments, the far samples queued ahead included; push() returns what it returns and never syncs.  echoes() -> {slot:
    EchoReport} (ERLE, adapted and frozen blocks, missing far samples) for every slot with a canceller that is open or ended in
    the most recent push, from ONE device-to-host copy of the rows' headers, the only sync and only when asked;
    echo_blocks(slot) -> (block_in, block_res), device fp32 views of the energies of the blocks the slot's last push completed.
    A pool built without echo=True allocates and launches exactly what it did, refuses open(echo=), push(far=) and a snapshot
    that carries a canceller; a session without one snapshots to the bytes it always did.  Not served: a residual suppressor,
    comfort noise, a bulk-delay search, stereo far ends, far streams at another rate or format, decode pools, the lockstep
    StreamingEncoder and whole-clip encode() (callers have echo.scan / echo.echo_items).

    Every option above assumes that the wire delivers every sample, and RTP does not.  A pool built with conceal=True serves
    sessions opened with open(conceal=True | ConcealConfig), each with a packet-loss concealment of its own: pitch waveform
    repetition with zero added latency on the same codec-rate samples (the rule, its state row and its caveats: utils/conceal.py,
    which is also the host reference the pool is tested against bit for bit).  push(audio, final, lost={slot: n}) says that n
    frames of the slot's WIRE (its rate; frames, not samples, for a session with channels) were lost in front of this push's
    samples for that slot; the slot is named in `audio` (an empty chunk is fine) and n + len(chunk) <= max_push_samples, so a longer
    hole is spread over steps.  The pool puts n frames of the format's silence in front of the chunk (f32 0.0, s16 0, mu-law 0xFF,
    A-law 0xD5), so the convert launch, the resampler, the schedule, the far alignment and every counter keep the true timeline;
    it records the wire range, maps it to the codec-rate samples it damages (conceal.damaged: through a resampler, every output
    whose filter window reads a lost frame) and keeps the part the resampler has not released for later steps.  In front of the
    echo launch of a step, ONE dmel_conceal_items launch serves every named concealing slot that gained samples -- on steps
    without a loss too: the ring needs the samples -- and re-writes in place the damaged columns and the recovery behind them:
    the order of a step is convert, resample, conceal, echo, DTMF, denoise, level, STFT.  Contract: the ids of a concealing session are the
    bits of encode(y, len) with y = conceal.scan(x0, ranges, config)[0], x0 the silence-filled stream at the codec's rate and
    ranges = conceal.damaged(lost wire ranges, rate, codec rate), however audio and losses were cut into pushes; with echo, DTMF
    or a leveller their rules apply to y in the order above.  The state is one row of 4112 words per slot (`conceal`: counters
    and a ring of the last 4096 output samples), zeroed with the slot's other rows; it travels with snapshot / restore as one more
    segment, the damaged ranges still pending as plain integers in the meta; push() returns what it returns and never syncs.
    concealed() -> {slot: ConcealReport} (lost and muted samples, runs, the longest, the last period and score) for every
    concealing slot that is open or ended in the most recent push, from ONE device-to-host copy of the rows' headers, the only
    sync and only when asked; conceal_onsets(slot) -> (periods, scores), device views of the onsets of the slot's last push.  A
    pool built without conceal=True allocates and launches exactly what it did, refuses open(conceal=), push(lost=) and a
    snapshot that carries the option; a session without it snapshots to the bytes it always did.  Not served: jitter buffers and
    reordering, reading RTP sequence numbers, FEC / RED, decode pools, losses in the far stream, the lockstep StreamingEncoder and
    whole-clip encode() (callers have conceal.scan / conceal.conceal_items).

    Nothing above removes a steady background -- a fan, a car cabin, line hiss -- and the leveller brings it up with the speech.  A
    pool built with denoise=True serves sessions opened with open(denoise=True | DenoiseConfig), each with a noise suppressor of its
    own: an overlap-add spectral gain over a learnt and slowly tracked noise power per bin (the rule, its constant table, its state
    row and its caveats: utils/denoise.py, which is also the host reference the pool is tested against bit for bit).  Behind the DTMF
    launch of a step -- the detector reads the samples as received: a pool's DTMF reports do not change with denoise -- and in front
    of the leveller, ONE dmel_denoise_items launch re-writes in place exactly the columns every named slot with a suppressor gained;
    a step without such a slot launches what it did.  IT IS THE FIRST OPTION WITH A DELAY: the samples the leveller, the STFT and the
    voice detector see are the suppressed ones delayed by the config's frame_samples (512 by default, 21.3 ms at 24 kHz), the
    session's length and timeline are kept, its first frame_samples samples are zeros and its last frame_samples input samples are
    not emitted (push that many zeros in front of `final` to have them).  Contract: the ids of a denoising session are the bits of
    encode(y, len) with y = denoise.scan(x, config)[0] and x the session's clip at the codec's rate; with a leveller as well, of
    encode(level.scan(y, ...)[0]).  The state is one row of 3092 words per slot (`denoise`), zeroed with the slot's other rows, and
    travels with snapshot / restore as one more segment; push() returns what it returns and never syncs.  denoised() -> {slot:
    DenoiseReport} (frames, learning, power in and out, attenuation, noise power) for every slot with a suppressor that is open or
    ended in the most recent push, from ONE device-to-host copy of the rows' headers, the only sync and only when asked;
    denoise_frames(slot) -> (power_in, power_out), device fp32 views of the frames the slot's last push completed.  A pool built
    without denoise=True allocates and launches exactly what it did, refuses open(denoise=) and a snapshot that carries a suppressor;
    a session without one snapshots to the bytes it always did.  Not served: decode pools and the far stream, the lockstep
    StreamingEncoder and whole-clip encode() (callers have denoise.scan / denoise.denoise_items), a residual echo suppressor driven
    by the canceller, comfort noise, transient noise, delay compensation of the reports of the other options.

    Only encoders the one-launch streaming kernel takes (residual channels in (32, 80], no condition, no output projection,
    dilations <= 8, fp32): anything else is refused at construction.

    All launches are on the current stream, so nothing new meets DESIGN section 7's unexplained wrong-frame behaviour of the STFT next to
    convolutions.  The warning of StreamingEncoder stands: a caller that runs sessions next to convolutions on ANOTHER STREAM of the same
    process -- a streaming decode, for example -- must call dmel_stft_set_exclusive_cu(1) first, exactly as pipeline.CodecLanes does."""

    def __init__(self, codec, slots: int, max_push_samples: int = 7680, sample_rate: Optional[int] = None,
                 sample_rates: Iterable[int] = (), voice: bool = False, dtmf: bool = False, level: bool = False,
                 echo: bool = False, far_room_samples: int = 24000, conceal: bool = False, denoise: bool = False):
        enc, tr = codec.encoder, codec.encode_mel_transform
        if sample_rate is not None and int(sample_rate) != int(tr.sample_rate):
            raise NotImplementedError(f"sessions run at the codec's own rate ({tr.sample_rate} Hz); resample in front (StreamResampler), "
                                      f"or declare the sessions' rates (sample_rates=) and open each one at its own (open(sample_rate=))")
        if int(slots) <= 0 or int(max_push_samples) <= 0:
            raise ValueError("slots and max_push_samples must be positive")
        L, Cres = len(enc.residual_layers), enc.residual_channels
        cycle = enc.dilation_cycle or 0
        why = None
        if enc.condition_channels or enc.output_projection is not None:
            why = "it is conditioned or has an output projection"
        elif not 32 < Cres <= 80:
            why = f"{Cres} residual channels are outside (32, 80]"
        elif cycle > 4:
            why = f"dilation cycle {cycle} reaches dilations above 8"
        elif enc.input_projection is not None and enc.input_channels > 16:
            why = f"{enc.input_channels} input channels exceed 16"
        elif L > 32:
            why = f"{L} blocks exceed 32"
        elif getattr(enc, "_precision", 0):
            why = "its precision is not fp32"
        if why:
            raise NotImplementedError(f"encode sessions need an encoder the one-launch streaming kernel takes: {why}")
        self.codec, self.S, self.G = codec, int(slots), codec.dmel_groups
        self.L, self.C = L, Cres
        dils = tuple(2 ** (i % cycle) if cycle else 1 for i in range(L))
        self.maxdil = max(dils)
        self.geo = EncodeGeometry(hop=tr.hop_length, n_fft=tr.n_fft, dilations=dils,
                                  downsample_factor=tuple(codec.quantizer.downsample_factor))
        self.n_mels = tr.n_mels
        self.max_push = int(max_push_samples)
        self.codec_rate = int(tr.sample_rate)
        self.sample_rates = tuple(sorted({int(r) for r in sample_rates} - {self.codec_rate}))
        if any(r <= 0 for r in self.sample_rates):
            raise ValueError("sample rates must be positive")
        # the most samples at the codec's rate one push can put into a slot's row, over the declared rates
        self.codec_push = max([self.max_push] + [resample_max_outputs(r, self.codec_rate, self.max_push) for r in self.sample_rates])
        g = self.geo
        left, right = g.quant_context
        F = g.factor
        # Columns a slot holds: from the oldest one a later step reads -- the quantiser's left context in front of the next token, which
        # lies at most `hold` frames behind the newest frame -- to the newest frame of a push (+ 1 for the hop's remainder, + the frames
        # only the end of the signal releases).  Twice that, so that a slot is re-based once in several pushes and not in every one.
        hold = g.encoder_context + right + 1 + F * ((left + F - 1) // F) + F
        self.want_max = hold + self.codec_push // g.hop + 1 + (g.n_fft - g.pad + g.hop - 1) // g.hop
        self.cap = (2 * self.want_max + 31) // 32 * 32
        self.width = g.n_fft + self.codec_push        # samples per row: a tail is shorter than one window
        self._init_slots(self.codec_rate, "sample_rates", self.max_push)          # the per-slot resamplers in front, if any rate was declared
        self.s0 = [0] * self.S
        self.tail = [0] * self.S                      # valid samples in the slot's row
        self.pick = [-1] * self.S                     # the channel of its pushes the slot encodes; -1: their mean
        if not isinstance(voice, bool):
            raise ValueError(f"voice must be a bool (a session's config goes to open(voice=)), got {voice!r}")
        self.voice_on = voice                         # the pool keeps detector rows: sessions may open with voice=
        if voice and not 1 <= self.n_mels <= voice_rule.MAX_MELS:
            raise NotImplementedError(f"voice detection takes at most {voice_rule.MAX_MELS} mel bands, the transform has {self.n_mels}")
        self.vcfg: List[Optional[voice_rule.VoiceConfig]] = [None] * self.S      # the slot's detector (None: none)
        self._voice_n = [0] * self.S                  # frames of the slot's last push: the valid bytes of its flags / counts rows
        self._voice_ended: set = set()                # slots with detection that ended in the most recent push
        if not isinstance(dtmf, bool):
            raise ValueError(f"dtmf must be a bool (a session's config goes to open(dtmf=)), got {dtmf!r}")
        self.dtmf_on = dtmf                           # the pool keeps DTMF detector rows: sessions may open with dtmf=
        self.dcfg: List[Optional[dtmf_rule.DtmfConfig]] = [None] * self.S        # the slot's DTMF detector (None: none)
        self._dtmf_n = [0] * self.S                   # blocks the slot's last push completed: the valid bytes of its decided / pressed rows
        self._dtmf_ended: set = set()                 # slots with a DTMF detector that ended in the most recent push
        if not isinstance(level, bool):
            raise ValueError(f"level must be a bool (a session's config goes to open(level=)), got {level!r}")
        self.level_on = level                         # the pool keeps leveller rows: sessions may open with level=
        self.lcfg: List[Optional[level_rule.LevelConfig]] = [None] * self.S      # the slot's leveller (None: none)
        self._level_n = [0] * self.S                  # blocks the slot's last push completed: the valid words of its peak / gain rows
        self._level_ended: set = set()                # slots with a leveller that ended in the most recent push
        if not isinstance(echo, bool):
            raise ValueError(f"echo must be a bool (a session's config goes to open(echo=)), got {echo!r}")
        if isinstance(far_room_samples, bool) or not isinstance(far_room_samples, int) or not 0 <= far_room_samples <= echo_rule.MAX_AHEAD:
            raise ValueError(f"far_room_samples must be an integer in [0, {echo_rule.MAX_AHEAD}], got {far_room_samples!r}")
        self.echo_on, self.far_room = echo, far_room_samples         # the pool keeps canceller rows: sessions may open with echo=
        self.ecfg: List[Optional[echo_rule.EchoConfig]] = [None] * self.S        # the slot's canceller (None: none)
        self._far = [0] * self.S                      # far samples pushed to the slot (its own samples: sched[s].samples)
        self._echo_n = [0] * self.S                   # blocks the slot's last push completed: the valid words of its in / res rows
        self._echo_ended: set = set()                 # slots with a canceller that ended in the most recent push
        if not isinstance(conceal, bool):
            raise ValueError(f"conceal must be a bool (a session's config goes to open(conceal=)), got {conceal!r}")
        self.conceal_on = conceal                     # the pool keeps concealment rows: sessions may open with conceal=
        self.ccfg: List[Optional[conceal_rule.ConcealConfig]] = [None] * self.S  # the slot's concealment (None: none)
        self._lost: List[List[Tuple[int, int]]] = [[] for _ in range(self.S)]    # damaged codec-rate ranges not released yet, absolute
        self._lost_open = [False] * self.S            # the slot's newest sample was a lost one: a range at its next sample is no onset
        self._conceal_n = [0] * self.S                # onsets of the slot's last push: the valid words of its period / score rows
        self._conceal_ended: set = set()              # concealing slots that ended in the most recent push
        if not isinstance(denoise, bool):
            raise ValueError(f"denoise must be a bool (a session's config goes to open(denoise=)), got {denoise!r}")
        self.denoise_on = denoise                     # the pool keeps suppressor rows: sessions may open with denoise=
        self.ncfg: List[Optional[denoise_rule.DenoiseConfig]] = [None] * self.S  # the slot's noise suppressor (None: none)
        self._denoise_n = [0] * self.S                # frames the slot's last push completed: the valid words of its power rows
        self._denoise_ended: set = set()              # slots with a suppressor that ended in the most recent push

    def tokens_emitted(self, slot: int) -> int:
        self._check_open(slot)
        return self.sched[slot].tokens

    def open(self, sample_rate: Optional[int] = None, sample_format: str = "f32", channels: int = 1,
             channel: Optional[int] = None, voice=None, dtmf=None, level=None, echo=None, conceal=None, denoise=None) -> int:
        """take a free slot: fresh schedule, state zeroed before its first push.  sample_rate: the rate this session's pushes arrive
        at, one of the declared `sample_rates` (None: the codec's).  sample_format: "f32", "s16" for torch.int16 pushes (16-bit
        signed PCM, x / 32768), or "ulaw" / "alaw" for torch.uint8 pushes (G.711 codes).  channels: 1 .. 8; above 1 the pushes are
        interleaved frames (n, channels), downmixed to their mean, or to channel `channel` of them (0 .. channels - 1).  voice: True
        (the defaults of utils/voice.py) or a VoiceConfig starts the session's voice-activity detector, on a pool built with
        voice=True.  dtmf: True (the defaults of utils/dtmf.py) or a DtmfConfig starts the session's DTMF key detector, on a pool
        built with dtmf=True.  level: True (the defaults of utils/level.py) or a LevelConfig starts the session's input leveller, on
        a pool built with level=True: the encoder then sees the levelled samples.  echo: True (the defaults of utils/echo.py) or an
        EchoConfig starts the session's echo canceller, on a pool built with echo=True: push(far=) then takes its far-end samples.
        conceal: True (the defaults of utils/conceal.py) or a ConcealConfig starts the session's packet-loss concealment, on a pool
        built with conceal=True: push(lost=) then takes the frames its wire lost.  denoise: True (the defaults of utils/denoise.py)
        or a DenoiseConfig starts the session's noise suppressor, on a pool built with denoise=True: the leveller and the encoder
        then see the suppressed samples, delayed by the config's frame_samples.
        Raises when every slot is taken; a refused open takes no slot."""
        rate = self.codec_rate if sample_rate is None else int(sample_rate)
        pick = self._check_wire(rate, sample_format, channels, channel)
        cfg = self._check_voice(voice_rule.as_config(voice))
        keys = self._check_dtmf(dtmf_rule.as_config(dtmf))
        lev = self._check_level(level_rule.as_config(level))
        ec = self._check_echo(echo_rule.as_config(echo))
        cc = self._check_conceal(conceal_rule.as_config(conceal))
        nc = self._check_denoise(denoise_rule.as_config(denoise))
        s = self._first_free()
        self._occupy(s, EncodeSchedule(self.geo), 0, rate, sample_format, channels)
        self.s0[s], self.tail[s], self.pick[s] = 0, 0, pick
        self.vcfg[s], self._voice_n[s] = cfg, 0
        self.dcfg[s], self._dtmf_n[s] = keys, 0
        self.lcfg[s], self._level_n[s] = lev, 0
        self.ecfg[s], self._echo_n[s], self._far[s] = ec, 0, 0
        self.ccfg[s], self._conceal_n[s], self._lost[s], self._lost_open[s] = cc, 0, [], False
        self.ncfg[s], self._denoise_n[s] = nc, 0
        return s

    def _check_voice(self, cfg: Optional[voice_rule.VoiceConfig]) -> Optional[voice_rule.VoiceConfig]:
        """a session's detector config, refused here for open() and for restore() alike"""
        if cfg is not None:
            if not self.voice_on:
                raise ValueError("voice on a pool built without voice=True: it has no detector rows")
            cfg.window(self.n_mels)
        return cfg

    def _check_dtmf(self, cfg: Optional[dtmf_rule.DtmfConfig]) -> Optional[dtmf_rule.DtmfConfig]:
        """a session's DTMF config, refused here for open() and for restore() alike"""
        if cfg is not None:
            if not self.dtmf_on:
                raise ValueError("dtmf on a pool built without dtmf=True: it has no detector rows")
            cfg.block(self.codec_rate)
        return cfg

    def _check_level(self, cfg: Optional[level_rule.LevelConfig]) -> Optional[level_rule.LevelConfig]:
        """a session's leveller config, refused here for open() and for restore() alike"""
        if cfg is not None:
            if not self.level_on:
                raise ValueError("level on a pool built without level=True: it has no leveller rows")
            cfg.block(self.codec_rate)
        return cfg

    def _check_echo(self, cfg: Optional[echo_rule.EchoConfig]) -> Optional[echo_rule.EchoConfig]:
        """a session's canceller config, refused here for open() and for restore() alike"""
        if cfg is not None and not self.echo_on:
            raise ValueError("echo on a pool built without echo=True: it has no canceller rows")
        return cfg

    def _check_conceal(self, cfg: Optional[conceal_rule.ConcealConfig]) -> Optional[conceal_rule.ConcealConfig]:
        """a session's concealment config, refused here for open() and for restore() alike"""
        if cfg is not None:
            if not self.conceal_on:
                raise ValueError("conceal on a pool built without conceal=True: it has no concealment rows")
            cfg.samples(self.codec_rate)
        return cfg

    def _check_denoise(self, cfg: Optional[denoise_rule.DenoiseConfig]) -> Optional[denoise_rule.DenoiseConfig]:
        """a session's suppressor config, refused here for open() and for restore() alike"""
        if cfg is not None and not self.denoise_on:
            raise ValueError("denoise on a pool built without denoise=True: it has no suppressor rows")
        return cfg

    def _validate_lost(self, audio: Mapping[int, torch.Tensor], lost) -> Dict[int, int]:
        """the lost frames of a step, refused like the audio: before any state changes and before any device call -> {slot: n > 0}"""
        if lost is None:
            return {}
        if not self.conceal_on:
            raise ValueError("lost frames on a pool built without conceal=True: it has no concealment rows")
        out = {}
        for slot, n in lost.items():
            if slot not in audio:
                raise ValueError(f"slot {slot!r} has lost frames but is not among the pushed slots (an empty push is fine)")
            self._check_open(slot)
            if self.ccfg[slot] is None:
                raise ValueError(f"slot {slot} has lost frames and no concealment (open(conceal=))")
            if isinstance(n, bool) or not isinstance(n, int) or n < 0:
                raise ValueError(f"slot {slot}: lost frames are a count, an integer >= 0, got {n!r}")
            if n:
                out[slot] = n
        return out

    def _validate_far(self, audio: Mapping[int, torch.Tensor], far) -> Dict[int, torch.Tensor]:
        """the far samples of a step, refused like the audio: before any state changes and before any device call"""
        if far is None:
            return {}
        if not self.echo_on:
            raise ValueError("far samples on a pool built without echo=True: it has no canceller rows")
        dev = next(iter(audio.values())).device
        out = {}
        for slot, x in far.items():
            if slot not in audio:
                raise ValueError(f"slot {slot!r} has far samples but is not among the pushed slots (an empty push is fine)")
            if self.ecfg[slot] is None:
                raise ValueError(f"slot {slot} has far samples and no canceller (open(echo=))")
            if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.ndim != 1:
                raise ValueError(f"slot {slot}: far samples are a 1-D fp32 tensor at the codec's rate, got "
                                 f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__} {getattr(x, 'dtype', '')}")
            if x.device != dev:
                raise ValueError(f"slot {slot}: far samples on {x.device}, audio on {dev}")
            ahead = self._far[slot] + x.shape[0] - self.sched[slot].samples
            if ahead > self.far_room:
                raise ValueError(f"slot {slot}: {x.shape[0]} far samples would run {ahead} ahead of the {self.sched[slot].samples} samples "
                                 f"the slot has seen before this push: far_room_samples = {self.far_room}")
            if x.shape[0]:
                out[slot] = x.contiguous()
        return out

    def _validate(self, audio: Mapping[int, torch.Tensor], final, lost: Optional[Mapping[int, int]] = None) -> Dict[int, torch.Tensor]:
        """everything that can be refused, before any state changes and before any device call; lost: {slot: frames of silence the
        pool will put in front of the slot's chunk}, which count as pushed"""
        if not audio:
            raise ValueError("push needs at least one slot")
        out, lost = {}, lost or {}
        for slot, a in audio.items():
            self._check_open(slot)
            c = self.ch[slot]
            if c > 1:
                if a.ndim != 2 or a.shape[1] != c or not a.is_contiguous():
                    raise ValueError(f"slot {slot} was opened with channels={c}: expected contiguous interleaved frames (n, {c}), got "
                                     f"{tuple(a.shape)} (stride {a.stride()})")
            else:
                if a.ndim == 2 and a.shape[0] == 1:
                    a = a[0]
                if a.ndim != 1:
                    raise ValueError(f"slot {slot}: expected mono audio (n,) or (1, n), got {tuple(a.shape)}")
            if a.shape[0] + lost.get(slot, 0) > self.max_push:
                raise ValueError(f"slot {slot}: a push of {a.shape[0]} samples" + (f" behind {lost[slot]} lost ones" if slot in lost else "")
                                 + f" exceeds max_push_samples = {self.max_push}")
            # the push's dtype is the dtype of the slot's format; an f32 slot refuses the dtypes of the other formats
            if (a.dtype in _WIRE_DTYPES) if self.fmt[slot] == "f32" else (a.dtype != pcm.FORMATS[self.fmt[slot]][1]):
                raise ValueError(f"slot {slot} was opened with sample_format={self.fmt[slot]!r}: a {a.dtype} push does not match")
            out[slot] = a
        for slot in final:
            if slot not in audio:
                raise ValueError(f"slot {slot} is in `final` but not among the pushed slots")
            pushed = out[slot].shape[0] + lost.get(slot, 0)
            total = self.sched[slot].samples + pushed
            if self._converts(slot):                  # its length at the codec's rate, as encode(..., sample_rate=) converts it
                rs = self.rs.sched[slot]
                total = rs.total_outputs(rs.samples + pushed)
            if total <= self.geo.pad:
                raise ValueError(f"slot {slot}: the stream is {total} samples long: encode() needs more than the reflect pad {self.geo.pad}")
        for slot, a in out.items():
            _lib.require_cuda(a, "audio")
        return out

    # -- buffers -----------------------------------------------------------------------------------------------------------
    def _allocate(self, dev) -> None:
        N = self.S * self.G
        rows = self.S * (2 * (self.L + 1) + 1)
        self.buf = dict(mel=torch.zeros(self.S, self.n_mels, self.cap, dtype=torch.float32, device=dev),
                        hist=torch.zeros(self.L + 1, N, self.C, self.cap, dtype=torch.float32, device=dev),
                        skip=torch.zeros(N, self.C, self.cap, dtype=torch.float32, device=dev),
                        feat=torch.zeros(N, self.C, self.cap, dtype=torch.float32, device=dev),
                        samples=torch.zeros(self.S, self.width, dtype=torch.float32, device=dev),
                        # dmel_wavenet_stream_step_items: the scratch of _ex (2 N C cap floats, N int64) and the row table behind it
                        scratch=torch.empty(2 * N * self.C * self.cap + 2 * N + rows, dtype=torch.float32, device=dev),
                        stft_tab=torch.empty(4 * self.S, dtype=torch.int64, device=dev),
                        pcm_tab=torch.empty(4 * self.S, dtype=torch.int64, device=dev))
        if self.voice_on:                             # dmel_voice_items: a state row per slot, the step's flags and counts (a step's
            #                                           frames fit the slot's cap columns), 12 words per slot of the table
            self.buf.update(voice=torch.zeros(self.S, self.n_mels + voice_rule.STATE_INTS, dtype=torch.int32, device=dev),
                            voice_flags=torch.zeros(self.S, self.cap, dtype=torch.uint8, device=dev),
                            voice_counts=torch.zeros(self.S, self.cap, dtype=torch.uint8, device=dev),
                            voice_tab=torch.empty(voice_rule.TABLE_WORDS * self.S, dtype=torch.int32, device=dev))

        if self.dtmf_on:                              # dmel_dtmf_items: a state row per slot, the step's decisions (a push completes at most
            #                                           codec_push // 32 + 1 blocks of 32 samples or more), 20 words per slot of the table
            pitch = self.codec_push // dtmf_rule.MIN_BLOCK + 2
            self.buf.update(dtmf=torch.zeros(self.S, dtmf_rule.STATE_WORDS, dtype=torch.int32, device=dev),
                            dtmf_decided=torch.zeros(self.S, pitch, dtype=torch.uint8, device=dev),
                            dtmf_pressed=torch.zeros(self.S, pitch, dtype=torch.uint8, device=dev),
                            dtmf_tab=torch.empty(dtmf_rule.TABLE_WORDS * self.S, dtype=torch.int32, device=dev))
        if self.level_on:                             # dmel_level_items: a state row per slot, the step's block peaks and gains (the pitch
            #                                           as above), 16 words per slot of the table
            pitch = self.codec_push // level_rule.MIN_BLOCK + 2
            self.buf.update(level=torch.zeros(self.S, level_rule.STATE_WORDS, dtype=torch.int32, device=dev),
                            level_peak=torch.zeros(self.S, pitch, dtype=torch.float32, device=dev),
                            level_gain=torch.zeros(self.S, pitch, dtype=torch.float32, device=dev),
                            level_tab=torch.empty(level_rule.TABLE_WORDS * self.S, dtype=torch.int32, device=dev))
        if self.echo_on:                              # dmel_echo_items: a state row per slot (the ring of far samples in it), the step's
            #                                           block energies (blocks of 16 samples or more), 16 words per slot of the table
            pitch = self.codec_push // echo_rule.MIN_BLOCK + 2
            self.buf.update(echo=torch.zeros(self.S, echo_rule.ROW_WORDS, dtype=torch.int32, device=dev),
                            echo_in=torch.zeros(self.S, pitch, dtype=torch.float32, device=dev),
                            echo_res=torch.zeros(self.S, pitch, dtype=torch.float32, device=dev),
                            echo_tab=torch.empty(echo_rule.TABLE_WORDS * self.S, dtype=torch.int32, device=dev))
        if self.conceal_on:                           # dmel_conceal_items: a state row per slot (the ring of its output in it), the step's
            #                                           onsets (at most one per lost range), 48 words per slot of the table
            self.buf.update(conceal=torch.zeros(self.S, conceal_rule.ROW_WORDS, dtype=torch.int32, device=dev),
                            conceal_period=torch.zeros(self.S, conceal_rule.MAX_RANGES, dtype=torch.int32, device=dev),
                            conceal_score=torch.zeros(self.S, conceal_rule.MAX_RANGES, dtype=torch.float32, device=dev),
                            conceal_tab=torch.empty(conceal_rule.TABLE_WORDS * self.S, dtype=torch.int32, device=dev))
        if self.denoise_on:                           # dmel_denoise_items: a state row per slot, the step's frame powers (a push completes
            #                                           at most codec_push // 32 + 1 frames of hop 32 or more), the constant transform table
            pitch = self.codec_push // (denoise_rule.MIN_FRAME // 2) + 2
            self.buf.update(denoise=torch.zeros(self.S, denoise_rule.STATE_WORDS, dtype=torch.int32, device=dev),
                            denoise_in=torch.zeros(self.S, pitch, dtype=torch.float32, device=dev),
                            denoise_out=torch.zeros(self.S, pitch, dtype=torch.float32, device=dev),
                            denoise_transform=denoise_rule.transform_table().to(dev),
                            denoise_tab=torch.empty(denoise_rule.TABLE_WORDS * self.S, dtype=torch.int32, device=dev))

    def _prepare_slot(self, s: int) -> None:
        super()._prepare_slot(s)
        if self.voice_on:
            self.buf["voice"][s].zero_()              # the fresh detector state (not one of _slot_views: a re-base does not shift it)
        if self.dtmf_on:
            self.buf["dtmf"][s].zero_()               # the fresh DTMF state
        if self.level_on:
            self.buf["level"][s].zero_()              # the fresh leveller state
        if self.echo_on:
            self.buf["echo"][s].zero_()               # the fresh canceller state, the ring with it
        if self.conceal_on:
            self.buf["conceal"][s].zero_()            # the fresh concealment state, the ring with it
        if self.denoise_on:
            self.buf["denoise"][s].zero_()            # the fresh suppressor state: windows, overlap tail and noise estimate

    def _slot_views(self, s: int):
        b, G = self.buf, self.G
        return (b["mel"][s], b["hist"][:, s * G:(s + 1) * G], b["skip"][s * G:(s + 1) * G], b["feat"][s * G:(s + 1) * G])

    def _rebase(self, s: int, st) -> None:
        """make room for the frames of step `st` in slot s: drop the columns nothing reads again and shift that slot's rows"""
        if st.frames[1] - self.origin[s] <= self.cap:
            return
        need_from = encode_need_from(self.geo, st.prev[self.L], st.tokens[0])     # the lower end of encode_live_window in front of the step
        shift, keep = need_from - self.origin[s], max(0, st.frames[0] - need_from)
        if st.frames[1] - need_from > self.cap:       # cannot happen: cap covers twice the widest window (want_max)
            raise RuntimeError(f"slot {s}: {st.frames[1] - need_from} columns do not fit the capacity {self.cap}")
        for v in self._slot_views(s):
            v[..., :keep] = v[..., shift:shift + keep].clone()
        self.origin[s] = need_from

    # -- a session leaves its slot and comes back (models/stream_park.py) ----------------------------------------------------
    _park_kind, _park_windowed, _own_rate_of, _resamples_in = "encode", ("mel", "hist.", "skip", "feat"), "codec's", True
    _live_window = staticmethod(encode_live_window)

    def _park_meta(self, s: int) -> dict:
        meta = dict(super()._park_meta(s), s0=self.s0[s], tail=self.tail[s], channel=None if self.pick[s] < 0 else self.pick[s])
        if self.vcfg[s] is not None:                  # only a session with detection carries the key: the others' snapshots are unchanged
            meta["voice"] = self.vcfg[s].as_dict()
        if self.dcfg[s] is not None:                  # likewise
            meta["dtmf"] = self.dcfg[s].as_dict()
        if self.lcfg[s] is not None:                  # likewise
            meta["level"] = self.lcfg[s].as_dict()
        if self.ecfg[s] is not None:                  # likewise, and the far samples pushed (the slot's own are the schedule's)
            meta["echo"], meta["echo_far"] = self.ecfg[s].as_dict(), self._far[s]
        if self.ccfg[s] is not None:                  # likewise, and the damaged ranges the resampler has not released yet
            meta["conceal"], meta["conceal_lost"] = self.ccfg[s].as_dict(), [list(r) for r in self._lost[s]]
            meta["conceal_open"] = self._lost_open[s]
        if self.ncfg[s] is not None:                  # likewise
            meta["denoise"] = self.ncfg[s].as_dict()
        return meta

    def _park_schedule(self, meta: Mapping) -> EncodeSchedule:
        return EncodeSchedule.from_state(self.geo, meta["schedule"])

    def _park_shapes(self, meta: Mapping) -> List[Tuple[str, int, int]]:
        W, rows, rs = meta["window"][1] - meta["window"][0], self.G * self.C, meta["resampler"]
        shapes = ([("mel", self.n_mels, W)] + [(f"hist.{l}", rows, W) for l in range(self.L + 1)] + [("skip", rows, W), ("feat", rows, W),
                  ("samples", 1, meta["tail"]), ("resampler", 1, rs["fill"] if rs else 0)])
        if meta.get("voice") is not None:             # the detector row; a session that has seen no frame owns the zeroed row: nothing
            shapes.append(("voice", 1, self.n_mels + voice_rule.STATE_INTS if meta["schedule"]["frames"] > 0 else 0))
        if meta.get("dtmf") is not None:              # the DTMF row; a session that has seen no sample owns the zeroed row: nothing
            shapes.append(("dtmf", 1, dtmf_rule.STATE_WORDS if meta["schedule"]["samples"] > 0 else 0))
        if meta.get("level") is not None:             # the leveller row, likewise
            shapes.append(("level", 1, level_rule.STATE_WORDS if meta["schedule"]["samples"] > 0 else 0))
        if meta.get("echo") is not None:              # the canceller row without its ring, then the ring's live samples in two runs
            T, F = meta["schedule"]["samples"], meta["echo_far"]
            shapes.append(("echo", 1, echo_rule.STATE_WORDS if T > 0 or F > 0 else 0))
            pieces = echo_rule.ring_pieces(*echo_rule.far_live(self._park_echo(meta), T, F))
            shapes += [(f"echo_far.{i}", 1, n) for i, (_, n) in enumerate(pieces)]
        if meta.get("conceal") is not None:           # the concealment row, its ring included; a session without a sample owns the zeroed one
            shapes.append(("conceal", 1, conceal_rule.ROW_WORDS if meta["schedule"]["samples"] > 0 else 0))
        if meta.get("denoise") is not None:           # the suppressor row, likewise
            shapes.append(("denoise", 1, denoise_rule.STATE_WORDS if meta["schedule"]["samples"] > 0 else 0))
        return shapes

    def _park_rows(self, s: int) -> Dict[str, torch.Tensor]:
        b, G = self.buf, self.G
        rows = {"mel": b["mel"][s], "skip": b["skip"][s * G:(s + 1) * G], "feat": b["feat"][s * G:(s + 1) * G],
                "samples": b["samples"][s:s + 1]}
        for l in range(self.L + 1):
            rows[f"hist.{l}"] = b["hist"][l, s * G:(s + 1) * G]             # the slot's G rows are contiguous: one piece per level
        if self.rs is not None and self.rs.buf is not None:
            rows["resampler"] = self.rs.buf["rows"][s:s + 1]
        if self.voice_on:
            rows["voice"] = b["voice"][s:s + 1]
        if self.dtmf_on:
            rows["dtmf"] = b["dtmf"][s:s + 1]
        if self.level_on:
            rows["level"] = b["level"][s:s + 1]
        if self.echo_on:
            rows["echo"] = b["echo"][s:s + 1]
        if self.conceal_on:
            rows["conceal"] = b["conceal"][s:s + 1]
        if self.denoise_on:
            rows["denoise"] = b["denoise"][s:s + 1]
        return rows

    def _park_places(self, s: int):
        """the runs of the ring a canceller's snapshot carries begin where the session's counters say: not cached"""
        places = super()._park_places(s)
        if self.ecfg[s] is None:
            return places
        ptr, pitch, _ = places["echo"]
        pieces = echo_rule.ring_pieces(*echo_rule.far_live(self.ecfg[s], self.sched[s].samples, self._far[s]))
        return dict(places, **{f"echo_far.{i}": (ptr + 4 * (echo_rule.O_FAR + col), pitch, False) for i, (col, _) in enumerate(pieces)})

    def _park_widths(self):
        return ("n_mels", self.n_mels), ("codec_rate", self.codec_rate)

    def _park_voice(self, meta: Mapping) -> Optional[voice_rule.VoiceConfig]:
        """the detector config a snapshot carries (None: none); ValueError where it is no config"""
        if meta.get("voice") is None:
            return None
        try:
            return voice_rule.VoiceConfig.from_dict(meta["voice"])
        except TypeError as e:
            raise ValueError(f"the voice config of the snapshot is not a VoiceConfig: {e}") from None

    def _park_dtmf(self, meta: Mapping) -> Optional[dtmf_rule.DtmfConfig]:
        """the DTMF config a snapshot carries (None: none); ValueError where it is no config"""
        if meta.get("dtmf") is None:
            return None
        try:
            return dtmf_rule.DtmfConfig.from_dict(meta["dtmf"])
        except TypeError as e:
            raise ValueError(f"the dtmf config of the snapshot is not a DtmfConfig: {e}") from None

    def _park_level(self, meta: Mapping) -> Optional[level_rule.LevelConfig]:
        """the leveller config a snapshot carries (None: none); ValueError where it is no config"""
        if meta.get("level") is None:
            return None
        try:
            return level_rule.LevelConfig.from_dict(meta["level"])
        except TypeError as e:
            raise ValueError(f"the level config of the snapshot is not a LevelConfig: {e}") from None

    def _park_echo(self, meta: Mapping) -> Optional[echo_rule.EchoConfig]:
        """the canceller config a snapshot carries (None: none); ValueError where it is no config or its far count is no count"""
        if meta.get("echo") is None:
            return None
        try:
            cfg = echo_rule.EchoConfig.from_dict(meta["echo"])
        except TypeError as e:
            raise ValueError(f"the echo config of the snapshot is not an EchoConfig: {e}") from None
        F = meta.get("echo_far")
        if isinstance(F, bool) or not isinstance(F, int) or F < 0:
            raise ValueError(f"the far samples of the snapshot's canceller are no count: {F!r}")
        return cfg

    def _park_conceal(self, meta: Mapping):
        """(the concealment config a snapshot carries (None: none), its pending damaged ranges, whether its newest sample was lost);
        ValueError where it is no config or the ranges are no sorted, separate ranges behind what the session has released"""
        if meta.get("conceal") is None:
            return None, [], False
        try:
            cfg = conceal_rule.ConcealConfig.from_dict(meta["conceal"])
        except TypeError as e:
            raise ValueError(f"the conceal config of the snapshot is not a ConcealConfig: {e}") from None
        raw, at, ranges = meta.get("conceal_lost"), meta["schedule"]["samples"], []
        ok = isinstance(raw, (list, tuple)) and all(isinstance(r, (list, tuple)) and len(r) == 2 and all(
            isinstance(v, int) and not isinstance(v, bool) for v in r) for r in raw)
        for lo, hi in raw if ok else ():
            ok = ok and at <= lo < hi
            at = hi + 1
            ranges.append((lo, hi))
        if not ok or not isinstance(meta.get("conceal_open"), bool):
            raise ValueError(f"conceal_lost of the snapshot is no list of sorted, separate [lo, hi) behind the {meta['schedule']['samples']} "
                             f"samples the session has released: {raw!r} (conceal_open: {meta.get('conceal_open')!r})")
        return cfg, ranges, meta["conceal_open"]

    def _park_denoise(self, meta: Mapping) -> Optional[denoise_rule.DenoiseConfig]:
        """the suppressor config a snapshot carries (None: none); ValueError where it is no config"""
        if meta.get("denoise") is None:
            return None
        try:
            return denoise_rule.DenoiseConfig.from_dict(meta["denoise"])
        except TypeError as e:
            raise ValueError(f"the denoise config of the snapshot is not a DenoiseConfig: {e}") from None

    def _park_fits(self, meta: Mapping, sc: EncodeSchedule) -> None:
        g, (lo, hi) = self.geo, meta["window"]
        room = self.codec_push // g.hop + 1 + (g.n_fft - g.pad + g.hop - 1) // g.hop
        if hi - lo + room > self.cap:
            raise ValueError(f"a window of {hi - lo} frames and one maximal push ({room} frames) do not fit the capacity {self.cap}")
        if not 0 <= meta["tail"] <= self.width - self.codec_push:
            raise ValueError(f"a sample tail of {meta['tail']} samples and one maximal push do not fit a row of {self.width} samples")
        self._check_voice(self._park_voice(meta))
        self._check_dtmf(self._park_dtmf(meta))
        self._check_level(self._park_level(meta))
        if self._check_echo(self._park_echo(meta)) is not None and meta["echo_far"] - meta["schedule"]["samples"] > self.far_room:
            raise ValueError(f"{meta['echo_far']} far samples against {meta['schedule']['samples']} samples of the session do not fit "
                             f"far_room_samples = {self.far_room}")
        self._check_conceal(self._park_conceal(meta)[0])
        self._check_denoise(self._park_denoise(meta))

    def _park_adopt(self, s: int, meta: Mapping) -> None:
        super()._park_adopt(s, meta)
        self.s0[s], self.tail[s], self.pick[s] = meta["s0"], meta["tail"], -1 if meta["channel"] is None else meta["channel"]
        self.vcfg[s], self._voice_n[s] = self._park_voice(meta), 0
        self.dcfg[s], self._dtmf_n[s] = self._park_dtmf(meta), 0
        self.lcfg[s], self._level_n[s] = self._park_level(meta), 0
        self.ecfg[s], self._echo_n[s], self._far[s] = self._park_echo(meta), 0, meta.get("echo_far", 0)
        self.ccfg[s], self._lost[s], self._lost_open[s] = self._park_conceal(meta)
        self._conceal_n[s] = 0
        self.ncfg[s], self._denoise_n[s] = self._park_denoise(meta), 0

    # -- one step ----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def push(self, audio: Mapping[int, torch.Tensor], final: Iterable[int] = (),
             far: Optional[Mapping[int, torch.Tensor]] = None, lost: Optional[Mapping[int, int]] = None) -> Dict[int, torch.Tensor]:
        """audio: {slot: (n,) samples, n >= 0}; final: slots that end with these samples; far: {slot: (m,) f32 far-end samples at the
        codec's rate, m >= 0} for pushed slots with a canceller (a pool built with echo=True); lost: {slot: frames of the slot's wire
        that were lost in front of these samples} for pushed concealing slots (a pool built with conceal=True)
        -> {slot: ids (G, m) int32, m >= 0}"""
        final = set(final)
        lost = self._validate_lost(audio, lost)
        audio = self._validate(audio, final, lost)
        far = self._validate_far(audio, far)
        if lost:
            audio = self._fill_lost(audio, lost)
        dev = next(iter(audio.values())).device
        self._ensure_buffers(dev)
        converted, placed = self._place(audio)
        released = self._resample(converted, final, placed)
        tails = list(self.tail) if self.dtmf_on or self.level_on or self.echo_on or self.conceal_on or self.denoise_on else None
        steps = self._intake(audio, released, placed, final)
        with torch.cuda.device(dev):
            if self.conceal_on:
                self._conceal(steps, final, tails)
            if self.echo_on:
                self._echo(steps, final, tails, far)
            if self.dtmf_on:
                self._dtmf(steps, final, tails)
            if self.denoise_on:
                self._denoise(steps, final, tails)
            if self.level_on:
                self._level(steps, final, tails)
            mel = self._stft(steps, dev)
            if self.voice_on:
                self._voice(steps, final, mel)
            self._wavenet(steps)
            out = self._quantise(steps, dev)
        self._release(final)
        return out

    def _place(self, audio) -> Tuple[Dict[int, torch.Tensor], bool]:
        """the wire's format and channels: a step that names an s16, a G.711 or a multi-channel slot puts ALL its chunks in place with
        ONE convert launch (which downmixes on the way), each where the float path's per-slot copy would put it -- behind the slot's
        resampler tail or behind its sample tail.  -> ({slot: what the resample launch takes for it}, whether the chunks are placed)"""
        b = self.buf
        converted = {s: a for s, a in audio.items() if self._converts(s)}
        placed = any(self._wired(s) for s in audio)
        if placed:
            converted = self.rs.destinations({s: a.shape[0] for s, a in converted.items()}) if converted else {}
            moves = [((a.to(torch.float32) if self.fmt[s] == "f32" else a).contiguous(),
                      converted[s] if s in converted else b["samples"][s, self.tail[s]:self.tail[s] + a.shape[0]], s)
                     for s, a in audio.items() if a.shape[0]]
            if moves:
                pcm.convert_items([x for x, _, _ in moves], [y for _, y, _ in moves], table=b["pcm_tab"],
                                  src_formats=[self.fmt[s] for _, _, s in moves], src_channels=[self.ch[s] for _, _, s in moves],
                                  src_pick=[self.pick[s] for _, _, s in moves])
        return converted, placed

    def _resample(self, converted, final, placed: bool) -> Dict[int, int]:
        """the sound cards' rates: ONE launch converts every slot that needs it, straight behind its sample tail -> {slot: samples released}"""
        if not converted:
            return {}
        return self.rs.push(converted, final & set(converted), out=self.buf["samples"], out_off=self.tail, placed=placed)

    def _intake(self, audio, released, placed: bool, final) -> dict:
        """every named slot's new samples behind its tail (the float path's copy, where neither launch above placed them) and its
        schedule stepped -> {slot: its step}"""
        steps = {}
        for s, a in audio.items():
            if self._fresh[s]:
                self._prepare_slot(s)
            if s in released:
                n = released[s]
            else:
                n = a.shape[0]
                if n and not placed:
                    self.buf["samples"][s, self.tail[s]:self.tail[s] + n] = a
            self.tail[s] += n
            steps[s] = self.sched[s].step(n, s in final)
        return steps

    def _stft(self, steps, dev) -> Optional[torch.Tensor]:
        """STFT: the new frames of every slot, each from its own sample tail (re-based first), into the slot's mel columns; the
        samples no later frame reads leave the tail -> the launch's (S, n_mels, tmax) output, slot s's new frames at its columns
        [0, frames[1] - frames[0]) (None: no slot had a frame)"""
        b, geo, S = self.buf, self.geo, self.S
        I64 = C.c_int64 * S
        n_frames = [0] * S
        for s, st in steps.items():
            if st.frames[1] > 0:
                self._rebase(s, st)
            n_frames[s] = st.frames[1] - st.frames[0]
        tmax = max(n_frames)
        if not tmax:
            return None
        from ..torch_ops import _stft_plan
        sp = self.codec.encode_mel_transform.spectrogram
        plan = _stft_plan(dev, sp.sample_rate, sp.n_fft, sp.win_length, sp.hop_length, sp.num_mels, float(sp.f_min or 0.0),
                          float(sp.f_max) if sp.f_max else 0.0)
        mel = torch.empty(S, self.n_mels, tmax, dtype=torch.float32, device=dev)
        first = [steps[s].frames[0] if s in steps else 0 for s in range(S)]
        total = [steps[s].total_length if s in steps else -1 for s in range(S)]
        _lib.check(_lib.lib().dmel_stft_window_items_f32(plan, b["samples"].data_ptr(), self.width, self.width, I64(*self.s0),
                                                         I64(*self.tail), None, mel.data_ptr(), None, S, I64(*first), I64(*n_frames),
                                                         I64(*total), b["stft_tab"].data_ptr(), _lib.stream_ptr()), "stft_window_items")
        for s, st in steps.items():
            f0, f1 = st.frames
            if f1 > f0:
                o = self.origin[s]
                b["mel"][s, :, f0 - o:f1 - o] = mel[s, :, :f1 - f0]
                drop = max(0, f1 * geo.hop - geo.pad) - self.s0[s]
                if drop > 0:
                    keep = self.tail[s] - drop
                    row = b["samples"][s]
                    row[:keep] = row[drop:drop + keep] if drop >= keep else row[drop:drop + keep].clone()
                    self.s0[s], self.tail[s] = self.s0[s] + drop, keep
        return mel

    def _voice(self, steps, final, mel: Optional[torch.Tensor]) -> None:
        """voice activity: ONE launch over the new frames of every named slot with detection, read from the STFT launch's own output"""
        self._voice_ended = {s for s in final if self.vcfg[s] is not None}
        counts = [0] * self.S
        for s, st in steps.items():
            if self.vcfg[s] is not None:
                counts[s] = self._voice_n[s] = st.frames[1] - st.frames[0]
        if mel is None or not any(counts):
            return
        b = self.buf
        voice_rule.voice_items(mel, counts, self.vcfg, b["voice"], b["voice_flags"], b["voice_counts"], table=b["voice_tab"])

    def _voice_slots(self) -> List[int]:
        return [s for s in range(self.S) if self.vcfg[s] is not None and (self.sched[s] is not None or s in self._voice_ended)]

    def voice(self) -> Dict[int, voice_rule.VoiceReport]:
        """{slot: VoiceReport} of every slot with detection that is open or ended in the most recent push: ONE device-to-host copy of
        the detector table (the only sync of the detector, and only here).  A slot that has not been pushed to reports no frames."""
        slots = self._voice_slots()
        live = [s for s in slots if not self._fresh[s]] if self.buf is not None else []
        table = self.buf["voice"].cpu() if live else None
        zero = voice_rule.fresh_state(self.n_mels)
        return {s: voice_rule.report(table[s] if s in live else zero, self.geo.hop, self.codec_rate) for s in slots}

    def voice_frames(self, slot: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(flags, counts) of the frames of the slot's last push: device uint8 views (n,), valid until the slot's next push.  flags:
        active | speaking << 1 (the state after the frame); counts: the bands of the window that stood out of their floors"""
        if not isinstance(slot, int) or slot not in self._voice_slots():
            raise ValueError(f"slot {slot!r} has no voice detection (open(voice=)) or is neither open nor ended in the last push")
        if self.buf is None or self._fresh[slot]:
            empty = torch.empty(0, dtype=torch.uint8, device=self._device())
            return empty, empty.clone()
        n = self._voice_n[slot]
        return self.buf["voice_flags"][slot, :n], self.buf["voice_counts"][slot, :n]

    def _dtmf(self, steps, final, tails: List[int]) -> None:
        """DTMF keys: ONE launch over the samples every named slot with a detector gained in this step -- columns [tail before,
        tail after) of its row, whichever of the copy, the convert launch and the resample launch put them there -- in front of the
        STFT phase, which re-bases the rows"""
        self._dtmf_ended = {s for s in final if self.dcfg[s] is not None}
        first, n_new = [0] * self.S, [0] * self.S
        for s, st in steps.items():
            if self.dcfg[s] is not None:
                first[s], n_new[s] = tails[s], self.tail[s] - tails[s]
                N = self.dcfg[s].block(self.codec_rate)
                self._dtmf_n[s] = st.samples // N - (st.samples - n_new[s]) // N
        if not any(n_new):
            return
        b = self.buf
        dtmf_rule.dtmf_items(b["samples"], first, n_new, self.dcfg, b["dtmf"], b["dtmf_decided"], b["dtmf_pressed"],
                             sample_rate=self.codec_rate, table=b["dtmf_tab"])

    def _dtmf_slots(self) -> List[int]:
        return [s for s in range(self.S) if self.dcfg[s] is not None and (self.sched[s] is not None or s in self._dtmf_ended)]

    def dtmf(self) -> Dict[int, dtmf_rule.DtmfReport]:
        """{slot: DtmfReport} of every slot with a DTMF detector that is open or ended in the most recent push: ONE device-to-host
        copy of the detector table (the only sync of the detector, and only here).  A slot that has not been pushed to reports
        no sample."""
        slots = self._dtmf_slots()
        live = [s for s in slots if not self._fresh[s]] if self.buf is not None else []
        table = self.buf["dtmf"].cpu() if live else None
        zero = dtmf_rule.fresh_state()
        return {s: dtmf_rule.report(table[s] if s in live else zero, self.dcfg[s].block(self.codec_rate), self.codec_rate) for s in slots}

    def dtmf_blocks(self, slot: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(decided, pressed) of the blocks the slot's last push completed: device uint8 views (n,), valid until the slot's next
        push.  decided: the key + 1 the block decided (0: none); pressed: the key + 1 held after the block"""
        if not isinstance(slot, int) or slot not in self._dtmf_slots():
            raise ValueError(f"slot {slot!r} has no DTMF detector (open(dtmf=)) or is neither open nor ended in the last push")
        if self.buf is None or self._fresh[slot]:
            empty = torch.empty(0, dtype=torch.uint8, device=self._device())
            return empty, empty.clone()
        n = self._dtmf_n[slot]
        return self.buf["dtmf_decided"][slot, :n], self.buf["dtmf_pressed"][slot, :n]

    def _fill_lost(self, audio: Dict[int, torch.Tensor], lost: Mapping[int, int]) -> Dict[int, torch.Tensor]:
        """the lost frames of a step take their place in the timeline: n frames of the format's silence in front of the slot's chunk,
        and the wire range they cover, mapped to the codec-rate samples it damages, joins the slot's pending ranges"""
        audio = dict(audio)
        for s, n in lost.items():
            a = audio[s]
            quiet = torch.full((n,) + tuple(a.shape[1:]), conceal_rule.SILENCE[self.fmt[s]], dtype=a.dtype, device=a.device)
            audio[s] = torch.cat((quiet, a))
            at = self.rs.sched[s].samples if self._converts(s) else self.sched[s].samples       # wire frames seen so far
            new = conceal_rule.damaged([(at, at + n)], self.rate[s], self.codec_rate)
            # a released output had its whole window in hand before the loss arrived
            assert all(lo >= self.sched[s].samples for lo, _ in new), (new, self.sched[s].samples)
            self._lost[s] = conceal_rule.damaged(self._lost[s] + new, self.codec_rate, self.codec_rate)
        return audio

    def _conceal(self, steps, final, tails: List[int]) -> None:
        """concealment: ONE launch takes the samples every named concealing slot gained in this step -- columns [tail before, tail
        after) of its row -- through its rule and re-writes in place the damaged ones and the recovery behind them, in front of the
        echo, DTMF and leveller launches, which read them concealed.  The part of a damaged range the step released leaves the
        slot's pending ranges; the rest waits for the samples"""
        self._conceal_ended = {s for s in final if self.ccfg[s] is not None}
        first, n_new, ranges = [0] * self.S, [0] * self.S, [[] for _ in range(self.S)]
        for s, st in steps.items():
            if self.ccfg[s] is None:
                continue
            first[s], n_new[s] = tails[s], self.tail[s] - tails[s]
            self._conceal_n[s] = 0
            if not n_new[s]:
                continue
            a, b = st.samples - n_new[s], st.samples                          # the absolute samples of the step
            mine = [(max(lo, a) - a, min(hi, b) - a) for lo, hi in self._lost[s] if lo < b]
            self._lost[s] = [(max(lo, b), hi) for lo, hi in self._lost[s] if hi > b]
            ranges[s] = mine
            self._conceal_n[s] = len(mine) - (1 if mine and mine[0][0] == 0 and self._lost_open[s] else 0)
            self._lost_open[s] = bool(mine) and mine[-1][1] == n_new[s]
        for s in self._conceal_ended:                 # what lies behind the end of a stream damages nothing
            self._lost[s] = []
        if not any(n_new):
            return
        b = self.buf
        conceal_rule.conceal_items(b["samples"], first, n_new, ranges, self.ccfg, b["conceal"], b["conceal_period"], b["conceal_score"],
                                   sample_rate=self.codec_rate, table=b["conceal_tab"])

    def _conceal_slots(self) -> List[int]:
        return [s for s in range(self.S) if self.ccfg[s] is not None and (self.sched[s] is not None or s in self._conceal_ended)]

    def concealed(self) -> Dict[int, conceal_rule.ConcealReport]:
        """{slot: ConcealReport} of every concealing slot that is open or ended in the most recent push: ONE device-to-host copy of
        the headers of the concealment rows (the only sync of the option, and only here).  A slot that has not been pushed to
        reports no sample."""
        slots = self._conceal_slots()
        live = [s for s in slots if not self._fresh[s]] if self.buf is not None else []
        table = self.buf["conceal"][:, :conceal_rule.HEADER_WORDS].cpu() if live else None
        zero = torch.zeros(conceal_rule.HEADER_WORDS, dtype=torch.int32)
        return {s: conceal_rule.report(table[s] if s in live else zero, self.codec_rate) for s in slots}

    def conceal_onsets(self, slot: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(periods, scores) of the onsets of the slot's last push: device views (n,), int32 and fp32, valid until the slot's next
        push.  periods: the lag repeated from each onset on (0: none, the run is silence); scores: its normalised correlation energy"""
        if not isinstance(slot, int) or slot not in self._conceal_slots():
            raise ValueError(f"slot {slot!r} has no concealment (open(conceal=)) or is neither open nor ended in the last push")
        if self.buf is None or self._fresh[slot]:
            return (torch.empty(0, dtype=torch.int32, device=self._device()), torch.empty(0, dtype=torch.float32, device=self._device()))
        n = self._conceal_n[slot]
        return self.buf["conceal_period"][slot, :n], self.buf["conceal_score"][slot, :n]

    def _echo(self, steps, final, tails: List[int], far: Mapping[int, torch.Tensor]) -> None:
        """echo: ONE launch appends the step's far samples to the history of every named slot with a canceller and re-writes in place
        the samples it gained -- columns [tail before, tail after) of its row -- in front of the DTMF and leveller launches, which
        read them cancelled"""
        self._echo_ended = {s for s in final if self.ecfg[s] is not None}
        first, n_new, chunks = [0] * self.S, [0] * self.S, [None] * self.S
        for s, st in steps.items():
            if self.ecfg[s] is not None:
                first[s], n_new[s], chunks[s] = tails[s], self.tail[s] - tails[s], far.get(s)
                N = self.ecfg[s].block_samples
                self._echo_n[s] = st.samples // N - (st.samples - n_new[s]) // N
                self._far[s] += 0 if chunks[s] is None else chunks[s].shape[0]
        if not any(n_new) and not any(c is not None for c in chunks):
            return
        b = self.buf
        echo_rule.echo_items(b["samples"], first, n_new, chunks, self.ecfg, b["echo"], b["echo_in"], b["echo_res"], table=b["echo_tab"])

    def _echo_slots(self) -> List[int]:
        return [s for s in range(self.S) if self.ecfg[s] is not None and (self.sched[s] is not None or s in self._echo_ended)]

    def echoes(self) -> Dict[int, echo_rule.EchoReport]:
        """{slot: EchoReport} of every slot with a canceller that is open or ended in the most recent push: ONE device-to-host copy
        of the headers of the canceller rows (the only sync of the canceller, and only here).  A slot that has not been pushed to
        reports no sample."""
        slots = self._echo_slots()
        live = [s for s in slots if not self._fresh[s]] if self.buf is not None else []
        table = self.buf["echo"][:, :echo_rule.HEADER_WORDS].cpu() if live else None
        zero = torch.zeros(echo_rule.HEADER_WORDS, dtype=torch.int32)
        return {s: echo_rule.report(table[s] if s in live else zero, self.ecfg[s].block_samples, self.codec_rate) for s in slots}

    def echo_blocks(self, slot: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(block_in, block_res) of the blocks the slot's last push completed: device fp32 views (n,), valid until the slot's next
        push.  block_in: the energy sum d^2 of the block as received; block_res: sum e^2, what the canceller left of it"""
        if not isinstance(slot, int) or slot not in self._echo_slots():
            raise ValueError(f"slot {slot!r} has no echo canceller (open(echo=)) or is neither open nor ended in the last push")
        if self.buf is None or self._fresh[slot]:
            empty = torch.empty(0, dtype=torch.float32, device=self._device())
            return empty, empty.clone()
        n = self._echo_n[slot]
        return self.buf["echo_in"][slot, :n], self.buf["echo_res"][slot, :n]

    def _level(self, steps, final, tails: List[int]) -> None:
        """input level: ONE launch re-writes in place the samples every named slot with a leveller gained in this step -- columns
        [tail before, tail after) of its row -- behind the DTMF launch, which reads them as received, and in front of the STFT
        phase, which reads them levelled and re-bases the rows"""
        self._level_ended = {s for s in final if self.lcfg[s] is not None}
        first, n_new = [0] * self.S, [0] * self.S
        for s, st in steps.items():
            if self.lcfg[s] is not None:
                first[s], n_new[s] = tails[s], self.tail[s] - tails[s]
                N = self.lcfg[s].block(self.codec_rate)
                self._level_n[s] = st.samples // N - (st.samples - n_new[s]) // N
        if not any(n_new):
            return
        b = self.buf
        level_rule.level_items(b["samples"], first, n_new, self.lcfg, b["level"], b["level_peak"], b["level_gain"],
                               sample_rate=self.codec_rate, table=b["level_tab"])

    def _level_slots(self) -> List[int]:
        return [s for s in range(self.S) if self.lcfg[s] is not None and (self.sched[s] is not None or s in self._level_ended)]

    def levels(self) -> Dict[int, level_rule.LevelReport]:
        """{slot: LevelReport} of every slot with a leveller that is open or ended in the most recent push: ONE device-to-host copy
        of the leveller table (the only sync of the leveller, and only here).  A slot that has not been pushed to reports no
        sample."""
        slots = self._level_slots()
        live = [s for s in slots if not self._fresh[s]] if self.buf is not None else []
        table = self.buf["level"].cpu() if live else None
        zero = level_rule.fresh_state()
        return {s: level_rule.report(table[s] if s in live else zero, self.lcfg[s].block(self.codec_rate), self.codec_rate,
                                     self.lcfg[s].initial_gain) for s in slots}

    def level_blocks(self, slot: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(peaks, gains) of the blocks the slot's last push completed: device fp32 views (n,), valid until the slot's next push.
        peaks: the raw peak of the block; gains: the gain the block after it ramps to"""
        if not isinstance(slot, int) or slot not in self._level_slots():
            raise ValueError(f"slot {slot!r} has no leveller (open(level=)) or is neither open nor ended in the last push")
        if self.buf is None or self._fresh[slot]:
            empty = torch.empty(0, dtype=torch.float32, device=self._device())
            return empty, empty.clone()
        n = self._level_n[slot]
        return self.buf["level_peak"][slot, :n], self.buf["level_gain"][slot, :n]

    def _denoise(self, steps, final, tails: List[int]) -> None:
        """noise suppression: ONE launch re-writes in place the samples every named slot with a suppressor gained in this step --
        columns [tail before, tail after) of its row -- behind the DTMF launch, which reads them as received, and in front of the
        leveller and the STFT phase, which read them suppressed (and delayed by the slot's frame)"""
        self._denoise_ended = {s for s in final if self.ncfg[s] is not None}
        first, n_new = [0] * self.S, [0] * self.S
        for s, st in steps.items():
            if self.ncfg[s] is not None:
                first[s], n_new[s] = tails[s], self.tail[s] - tails[s]
                H = self.ncfg[s].hop
                self._denoise_n[s] = st.samples // H - (st.samples - n_new[s]) // H
        if not any(n_new):
            return
        b = self.buf
        denoise_rule.denoise_items(b["samples"], first, n_new, self.ncfg, b["denoise"], b["denoise_in"], b["denoise_out"],
                                   b["denoise_transform"], table=b["denoise_tab"])

    def _denoise_slots(self) -> List[int]:
        return [s for s in range(self.S) if self.ncfg[s] is not None and (self.sched[s] is not None or s in self._denoise_ended)]

    def denoised(self) -> Dict[int, denoise_rule.DenoiseReport]:
        """{slot: DenoiseReport} of every slot with a suppressor that is open or ended in the most recent push: ONE device-to-host
        copy of the headers of the suppressor rows (the only sync of the suppressor, and only here).  A slot that has not been
        pushed to reports no sample."""
        slots = self._denoise_slots()
        live = [s for s in slots if not self._fresh[s]] if self.buf is not None else []
        table = self.buf["denoise"][:, :denoise_rule.HEADER_WORDS].cpu() if live else None
        zero = torch.zeros(denoise_rule.HEADER_WORDS, dtype=torch.int32)
        return {s: denoise_rule.report(table[s] if s in live else zero, self.ncfg[s].frame_samples, self.codec_rate,
                                       self.ncfg[s].learn_frames) for s in slots}

    def denoise_frames(self, slot: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(power_in, power_out) of the frames the slot's last push completed: device fp32 views (n,), valid until the slot's next
        push.  power_in: the sum of the bin powers of the frame as received; power_out: the same behind the gain"""
        if not isinstance(slot, int) or slot not in self._denoise_slots():
            raise ValueError(f"slot {slot!r} has no noise suppressor (open(denoise=)) or is neither open nor ended in the last push")
        if self.buf is None or self._fresh[slot]:
            empty = torch.empty(0, dtype=torch.float32, device=self._device())
            return empty, empty.clone()
        n = self._denoise_n[slot]
        return self.buf["denoise_in"][slot, :n], self.buf["denoise_out"][slot, :n]

    def _wavenet(self, steps) -> None:
        """encoder WaveNet: every level of every slot advances to its own new frontier"""
        if not any(st.next != st.prev for st in steps.values()):
            return
        b, codec, G, S = self.buf, self.codec, self.G, self.S
        prev, nxt, org = session_rows(S, steps, self.origin)
        rows = C.c_int64 * (S * (self.L + 1))
        x = b["mel"].data_ptr() if codec.encoder.input_projection is not None else None
        if x is None:
            for s, st in steps.items():
                o = self.origin[s]
                b["hist"][0][s * G:(s + 1) * G, :, st.prev[0] - o:st.next[0] - o] = \
                    b["mel"][s].view(G, -1, self.cap)[:, :, st.prev[0] - o:st.next[0] - o]
        _lib.check(_lib.lib().dmel_wavenet_stream_step_items(codec.encoder.native(), x, b["hist"].data_ptr(), b["skip"].data_ptr(), None,
                                                             b["feat"].data_ptr(), b["scratch"].data_ptr(), S * G, self.cap, rows(*prev),
                                                             rows(*nxt), None, G, (C.c_int64 * S)(*org), _lib.stream_ptr()),
                   "wavenet_stream_step_items")

    def _quantise(self, steps, dev) -> Dict[int, torch.Tensor]:
        """quantiser: ONE call over every slot with new tokens, whatever the lengths of their windows, cropped per slot"""
        b, codec, G = self.buf, self.codec, self.G
        out, members = {}, []
        for s, st in steps.items():
            if st.tokens[1] > st.tokens[0]:
                members.append(s)
            else:
                out[s] = torch.empty(G, 0, dtype=torch.int32, device=dev)
        if members:
            wins = []
            for s in members:
                (lo, hi), o = steps[s].quant_window, self.origin[s]
                wins.append(b["feat"][s * G:(s + 1) * G, :, lo - o:hi - o])
            feat, widths = pad_windows(wins)                                  # (n, G, C, Wmax)
            feat = feat.view(len(members) * G, self.C, -1).to(codec.encode_dtype).contiguous()
            ids = codec.quantizer.encode(feat) if widths is None else codec.quantizer.encode(feat, lengths=widths)
            for i, s in enumerate(members):
                st = steps[s]
                j = st.quant_window[0] // self.geo.factor
                out[s] = ids[i, :, st.tokens[0] - j:st.tokens[1] - j].contiguous()
        return out

    def close(self, slot: int) -> torch.Tensor:
        """no more audio for this slot: its remaining tokens, and the slot is free"""
        self._check_open(slot)
        shape = (0,) if self.ch[slot] == 1 else (0, self.ch[slot])
        return self.push({slot: torch.empty(shape, dtype=pcm.FORMATS[self.fmt[slot]][1], device=self._device())}, final=(slot,))[slot]


def pad_windows(wins: List[torch.Tensor]) -> Tuple[torch.Tensor, Optional[List[int]]]:
    """(C, W_i) windows -> ((n, C, Wmax) batch, None) when every W_i is Wmax, else (the batch with every window right-padded by zeros,
    [W_0, ..., W_{n-1}]).  The padding is never read: the lengths travel with the batch.  Windows with more leading dimensions -- the
    (G, C, W_i) feature windows of the encode pool -- are padded along the last one in the same way: (n, G, C, Wmax)."""
    widths = [int(w.shape[-1]) for w in wins]
    wmax = max(widths)
    if all(w == wmax for w in widths):
        return torch.stack(wins).contiguous(), None
    batch = wins[0].new_zeros((len(wins),) + tuple(wins[0].shape[:-1]) + (wmax,))
    for i, w in enumerate(wins):
        batch[i, ..., :widths[i]] = w
    return batch, widths


class DecodeSessions(ParkingPool):
    """`slots` independent incremental decodes, each with the audio and mel of decode() on its own finished token sequence.

        slot = pool.open()                                              # a free slot, fresh state; open(output_sample_rate=48000);
                                                                        # open(lookahead_frames=8) in a pool built with early_emit=True;
                                                                        # open(lookahead_frames=0, crossfade_samples=256) in one built
                                                                        # with crossfade_samples=256 as well; set_lookahead(slot, 8)
        out = pool.push({slot: ids (G, n) int, ...}, noise=None | {slot: (C, n * factor)}, final=())
                                                                        # -> {slot: (audio (1, m * up) | None, mel (n_mels, m))}
        out = pool.close(slot)                                          # = push({slot: empty}, final=(slot,))[slot]

    StreamingDecoder(batch=B) is B replies in lockstep: one token count, one origin, one (prev, next) row, one `finished`.  An LM server's
    replies start at different times, grow by different token counts and end on their own.  Here any subset of the open slots is named
    in a step, each with its own token count (0 is allowed, more than `max_push_tokens` is refused); slots that are not named are idle.
    A slot in `final` ends with these tokens: the step flushes everything that waited for right context, computed with the true end of
    its sequence, and frees the slot.  m >= 0 frames become final per step, after the lookahead StreamingDecoder has (quantiser 4 tokens,
    decoder WaveNet sum(dilations) frames, vocoder receptive_field_frames()).  noise: the decoder's input noise for the pushed frames
    (reproducible runs); a slot without an entry draws its own, as decode() does.

    Per step: ONE quantiser decode over all slots with new condition frames, whatever the lengths of their token windows (right-padded
    into one batch and passed with their lengths: get_quantized_features_from_indices(..., item_features=True); a step whose token
    windows all have one length makes the plain call), ONE decoder
    WaveNet step over all slots (dmel_wavenet_stream_step_items_layered: every launch of the layered step covers all slots, each with
    its own column window), and ONE vocoder call over all slots, whatever the lengths of their mel windows: the windows are right-padded
    into one (n, n_mels, Wmax) batch and passed with their lengths (BigVGAN.forward(x, lengths): every layer sees each item's own end),
    then cropped per slot as StreamingDecoder crops.  A step whose windows all have one length -- the steady state of equal pushes --
    makes the plain call, vocoder(x), as it always did.

    State: buffers of (L + 1, slots, C, cap) and so on, laid out like StreamingDecoder's, `cap` fixed at construction from
    max_push_tokens (stream_schedule.decode_capacity); each slot has its own origin (the absolute frame in column 0 of ITS rows), its own
    token tail and noise tail; re-basing shifts one slot's columns only; a reopened slot's rows are zeroed before its first push.  Memory
    grows neither with the length of a stream nor with the number of sessions served over time.

    Playback rates belong to SESSIONS, not to the pool: `output_sample_rates` declares the rates replies may leave at,
    open(output_sample_rate=r) starts one.  After the vocoder call every such slot's new audio piece is copied behind that slot's
    resampler tail (the copy the codec-rate path spends on detaching the piece from the vocoder's batch), ONE resample launch converts
    all slots (utils/resample.py: SessionResampler), and a final slot is flushed with its true length.  The slot's audio pieces then
    concatenate to resample(decode() audio, vocoder rate, r), bit for bit, m * up samples no longer; its mel is the unchanged decode()
    mel.  return_audios=False with a declared rate is a ValueError.

    The sample format belongs to a session as well and sizes nothing: open(sample_format="s16") starts a reply whose audio comes back as
    torch.int16 (16-bit signed PCM) of the same shape, the rounding of utils/pcm.py (x 32768, clamp, nearest with ties to even) applied to
    the float audio the same session would have returned; its mel is unchanged.  After the vocoder call and the one resample launch,
    ONE dmel_pcm_convert_items launch takes every s16 slot's new piece -- the crop inside the vocoder's batch, or the slot's resampler
    output -- and writes it into one packed int16 buffer of the step; the tensors returned are views of that buffer (this takes the
    place of the clone that detaches a float piece).  f32 slots of such a step keep their path and their bits.  "s16" with
    return_audios=False is a ValueError at open.  open(sample_format="ulaw" | "alaw") starts a G.711 reply the same way: its audio
    comes back as torch.uint8 codes, the companding rule of utils/pcm.py applied to the s16 rounding of that float audio.  The packed
    buffer of the step holds bytes, each piece at a multiple of 16 of them; s16 pieces are int16 views of it, law pieces uint8 views.
    Out of scope: the lockstep StreamingDecoder and whole-clip decode() (callers have utils.pcm.to_pcm16 / to_g711), other formats
    (s24, s32, u8), dither.

    The channel count belongs to a session too and sizes nothing: open(channels=c), 1 < c <= 8, starts a reply for a playback device
    opened with c channels.  Its audio comes back as interleaved frames (m * up, c) -- or (its resampled length, c) -- in its format's
    dtype, the empty piece as (0, c): every channel is, bit for bit, the audio of the same session opened with channels=1 (the sample
    is converted once and stored c times: the fan-out of the channel rule of utils/pcm.py).  Every slot whose format is not f32 OR
    whose channel count exceeds 1 joins the ONE convert launch into the packed buffer of the step; mono f32 slots keep their path and
    their bits.  channels > 1 with return_audios=False is a ValueError at open.  Not served: channel maps, more than 8 channels,
    planar (channel-first) audio, the lockstep StreamingDecoder and whole-clip decode() (callers have utils.pcm.fan_out).

    The look-ahead belongs to a session too.  An exact session hands a frame out once its whole right context exists -- the quantiser's
    4 tokens, the decoder WaveNet's sum(dilations) frames, the vocoder's halo: about 110 frames, 1.2 s, before a reply's first
    sample.  A pool built with early_emit=True also serves sessions opened with open(lookahead_frames=k), k >= 0 mel frames: after a
    push that brings the session to n tokens, T = n * factor frames, it has handed out the frames [0, max(what it had, what the exact
    schedule has, T - k)), and the piece of the push is cut, bit for bit, from the PREFIX decode
    decode(ids[:, :n][None], [n], return_audios, noise=the session's noise for those frames) -- the stream as if it ended here.  A
    final push hands out the rest, cut from decode() of the whole sequence.  So: the pieces tile [0, T_total) without gap or overlap
    and the total length is decode()'s; a frame that had its full context when it left carries decode()'s bits, one that left earlier
    carries the bits of the decode of a shorter clip (audio may be provisional -- token ids never are, which is why EncodeSessions has
    no such option); k = 0 hands out every received frame at once; with k >= geo.hold_frames (k = 10 ** 6) the session IS the exact
    one, piece for piece, and costs nothing more.  Rate, format and channels consume the float piece as before: the resampler sees
    the concatenation of the pieces.  return_audios=False works too (mel only).  stream_schedule.EarlyDecodeSchedule has the rule.
    How: such a pool's state buffers have 2 * slots item rows, row slots + s the SHADOW of slot s.  The committed row of every slot
    advances exactly as an exact session's.  In a step in which T - k lies ahead of it, the quantiser call of the step -- still ONE,
    the slot's token window ends at its newest token anyway -- also yields the frames that wait for right context; ONE
    dmel_stream_fork_items launch copies the committed columns the shadows read (every level's history, the partial skip sums,
    condition, mel) into the shadow rows; the ONE layered WaveNet step runs over all 2 * slots rows, the shadows as final-style rows
    from the committed frontiers to T on every level (the fork comes first and the shadow recomputes the few columns the committed
    row also computes: that keeps the one call); and the ONE vocoder call takes the shadow's window [emitted - halo, T) with its own
    end.  A step that serves only exact sessions launches what it always did; a pool built without early_emit allocates what it
    always did, and refuses lookahead_frames at open.  The final step of an early session is the committed row's: no shadow.

    The look-ahead may move while the session lives: set_lookahead(slot, k) applies from the slot's next push.  The emit rule is the
    one above with the k of the moment; what has left never comes back, so raising k only pauses the session until T - k passes what
    it had, and every piece is still the crop of the prefix decode.  From a push with k >= geo.hold_frames on nothing is forked.
    Start at k = 0 for a fast first sample and raise k once the playback buffer has slack, as a jitter buffer does.

    Pieces cut from different prefix decodes step where they meet.  A pool built with crossfade_samples=Fmax (with early_emit=True
    and audio; 1 <= Fmax <= samples per mel frame) also serves sessions opened with open(lookahead_frames=k, crossfade_samples=F),
    1 <= F <= Fmax, whose pieces join without a step -- the rule of utils/crossfade.py, which is also the host reference the pool is
    tested against bit for bit.  With [A, B) the raw sample range of a push (what it hands out without a fade): a non-final push
    with new frames hands out only up to B - F and keeps the tail P[B - F, B) as F floats of slot state; the next push with new
    frames begins with old + w * (new - old) over the tail and the new prefix decode's version of the same samples, w the raised
    cosine 0.5 - 0.5 cos(pi (i + 0.5) / F) in fp32, three separately rounded fp32 operations; a push without new frames keeps the
    tail; a final push without new frames hands it out as it is.  The pieces still tile [0, total); the audio runs F samples (at
    most one frame, 10.7 ms at 24 kHz) behind the mel, whose pieces are unchanged.  Where both decodes agree the blend returns the old
    sample, so with k >= geo.hold_frames the session returns decode()'s audio exactly, F samples late.  How: the vocoder window of
    such a slot starts one frame earlier ([emitted - halo - 1, ...): the frame in front of the frontier is rendered again with the
    prefix decode's bits; EarlyDecodeSchedule(fade_frames=1) widens the fork window and need_from with it, and `cap` is sized from
    hold_frames + 1).  After the ONE vocoder call, ONE dmel_crossfade_items launch blends in place in the vocoder's batch and saves
    the new tails, for all fading slots of the step; each slot's piece is then the view shifted by F and goes, unchanged, to the
    clone, the resampler or the convert launch -- rate, format and channels see the cross-faded float piece.  A step without a
    fading slot launches what it did; sessions without a fade in such a pool return the pieces they always returned; a pool built
    with crossfade_samples=0 allocates, sizes `cap` and launches exactly as before and refuses crossfade_samples at open.  A fade
    without lookahead_frames or with return_audios=False is a ValueError.  Not served: fades longer than a frame, other windows.

    A session is not tied to its slot: snapshot(slots) gathers everything the named sessions own -- the live window of every level's
    history, of the skip sums, the condition and the mel (stream_schedule.decode_live_window: what a re-base in front of the next push
    would keep), the valid part of the token tail and of the noise tail, the fade tail when one is held, the resampler tail, the
    counters -- with ONE dmel_stream_pack_items launch into one blob; drop(slot) frees a slot without flushing it (a reply's abort);
    park(slots) is both; restore(snapshots) continues the sessions in free slots of this or another pool of the same codec (other
    slots, max_push_tokens and capacity are fine) with ONE launch, each window at column 0 of its zeroed rows.  Every later piece of
    a parked and restored session carries the bits of the uninterrupted one; a snapshot restored while its session lives on is a
    BRANCH: both go on from the same state (an LM server's two continuations, or the roll-back of rejected tokens).  Not shipped:
    shadow rows, fade weights, table scratch, and torch's RNG -- a session pushed without noise draws at the time of the push, in
    the process it runs in.  Refused with ValueError, no slot taken: the other kind, another geometry, width or depth, a rate the
    pool did not declare, an early session into a pool without early_emit, a fade above the pool's, audio into a
    return_audios=False pool, a window or tail that does not fit, an unknown format version.  Equal weights are the caller's
    contract (models/stream_park.py).

    A reply on a phone line also presses keys and plays tones: a pool built with tones=True (and audio) serves
    send_dtmf(slot, "42#") and send_tones(slot, program), which queue a program of tone segments (utils/tones.py: the rule, the
    tables and the host reference the pool is tested against bit for bit) at a mel frame of the session -- at_frame=None: behind
    everything received so far -- and make no device call but the upload of a ramp table of a new length.  With P = at_frame * up
    and [h0, h1) the codec-rate speech samples the slot hands out in a step (`handed` counts them: emitted * up, less the fade tail
    that waits), every request with P <= h1 leaves in that step, and every request in the slot's last one; a push of no tokens
    serves what is due.  ONE dmel_tone_items launch composes speech[h0:P1] | tone 1 | speech[P1:P2] | ... for all such slots,
    straight where each slot's route reads it: behind its resampler tail (destinations() / push(placed=True); the launch then
    places the step's other resampled pieces too, since a push is placed as a whole), in its row of a staging buffer the convert
    launch reads, or in a fresh tensor that is handed out in place of the clone.  So a session's audio is, bit for bit, its wire
    chain (resample, format, channels) applied to tones.splice(its codec-rate stream, [(P, program), ...]), however the tokens were
    cut into pushes.  Mel pieces and frames_emitted do not change; a step that serves no request launches, allocates and returns
    what it did; a pool built without tones=True is what it was and refuses send_*.  Refused with ValueError, nothing queued: a
    frequency at or above half the session's output rate, an anchor outside [frames_emitted, frames received] or before an earlier
    request's, more than max_tone_samples (default: two seconds at the vocoder's rate) pending samples or 64 pending segments in the
    slot.  tones_pending(slot) -> [(at_frame, samples)].  The queue travels with snapshot / restore as plain values (meta keys
    tones, handed, tone_samples; a pool without tones=True refuses a snapshot with pending requests, a tone pool one above its
    max_tone_samples; snapshots without the keys restore with none); drop discards it.  The resampler's rows are sized for
    cap * up + max_tone_samples.  Not served: RFC 4733 telephone-events, tones mixed over speech, non-integer frequencies, tones in
    the mel; no ITU-T Q.23 / Q.24 conformance is claimed.

    How loud a reply is and how it ends: a pool built with shape=True (and audio) serves sessions opened with shape=True or a
    ShapeConfig (utils/shape.py: the rule, its defaults and its caveats).  set_gain(slot, gain_db, ramp_ms, at_sample) moves the
    session's commanded gain along a raised cosine from a sample of z -- its float stream at the vocoder's rate behind the tone
    splice -- on (ducking, output level, float("-inf") for mute); a block look-ahead limiter keeps |y| <= ceiling, for which the
    audio runs N .. 2 N - 1 samples behind the mel; stop(slot, fade_ms) ends a reply on barge-in: close() behind a fade to 0 and the
    end E of it, the hold and the resampler flushed at the true length (a stop of an exact session still computes its whole
    flush).  ONE dmel_shape_items launch per step, between the tone launch and the resampler, serves all shaping slots with a new
    piece or their end.  A shaping session's audio is, bit for bit, its wire chain (resample, format, channels) applied to
    shape.scan(tones.splice(its codec-rate stream, inserts), requests, config, end), however the tokens were cut into pushes; mel
    pieces and frames_emitted do not change; a session opened without shape= and a pool built without shape=True are what they
    were, and such a pool refuses open(shape=), set_gain, stop, shaped and the snapshot of a shaping session.  shaped() ->
    {slot: ShapeReport} (one copy of the headers); shape_blocks(slot): per-block (peak, gain) of the last push; samples_fed(slot):
    "now" of set_gain.  The state travels with snapshot / restore (meta keys shape, shape_segments, shape_base, shape_fed, shape_hold,
    shape_end; a snapshot without them restores as a session without the option); drop discards it.  The resampler's rows of such
    a pool hold 2 * 1024 - 1 samples more: what a limiter hands out late.

    How fast a reply speaks: a pool built with pace=True (and audio) serves sessions opened with pace=True or a PaceConfig
    (utils/pace.py: the rule -- WSOLA time-scaling, the pitch stays --, its defaults and its caveats).  set_pace(slot, permille,
    at_sample) sets the rate (500 .. 2000 permille of the unchanged speed) from an input sample of the slot's pacer on; pace_fed(slot)
    is "now".  The pacer acts on the slot's speech pieces as _route receives them -- behind the vocoder and the cross-fade, the
    flushed fade tail included --, in front of the shaper, the resampler and the wire convert: ONE dmel_pace_items launch per step
    serves all pacing slots with a new piece or their end and writes where the slot's route reads -- the shaper's source row when
    the session also shapes, else a staging row for the resampler or the convert launch, else a fresh tensor handed out in place of
    the clone.  A pacing session's audio is, bit for bit, its wire chain applied to pace.scan(its codec-rate stream, requests,
    config, final=True)[0] -- to shape.scan of that where it also shapes --, however the tokens were cut into pushes; rate 1000 is
    the plain audio.  For such a session set_gain(at_sample=), samples_fed and stop count in the PACED stream.  Mel pieces and
    frames_emitted do not change; a session opened without pace= and a pool built without pace=True are what they were, and such a
    pool refuses open(pace=), set_pace, pace_fed, paced, pace_frames and the snapshot of a pacing session.  paced() ->
    {slot: PaceReport} (one copy of the headers); pace_frames(slot): per-frame (offset, score) of the last push.  The state travels
    with snapshot / restore (meta keys pace, pace_ints, pace_requests, pace_base; a snapshot without them restores as a session
    without the option); drop discards it.  The rows downstream of the pacer -- the shaper's staging, the resampler's rows, the
    convert staging -- are sized from pace.max_out(cap * up + fade, 512, 512) in such a pool.  Not served: tones on a pacing
    session (send_dtmf / send_tones are refused: tones must not be stretched, and mapping an anchor frame through a rate that may
    still change is a separate piece of work), pacing the lockstep StreamingDecoder and whole-clip decode() (callers have
    pace.scan), a playout buffer that chooses the rate.

    Out of scope, NotImplementedError: overlap_vocoder, graph_chunk_tokens, and a pool-wide output_sample_rate (a pool has no rate of
    its own).

    All launches are on the current stream; there is no side stream for the vocoder.  The warning of StreamingEncoder / EncodeSessions
    about the STFT next to convolutions on ANOTHER STREAM applies to this pool's convolutions: a caller that runs
    encode sessions on a second stream beside this pool must call dmel_stft_set_exclusive_cu(1) first, exactly as pipeline.CodecLanes
    does."""

    def __init__(self, codec, slots: int, max_push_tokens: int = 64, return_audios: bool = True, overlap_vocoder: bool = False,
                 graph_chunk_tokens: Optional[int] = None, output_sample_rate: Optional[int] = None,
                 output_sample_rates: Iterable[int] = (), early_emit: bool = False, crossfade_samples: int = 0, tones: bool = False,
                 max_tone_samples: Optional[int] = None, shape: bool = False, pace: bool = False):
        if overlap_vocoder or graph_chunk_tokens is not None or output_sample_rate is not None:
            raise NotImplementedError("decode sessions launch everything on the current stream, eagerly, and have no rate of their own: "
                                      "overlap_vocoder, graph_chunk_tokens and output_sample_rate belong to StreamingDecoder (a session's "
                                      "playback rate: output_sample_rates= and open(output_sample_rate=))")
        output_sample_rates = tuple(int(r) for r in output_sample_rates)
        if output_sample_rates and not return_audios:
            raise ValueError("output_sample_rates without audio: return_audios=False leaves nothing to resample")
        if any(r <= 0 for r in output_sample_rates):
            raise ValueError("sample rates must be positive")
        if codec.decoder is None:
            raise ValueError("Decoder is not loaded")
        if return_audios and codec.vocoder is None:
            raise ValueError("Vocoder is not loaded")
        if int(slots) <= 0 or int(max_push_tokens) <= 0:
            raise ValueError("slots and max_push_tokens must be positive")
        dec = codec.decoder
        if dec.input_projection is not None:
            raise NotImplementedError("streaming needs a decoder without input projection (input_channels == residual_channels)")
        self.codec, self.S, self.G = codec, int(slots), codec.dmel_groups
        self.return_audios = self._has_audio = bool(return_audios)
        self.early_emit = bool(early_emit)
        self.N = 2 * self.S if self.early_emit else self.S    # item rows of the state buffers: rows S .. 2 S - 1 are the shadows
        self.L, self.C = len(dec.residual_layers), dec.residual_channels
        cycle = dec.dilation_cycle or 0
        dils = tuple(2 ** (i % cycle) if cycle else 1 for i in range(self.L))
        self.geo = DecodeGeometry(factor=math.prod(codec.quantizer.downsample_factor), dilations=dils,
                                  voc_halo=codec.vocoder.receptive_field_frames() if return_audios else 0)
        self.up = math.prod(codec.vocoder.h.upsample_rates) if return_audios else 1
        self.max_push = int(max_push_tokens)
        # the longest cross-fade a session of this pool may open with (0: none, and the pool is what it was without the option)
        self.fade_max = 0
        if crossfade_samples != 0:
            if not self.early_emit or not return_audios:
                raise ValueError("crossfade_samples joins the audio pieces of sessions that emit early: it needs early_emit=True and "
                                 "return_audios=True")
            self.fade_max = crossfade.check_fade(crossfade_samples, self.up)
        self.cap = decode_capacity(self.geo, self.max_push, extra_hold=1 if self.fade_max else 0)
        H, f = self.geo.quant_halo_tokens, self.geo.factor
        self.tok_width = 2 * H + self.max_push            # the token tail starts at most 2 H tokens behind the newest token of the last push
        self.noise_width = (H + self.max_push) * f        # frames [z_valid, tokens * factor): at most H tokens of them in front of a push
        self.voc_rate = int(codec.vocoder.h.get("sampling_rate", codec.encode_mel_transform.sample_rate)) if return_audios else None
        self.output_sample_rates = tuple(sorted(set(output_sample_rates) - {self.voc_rate}))      # none without audio (refused above)
        # the pool sends tones (send_dtmf / send_tones): at most max_tone samples of them wait in a slot, and leave in one step
        if not isinstance(tones, bool):
            raise ValueError(f"tones must be a bool, got {tones!r}")
        self.tones_on, self.max_tone = tones, 0
        if tones:
            if not return_audios:
                raise ValueError("tones without audio: return_audios=False leaves nothing to splice them into")
            tone_rule.check_rate(self.voc_rate)
            self.max_tone = 2 * self.voc_rate if max_tone_samples is None else max_tone_samples
            if isinstance(self.max_tone, bool) or not isinstance(self.max_tone, int) or self.max_tone < 1:
                raise ValueError(f"max_tone_samples must be a positive integer (samples at the vocoder's rate), got {max_tone_samples!r}")
        elif max_tone_samples is not None:
            raise ValueError("max_tone_samples on a pool built without tones=True")
        # the pool shapes replies (open(shape=), set_gain, stop): a limiter holds back at most 2 N - 1 samples, which leave with a later step
        if not isinstance(shape, bool):
            raise ValueError(f"shape must be a bool, got {shape!r}")
        if shape and not return_audios:
            raise ValueError("shape without audio: return_audios=False leaves nothing to shape")
        self.shape_on = shape
        self.shape_room = 2 * shape_rule.MAX_BLOCK - 1 if shape else 0
        # the pool paces replies (open(pace=), set_pace): a step's piece leaves the pacer longer or shorter than it came
        if not isinstance(pace, bool):
            raise ValueError(f"pace must be a bool, got {pace!r}")
        if pace and not return_audios:
            raise ValueError("pace without audio: return_audios=False leaves nothing to pace")
        self.pace_on = pace
        # a step emits frames that all lie in the slot's `cap` columns: at most cap * up samples and the tones that waited -- in a
        # pace pool at most what the pacer makes of a step's piece (or of a fade tail) -- and what a limiter held back, reach a
        # slot's resampler at once
        self.chain_w = self.cap * self.up + self.max_tone
        if pace:
            self.chain_w = max(self.chain_w, pace_rule.max_out(self.cap * self.up + self.fade_max, pace_rule.MAX_HOP, pace_rule.MAX_SEARCH))
        self._init_slots(self.voc_rate, "output_sample_rates", self.chain_w + self.shape_room)
        self.pcfg: List[Optional[pace_rule.PaceConfig]] = [None] * self.S
        self.preq: List[list] = [[] for _ in range(self.S)]   # the slot's live rate requests (P, permille), over the rate pbase
        self.pbase = [1000] * self.S
        self.pints: List[tuple] = [pace_rule.FRESH] * self.S  # (K, a_{K-1}, a_K, fed): the pacer's integers, tracked from the rule's
        self._pace_n = [0] * self.S                       # frames the slot's last push completed
        self._pace_src: Dict[int, torch.Tensor] = {}      # the float pieces of the step the pacer reads
        self._pw_off: Dict[int, int] = {}                 # hop -> offset of its weight table in the pool's pace arena
        self._pw_floats = 0
        self.scfg: List[Optional[shape_rule.ShapeConfig]] = [None] * self.S
        self.sreq: List[list] = [[] for _ in range(self.S)]   # the slot's live gain segments (P, g0, g1, ramp), over the base gain sbase
        self.sbase = [1.0] * self.S
        self.sfed = [0] * self.S                          # samples of z the slot's shaper has taken
        self.shold = [0] * self.S                         # samples its limiter holds (the row's `hold`, tracked from the rule's integers)
        self.send: List[Optional[int]] = [None] * self.S  # the end sample E of a stopped session
        self._shape_n = [0] * self.S                      # blocks the slot's last push completed
        self._shape_src: Dict[int, torch.Tensor] = {}     # the float pieces of the step the shaper reads
        self._sramp_off: Dict[int, int] = {}              # gain ramp length -> offset of its table in the pool's shape arena
        self._sramp_floats = 0
        self.tq: List[list] = [[] for _ in range(self.S)]     # the slot's pending requests, (P, program) in the order they leave
        self.handed = [0] * self.S                        # speech samples at the vocoder's rate the slot has handed out
        self.tone_samples = [0] * self.S                  # samples its pending requests render to
        self._ramp_off: Dict[int, int] = {}               # ramp length -> offset of its table in the pool's ramp arena
        self._ramp_floats = 0
        self._held: Dict[int, torch.Tensor] = {}          # the float pieces of the step that tones are spliced into
        self._ending: set = set()
        self.fade = [0] * self.S                          # the slot's cross-fade in samples (0: none)
        self.has_tail = [False] * self.S                  # the slot holds back the last `fade` samples of its newest piece
        self.tok_origin = [0] * self.S                    # absolute index of the token in column 0 of the slot's token tail
        self.n_noise = [0] * self.S                       # valid frames in the slot's noise tail

    def frames_emitted(self, slot: int) -> int:
        self._check_open(slot)
        return self.sched[slot].emitted

    def open(self, output_sample_rate: Optional[int] = None, sample_format: str = "f32", channels: int = 1,
             lookahead_frames: Optional[int] = None, crossfade_samples: int = 0, shape=None, pace=None) -> int:
        """take a free slot: fresh schedule, state zeroed before its first push.  output_sample_rate: the rate this session's audio
        leaves at, one of the declared `output_sample_rates` (None: the vocoder's).  sample_format: "f32", "s16" for audio returned
        as torch.int16 (16-bit signed PCM), or "ulaw" / "alaw" for torch.uint8 (G.711 codes).  channels: 1 .. 8; above 1 the audio
        comes back as interleaved frames (n, channels), every channel the mono audio.  lookahead_frames: None for the exact session;
        k >= 0 (mel frames) for a session that emits every frame at most k behind the newest one received, on a pool built with
        early_emit=True.  crossfade_samples: F >= 1 samples (at most the pool's crossfade_samples and one mel frame) over which
        such a session blends every piece into the next (utils/crossfade.py); its audio runs F samples behind its mel.  shape: True
        or a ShapeConfig (utils/shape.py) for a session whose audio passes the commanded gain and the limiter, on a pool built with
        shape=True: set_gain and stop serve it, and its audio runs N .. 2 N - 1 samples behind with the limiter.  pace: True or a
        PaceConfig (utils/pace.py) for a session whose speech passes the pacer, on a pool built with pace=True: set_pace serves it.
        Raises when every slot is taken; a refused open takes no slot."""
        pcfg = pace_rule.as_config(pace)
        if pcfg is not None:
            if not self.pace_on:
                raise ValueError("pace on a pool built without pace=True: it has no rows to hold a reply's samples in")
            pcfg.samples(self.voc_rate)
        scfg = shape_rule.as_config(shape)
        if scfg is not None:
            if not self.shape_on:
                raise ValueError("shape on a pool built without shape=True: it has no rows to hold a reply back in")
            scfg.block(self.voc_rate)
        if isinstance(crossfade_samples, bool) or not isinstance(crossfade_samples, int) or crossfade_samples < 0:
            raise ValueError(f"crossfade_samples must be an integer >= 0 (samples), got {crossfade_samples!r}")
        if crossfade_samples:
            if not self.fade_max:
                raise ValueError("crossfade_samples on a pool built without crossfade_samples=: it has no tails to blend with")
            if lookahead_frames is None:
                raise ValueError("crossfade_samples without lookahead_frames: the pieces of an exact session join as they are")
            if not self.return_audios:
                raise ValueError("crossfade_samples without audio: return_audios=False leaves nothing to blend")
            if crossfade_samples > self.fade_max:
                raise ValueError(f"crossfade_samples={crossfade_samples} exceeds the pool's crossfade_samples={self.fade_max} (and a "
                                 f"fade is at most one mel frame, {self.up} samples)")
        if lookahead_frames is not None:
            if not self.early_emit:
                raise ValueError("lookahead_frames on a pool built without early_emit=True: it has no shadow rows to decode ahead in")
            if isinstance(lookahead_frames, bool) or not isinstance(lookahead_frames, int) or lookahead_frames < 0:
                raise ValueError(f"lookahead_frames must be an integer >= 0 (mel frames) or None, got {lookahead_frames!r}")
        rate = self.voc_rate if output_sample_rate is None else int(output_sample_rate)
        self._check_wire(rate, sample_format, channels)
        s = self._first_free()
        sched = (DecodeSchedule(self.geo) if lookahead_frames is None
                 else EarlyDecodeSchedule(self.geo, lookahead_frames, fade_frames=1 if crossfade_samples else 0))
        self._occupy(s, sched, 0, rate, sample_format, channels)
        self.tok_origin[s] = self.n_noise[s] = 0
        self.fade[s], self.has_tail[s] = crossfade_samples, False
        self.tq[s], self.handed[s], self.tone_samples[s] = [], 0, 0
        self._shape_adopt(s, scfg)
        self._pace_adopt(s, pcfg)
        return s

    # -- pacing: the speaking rate of a reply (utils/pace.py) ----------------------------------------------------------------------
    def _pace_adopt(self, s: int, cfg, requests=(), base=None, ints=pace_rule.FRESH) -> None:
        self.pcfg[s], self.preq[s], self.pbase[s] = cfg, [tuple(r) for r in requests], cfg.initial_permille if cfg and base is None else base or 0
        self.pints[s], self._pace_n[s] = tuple(ints), 0
        if cfg is not None:
            H = cfg.samples(self.voc_rate)[0]
            if H not in self._pw_off:
                self._pw_off[H], self._pw_floats = self._pw_floats, self._pw_floats + H
                if self.buf is not None:
                    self._upload_pace_weights([H])

    def _upload_pace_weights(self, hops) -> None:
        arena = self.buf["pace_w"]
        if arena.numel() < self._pw_floats:            # grow: the tables keep their offsets
            grown = torch.zeros(2 * self._pw_floats, dtype=torch.float32, device=arena.device)
            grown[:arena.numel()] = arena
            self.buf["pace_w"] = arena = grown
        for h in hops:
            arena[self._pw_off[h]:self._pw_off[h] + h] = torch.tensor(pace_rule.weight_table(h))

    def _pacing(self, slot: int, what: str) -> pace_rule.PaceConfig:
        if not self.pace_on:
            raise ValueError(f"{what} on a pool built without pace=True: it has no rows to hold a reply's samples in")
        self._check_open(slot)
        if self.pcfg[slot] is None:
            raise ValueError(f"{what}: slot {slot} was opened without pace=")
        return self.pcfg[slot]

    def pace_fed(self, slot: int) -> int:
        """input samples -- the slot's speech at the vocoder's rate, cross-faded where the session fades -- its pacer has taken:
        "now" of set_pace"""
        self._pacing(slot, "pace_fed")
        return self.pints[slot][3]

    def set_pace(self, slot: int, permille: int, at_sample: Optional[int] = None) -> int:
        """speak at `permille` of the unchanged speed (500 .. 2000; 1500 is one and a half times as fast) from input sample
        at_sample of the slot's pacer on -> that position.  at_sample=None is "now", pace_fed(slot); an explicit one lies at or
        beyond that and not before an earlier request's.  The rate of an output frame is the one in force where the frame before
        it was cut (utils/pace.py), so a request takes hold within about two hops.  No device call.  ValueError, nothing queued:
        a pool or a session without the option, a rate outside [500, 2000], a position outside those bounds, a ninth live
        request."""
        self._pacing(slot, "set_pace")
        fed = self.pints[slot][3]
        after = max([fed] + [r[0] for r in self.preq[slot]])
        request = pace_rule.check_request((fed if at_sample is None else at_sample, permille), fed, after)
        if len(self.preq[slot]) >= pace_rule.MAX_REQUESTS:
            raise ValueError(f"slot {slot}: {len(self.preq[slot])} rate requests are live, a ninth is refused")
        self.preq[slot] = self.preq[slot] + [request]
        return request[0]

    def paced(self) -> Dict[int, pace_rule.PaceReport]:
        """{slot: PaceReport} of every open pacing session: ONE device-to-host copy of the rows' headers"""
        if not self.pace_on:
            raise ValueError("paced on a pool built without pace=True")
        slots = [s for s in self.open_slots if self.pcfg[s] is not None]
        live = [s for s in slots if not self._fresh[s]] if self.buf is not None else []
        table = self.buf["pace"][:, :pace_rule.HEADER].cpu() if live else None
        zero = torch.zeros(pace_rule.HEADER, dtype=torch.int32)
        return {s: pace_rule.report(table[s] if s in live else zero, self.pcfg[s].initial_permille) for s in slots}

    def pace_frames(self, slot: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(offset, score) of the frames the slot's last push completed: device views (n,), int32 p - a and fp32 q, valid until
        the slot's next push"""
        self._pacing(slot, "pace_frames")
        if self.buf is None or self._fresh[slot]:
            dev = self._device()
            return torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.float32, device=dev)
        n = self._pace_n[slot]
        return self.buf["pace_off"][slot, :n], self.buf["pace_score"][slot, :n]

    # -- shaping: output gain, ducking, a limiter and a clean stop (utils/shape.py) ---------------------------------------------
    def _shape_adopt(self, s: int, cfg, segments=(), base=None, fed: int = 0, hold: int = 0, end=None) -> None:
        self.scfg[s], self.sreq[s], self.sbase[s] = cfg, [tuple(sg) for sg in segments], cfg.initial_gain if cfg and base is None else base or 0.0
        self.sfed[s], self.shold[s], self.send[s], self._shape_n[s] = fed, hold, end, 0

    def _shaping(self, slot: int, what: str) -> shape_rule.ShapeConfig:
        if not self.shape_on:
            raise ValueError(f"{what} on a pool built without shape=True: it has no rows to hold a reply back in")
        self._check_open(slot)
        if self.scfg[slot] is None:
            raise ValueError(f"{what}: slot {slot} was opened without shape=")
        return self.scfg[slot]

    def samples_fed(self, slot: int) -> int:
        """samples of z -- the slot's stream at the vocoder's rate behind the tone splice -- its shaper has taken: "now" of set_gain"""
        self._shaping(slot, "samples_fed")
        return self.sfed[slot]

    def _shape_request(self, slot: int, cfg, request, keep_future: bool = True) -> None:
        now = self.sfed[slot]
        segs, base = shape_rule.live(self.sreq[slot], self.sbase[slot], now)
        if not keep_future:
            segs = [sg for sg in segs if sg[0] <= now]
        if len(segs) >= shape_rule.MAX_SEGMENTS:
            raise ValueError(f"slot {slot}: {len(segs)} gain requests are live, a ninth is refused")
        ramp = request[2]
        if ramp and ramp not in self._sramp_off:
            self._sramp_off[ramp], self._sramp_floats = self._sramp_floats, self._sramp_floats + ramp
            if self.buf is not None:
                self._upload_shape_ramps([ramp])
        self.sreq[slot], self.sbase[slot] = segs + [shape_rule.extend(segs, base, request)], base

    def _upload_shape_ramps(self, lengths) -> None:
        arena = self.buf["shape_ramps"]
        if arena.numel() < self._sramp_floats:         # grow: the tables keep their offsets
            grown = torch.zeros(2 * self._sramp_floats, dtype=torch.float32, device=arena.device)
            grown[:arena.numel()] = arena
            self.buf["shape_ramps"] = arena = grown
        for n in lengths:
            arena[self._sramp_off[n]:self._sramp_off[n] + n] = torch.tensor(shape_rule.ramp_table(n))

    def set_gain(self, slot: int, gain_db: float, ramp_ms: float = 20.0, at_sample: Optional[int] = None) -> int:
        """move the slot's commanded gain to gain_db (float("-inf"): mute) over ramp_ms, from sample at_sample of z on -> that anchor.
        at_sample=None is "now", samples_fed(slot); an explicit anchor lies at or beyond that and not before an earlier request's.
        The request may interrupt a ramp that is under way (utils/shape.py).  No device call, apart from the upload of a ramp table
        of a length the pool has not seen.  ValueError, nothing queued: a pool or a session without the option, a gain above the
        config's max_gain, a ramp above 16384 samples, an anchor outside those bounds, a ninth live request."""
        cfg = self._shaping(slot, "set_gain")
        if isinstance(gain_db, bool) or not isinstance(gain_db, (int, float)) or gain_db != gain_db or gain_db == math.inf:
            raise ValueError(f"gain_db must be a level in dB or float('-inf'), got {gain_db!r}")
        gain = 0.0 if gain_db == -math.inf else 10.0 ** (gain_db / 20.0)
        now = self.sfed[slot]
        after = max([now] + [sg[0] for sg in self.sreq[slot]])
        anchor = now if at_sample is None else at_sample
        request = shape_rule.check_request((anchor, gain, tone_rule._samples(ramp_ms, self.voc_rate, "ramp_ms")), cfg, after)
        self._shape_request(slot, cfg, request)
        return request[0]

    def stop(self, slot: int, fade_ms: float = 20.0):
        """end a reply on barge-in: close(slot) behind a request (now, 0, ramp) and the end E = now + ramp -> (audio, mel) as close
        returns them.  The audio is the session's remaining output up to E, faded, the limiter's hold and the resampler flushed at
        the true length; the mel is the unchanged flush.  The slot is free afterwards; requests anchored behind now and tones behind
        E are discarded.  A stop of an exact session still computes its whole flush: the cost is not optimised here."""
        cfg = self._shaping(slot, "stop")
        now = self.sfed[slot]
        request = shape_rule.check_request((now, 0.0, tone_rule._samples(fade_ms, self.voc_rate, "fade_ms")), cfg, now)
        self._shape_request(slot, cfg, request, keep_future=False)
        self.send[slot] = now + request[2]
        return self.close(slot)

    def _shape_slots(self) -> List[int]:
        return [s for s in self.open_slots if self.scfg[s] is not None]

    def shaped(self) -> Dict[int, shape_rule.ShapeReport]:
        """{slot: ShapeReport} of every open shaping session: ONE device-to-host copy of the rows' headers"""
        if not self.shape_on:
            raise ValueError("shaped on a pool built without shape=True")
        slots = self._shape_slots()
        live = [s for s in slots if not self._fresh[s]] if self.buf is not None else []
        table = self.buf["shape"][:, :shape_rule.HEADER].cpu() if live else None
        zero = torch.zeros(shape_rule.HEADER, dtype=torch.int32)
        return {s: shape_rule.report(table[s] if s in live else zero, self.scfg[s].block(self.voc_rate), self.voc_rate,
                                     self.scfg[s].initial_gain) for s in slots}

    def shape_blocks(self, slot: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(peak, gain) of the blocks the slot's last push completed: device fp32 views (n,), valid until the slot's next push.
        peak: max |v| of the block; gain: the limiter's s behind it"""
        self._shaping(slot, "shape_blocks")
        if self.buf is None or self._fresh[slot]:
            empty = torch.empty(0, dtype=torch.float32, device=self._device())
            return empty, empty.clone()
        n = self._shape_n[slot]
        return self.buf["shape_peak"][slot, :n], self.buf["shape_gain"][slot, :n]

    # -- tones: DTMF keys, beeps and call-progress tones spliced into a session's audio (utils/tones.py) -----------------------
    def send_dtmf(self, slot: int, keys: str, *, tone_ms=80, gap_ms=80, level_dbfs=-10.0, twist_db=2.0, ramp_ms=1.0,
                  at_frame: Optional[int] = None) -> int:
        """queue the DTMF keys `keys` (tones.dtmf_program at the vocoder's rate) for the slot: send_tones of that program"""
        if not self.tones_on:
            raise ValueError("send_dtmf on a pool built without tones=True: it has no tone tables")
        return self.send_tones(slot, tone_rule.dtmf_program(keys, self.voc_rate, tone_ms, gap_ms, level_dbfs, twist_db, ramp_ms), at_frame)

    def send_tones(self, slot: int, program, at_frame: Optional[int] = None) -> int:
        """queue a program of tone segments (utils/tones.py) for the slot -> the samples at the vocoder's rate it renders to.  The
        rendering goes in front of speech sample at_frame * up of the session's audio at the vocoder's rate: at_frame=None is
        "behind everything received so far" (tokens * factor now); an explicit one lies in [frames_emitted(slot), frames received]
        and not before an earlier pending request's.  The request leaves with the step in which the session's speech reaches
        that sample (a push of no tokens will do where it already has), or with its last step.  No device call, apart from the
        upload of a ramp table of a length the pool has not seen.  ValueError, nothing queued: a pool without tones=True, a
        program outside the bounds of utils/tones.py, a frequency at or above half the session's output rate, an anchor outside
        those bounds, more than max_tone_samples pending samples or 64 pending segments in the slot."""
        if not self.tones_on:
            raise ValueError("send_tones on a pool built without tones=True: it has no tone tables")
        self._check_open(slot)
        if self.pcfg[slot] is not None:
            raise ValueError(f"slot {slot} paces its reply: tones must not be stretched, and a pacing session sends none")
        program = self._check_tones(tone_rule.check_program(program, self.voc_rate), self.rate[slot])
        sch, f = self.sched[slot], self.geo.factor
        frames, last = sch.tokens * f, self.tq[slot][-1][0] // self.up if self.tq[slot] else 0
        if at_frame is None:
            at_frame = frames
        elif isinstance(at_frame, bool) or not isinstance(at_frame, int) or not max(sch.emitted, last) <= at_frame <= frames:
            raise ValueError(f"slot {slot}: at_frame must be an integer in [{max(sch.emitted, last)}, {frames}] (frames emitted or an "
                             f"earlier request's anchor .. frames received), got {at_frame!r}")
        n = tone_rule.length(program)
        if self.tone_samples[slot] + n > self.max_tone:
            raise ValueError(f"slot {slot}: {self.tone_samples[slot]} pending samples and {n} more exceed max_tone_samples = {self.max_tone}")
        if sum(len(p) for _, p in self.tq[slot]) + len(program) > tone_rule.MAX_SEGMENTS:
            raise ValueError(f"slot {slot}: more than {tone_rule.MAX_SEGMENTS} pending segments")
        self._ramps_for(program)
        self.tq[slot].append((at_frame * self.up, program))
        self.tone_samples[slot] += n
        return n

    def tones_pending(self, slot: int) -> List[Tuple[int, int]]:
        """[(at_frame, samples at the vocoder's rate)] of the slot's requests that have not left yet, in the order they will"""
        self._check_open(slot)
        return [(P // self.up, tone_rule.length(p)) for P, p in self.tq[slot]]

    def _check_tones(self, program, rate):
        """a checked program against the rate the session's audio leaves at: what the resampler would fold is refused"""
        rate = self.voc_rate if rate is None else rate
        for k, seg in enumerate(program):
            if max(seg[0], seg[1]) * 2 >= rate:
                raise ValueError(f"segment {k}: {max(seg[0], seg[1])} Hz is not below half of the session's output rate {rate} Hz")
        return program

    def _ramps_for(self, program) -> None:
        """every ramp length of the program has its table in the pool's arena: appended, and uploaded where the arena exists"""
        for seg in program:
            n = seg[6]
            if n and n not in self._ramp_off:
                self._ramp_off[n], self._ramp_floats = self._ramp_floats, self._ramp_floats + n
                if self.buf is not None:
                    self._upload_ramps([n])

    def _upload_ramps(self, lengths) -> None:
        arena = self.buf["tone_ramps"]
        if arena.numel() < self._ramp_floats:          # grow: the tables keep their offsets
            grown = torch.zeros(2 * self._ramp_floats, dtype=torch.float32, device=arena.device)
            grown[:arena.numel()] = arena
            self.buf["tone_ramps"] = arena = grown
        for n in lengths:
            arena[self._ramp_off[n]:self._ramp_off[n] + n] = torch.tensor(tone_rule.ramp_table(n))

    def drop(self, slot: int) -> None:
        """ParkingPool.drop; the slot's pending tone requests are discarded with it"""
        super().drop(slot)
        self.tq[slot], self.tone_samples[slot] = [], 0      # what the session had not sent is gone with it
        self._shape_adopt(slot, None)
        self._pace_adopt(slot, None)

    def set_lookahead(self, slot: int, lookahead_frames: int) -> None:
        """the look-ahead of an open early session from its next push on.  What has left never comes back: raising it pauses the
        session's emission until the newest frame is that far ahead; from a push with lookahead_frames >= geo.hold_frames on, the
        steps are the exact session's and nothing is forked."""
        self._check_open(slot)
        if not isinstance(self.sched[slot], EarlyDecodeSchedule):
            raise ValueError(f"slot {slot} was opened without lookahead_frames: an exact session has no look-ahead to move")
        if isinstance(lookahead_frames, bool) or not isinstance(lookahead_frames, int) or lookahead_frames < 0:
            raise ValueError(f"lookahead_frames must be an integer >= 0 (mel frames), got {lookahead_frames!r}")
        self.sched[slot].set_lookahead(lookahead_frames)

    def _validate(self, ids: Mapping[int, torch.Tensor], noise, final) -> None:
        """everything that can be refused, before any state changes and before any device call"""
        if not ids:
            raise ValueError("push needs at least one slot")
        f = self.geo.factor
        for slot, t in ids.items():
            self._check_open(slot)
            if t.ndim != 2 or t.shape[0] != self.G:
                raise ValueError(f"slot {slot}: expected ids of shape ({self.G}, n), got {tuple(t.shape)}")
            if t.shape[1] > self.max_push:
                raise ValueError(f"slot {slot}: a push of {t.shape[1]} tokens exceeds max_push_tokens = {self.max_push}")
            _lib.require_cuda(t, "indices")
        for slot in final:
            if slot not in ids:
                raise ValueError(f"slot {slot} is in `final` but not among the pushed slots")
        for slot, z in (noise or {}).items():
            if slot not in ids:
                raise ValueError(f"noise for slot {slot}, which is not among the pushed slots")
            if tuple(z.shape) != (self.C, ids[slot].shape[1] * f):
                raise ValueError(f"slot {slot}: noise must have shape {(self.C, ids[slot].shape[1] * f)}")

    # -- buffers -----------------------------------------------------------------------------------------------------------
    def _allocate(self, dev) -> None:
        S, N, dec = self.S, self.N, self.codec.decoder
        rows = N * (2 * (self.L + 1) + 1)
        self.buf = dict(hist=torch.zeros(self.L + 1, N, self.C, self.cap, dtype=torch.float32, device=dev),
                        skip=torch.zeros(N, self.C, self.cap, dtype=torch.float32, device=dev),
                        cond=torch.zeros(N, dec.condition_channels, self.cap, dtype=torch.float32, device=dev),
                        mel=torch.zeros(N, dec.output_channels, self.cap, dtype=torch.float32, device=dev),
                        tokens=torch.zeros(S, self.G, self.tok_width, dtype=torch.int32, device=dev),
                        noise=torch.zeros(S, self.C, self.noise_width, dtype=torch.float32, device=dev),
                        # dmel_wavenet_stream_step_items_layered: 2 N C cap floats, N int64, and the row table behind them
                        scratch=torch.empty(2 * N * self.C * self.cap + 2 * N + rows, dtype=torch.float32, device=dev),
                        pcm_tab=torch.empty(4 * S, dtype=torch.int64, device=dev))
        if self.early_emit:                           # dmel_stream_fork_items: 5 int32 per fork, at most one fork per slot
            self.buf["fork_tab"] = torch.empty(5 * S, dtype=torch.int32, device=dev)
        if self.fade_max:                             # dmel_crossfade_items: a tail and the weights per slot, 5 int64 per row of the table
            self.buf["fade_tail"] = torch.zeros(S, self.fade_max, dtype=torch.float32, device=dev)
            self.buf["fade_w"] = torch.zeros(S, self.fade_max, dtype=torch.float32, device=dev)
            self.buf["fade_tab"] = torch.empty(5 * S, dtype=torch.int64, device=dev)
        if self.tones_on:                             # dmel_tone_items: the sine table of the vocoder's rate, the ramp arena, a row per
            #                                           slot in which the convert launch finds a spliced piece, and the table: a slot
            #                                           has at most 64 requests (one segment each at least) between 65 cuts of speech
            most = tone_rule.MAX_SEGMENTS
            self.buf.update(tone_sine=torch.tensor(tone_rule.sine_table(self.voc_rate)).to(dev),
                            tone_ramps=torch.zeros(max(2 * self._ramp_floats, 4 * tone_rule.MAX_RAMP), dtype=torch.float32, device=dev),
                            tone_stage=torch.empty(S, self.cap * self.up + self.max_tone, dtype=torch.float32, device=dev),
                            tone_tab=torch.empty(tone_rule.table_words(S * (2 * most + 2), S * most), dtype=torch.int64, device=dev))
            self._upload_ramps(list(self._ramp_off))
        if self.shape_on:                             # dmel_shape_items: a state row per slot, the row the tone launch splices a shaping
            #                                           slot's piece into, the row its route reads the shaped samples from, the
            #                                           per-block outputs, the table and the arena of gain ramps
            w = self.chain_w
            self.buf.update(shape=torch.zeros(S, shape_rule.HEADER + self.shape_room, dtype=torch.int32, device=dev),
                            shape_out=torch.empty(S, w + self.shape_room, dtype=torch.float32, device=dev),
                            shape_peak=torch.zeros(S, (w + self.shape_room) // shape_rule.MIN_BLOCK + 2, dtype=torch.float32, device=dev),
                            shape_gain=torch.zeros(S, (w + self.shape_room) // shape_rule.MIN_BLOCK + 2, dtype=torch.float32, device=dev),
                            shape_tab=torch.empty(shape_rule.TABLE_WORDS * S, dtype=torch.int32, device=dev),
                            shape_ramps=torch.zeros(max(2 * self._sramp_floats, 4 * tone_rule.MAX_RAMP), dtype=torch.float32, device=dev))
            if self.tones_on:
                self.buf["shape_in"] = torch.empty(S, w, dtype=torch.float32, device=dev)
            self._upload_shape_ramps(list(self._sramp_off))
        if self.pace_on:                              # dmel_pace_items: a state row per slot, the row its route (or its shaper) reads the
            #                                           paced samples from, the per-frame outputs, the table and the arena of weights
            w = pace_rule.max_out(self.cap * self.up + self.fade_max, pace_rule.MAX_HOP, pace_rule.MAX_SEARCH)
            frames = pace_rule.max_out(self.cap * self.up + self.fade_max, pace_rule.MIN_HOP, pace_rule.MAX_SEARCH) // pace_rule.MIN_HOP
            self.buf.update(pace=torch.zeros(S, pace_rule.HEADER + 2 * pace_rule.MAX_HOP + 2 * pace_rule.MAX_SEARCH, dtype=torch.int32, device=dev),
                            pace_out=torch.empty(S, w, dtype=torch.float32, device=dev),
                            pace_off=torch.zeros(S, frames, dtype=torch.int32, device=dev),
                            pace_score=torch.zeros(S, frames, dtype=torch.float32, device=dev),
                            pace_tab=torch.empty(pace_rule.TABLE_WORDS * S, dtype=torch.int32, device=dev),
                            pace_w=torch.zeros(max(2 * self._pw_floats, 4 * pace_rule.MAX_HOP), dtype=torch.float32, device=dev))
            self._upload_pace_weights(list(self._pw_off))

    def _slot_views(self, s: int):
        b = self.buf
        return (b["hist"][:, s], b["skip"][s], b["cond"][s], b["mel"][s])

    def _rebase(self, s: int, st, room=None) -> None:
        """make room for the frames of step `st` in slot s: drop the columns nothing reads again and shift that slot's rows.  room:
        the step whose need_from says what is still read, when that is not st's own (a cross-fading slot keeps one frame more)"""
        new = decode_rebase(self.origin[s], room or st, self.cap)
        shift = new - self.origin[s]
        if shift <= 0:
            return
        keep = max(0, st.z[0] - new)                  # nothing behind the condition frontier has been written
        if keep:
            for v in self._slot_views(s):
                v[..., :keep] = v[..., shift:shift + keep].clone()
        self.origin[s] = new

    # -- a session leaves its slot and comes back (models/stream_park.py) ----------------------------------------------------
    _park_kind, _park_windowed, _own_rate_of, _resamples_in = "decode", ("hist.", "skip", "cond", "mel"), "vocoder's", False
    _live_window = staticmethod(decode_live_window)

    def _park_meta(self, s: int) -> dict:
        sch = self.sched[s]
        meta = dict(super()._park_meta(s), return_audios=self.return_audios, fade=self.fade[s], has_tail=self.has_tail[s],
                    lookahead=sch.lookahead if isinstance(sch, EarlyDecodeSchedule) else None, tok_origin=self.tok_origin[s],
                    n_noise=self.n_noise[s])
        if self.tones_on:                             # only a pool that sends tones writes the keys: the others' snapshots are unchanged
            meta.update(tones=[[P, plain(p)] for P, p in self.tq[s]], handed=self.handed[s], tone_samples=self.tone_samples[s])
        if self.scfg[s] is not None:                  # only a shaping session carries the keys: the others' snapshots are unchanged
            segs, base = shape_rule.live(self.sreq[s], self.sbase[s], self.sfed[s])
            meta.update(shape=self.scfg[s].as_dict(), shape_segments=[list(sg) for sg in segs], shape_base=base, shape_fed=self.sfed[s],
                        shape_hold=self.shold[s], shape_end=self.send[s])
        if self.pcfg[s] is not None:                  # only a pacing session carries the keys: the others' snapshots are unchanged
            meta.update(pace=self.pcfg[s].as_dict(), pace_ints=list(self.pints[s]), pace_requests=[list(r) for r in self.preq[s]],
                        pace_base=self.pbase[s])
        return meta

    def _park_pace(self, meta: Mapping):
        """(the pacing config a snapshot carries (None: none), its live requests, the rate in force, its integers); ValueError
        where they are none this pool can continue"""
        if meta.get("pace") is None:
            return None, [], None, pace_rule.FRESH
        if not self.pace_on:
            raise ValueError("a pacing session into a pool built without pace=True")
        try:
            cfg = pace_rule.PaceConfig.from_dict(meta["pace"])
        except TypeError as e:
            raise ValueError(f"the pace config of the snapshot is not a PaceConfig: {e}") from None
        H, D = cfg.samples(self.voc_rate)
        ints, base, raw = (meta.get(k) for k in ("pace_ints", "pace_base", "pace_requests"))
        ok = isinstance(ints, (list, tuple)) and len(ints) == 4 and all(isinstance(v, int) and not isinstance(v, bool) and v >= 0 for v in ints)
        if ok:
            K, a_prev, a_next, fed = ints
            ok = (a_prev == a_next == 0) if K == 0 else (H // 2 <= a_next - a_prev <= 2 * H and a_next <= fed + 2 * H)
        if not ok:
            raise ValueError(f"the pacer's integers of the snapshot are none the rule makes: {ints!r}")
        pace_rule.check_permille(base)
        if not isinstance(raw, (list, tuple)) or len(raw) > pace_rule.MAX_REQUESTS:
            raise ValueError(f"the rate requests of the snapshot are no list of at most {pace_rule.MAX_REQUESTS} (P, permille): {raw!r}")
        reqs, after = [], 0
        for q in raw:
            reqs.append(pace_rule.check_request(tuple(q) if isinstance(q, (list, tuple)) else q, 0, after))
            after = reqs[-1][0]
        return cfg, reqs, base, tuple(ints)

    def _park_shape(self, meta: Mapping):
        """(the shaping config a snapshot carries (None: none), its live segments, base gain, samples fed, samples held, end);
        ValueError where they are none this pool can continue"""
        if meta.get("shape") is None:
            return None, [], None, 0, 0, None
        if not self.shape_on:
            raise ValueError("a shaping session into a pool built without shape=True")
        try:
            cfg = shape_rule.ShapeConfig.from_dict(meta["shape"])
        except TypeError as e:
            raise ValueError(f"the shape config of the snapshot is not a ShapeConfig: {e}") from None
        N = cfg.block(self.voc_rate)
        fed, hold, end, base, raw = (meta.get(k) for k in ("shape_fed", "shape_hold", "shape_end", "shape_base", "shape_segments"))
        ints = all(isinstance(v, int) and not isinstance(v, bool) for v in (fed, hold) + (() if end is None else (end,)))
        if not ints or fed < 0 or not 0 <= hold <= min(fed, 2 * N - 1 if cfg.limit else 0) or (end is not None and end < fed):
            raise ValueError(f"the shaper's counts of the snapshot are no counts: fed {fed!r}, hold {hold!r}, end {end!r}")
        if isinstance(base, bool) or not isinstance(base, (int, float)) or not 0 <= base <= cfg.max_gain:
            raise ValueError(f"the shaper's base gain of the snapshot is no gain in [0, {cfg.max_gain}]: {base!r}")
        segs, after = [], 0
        ok = isinstance(raw, (list, tuple)) and len(raw) <= shape_rule.MAX_SEGMENTS and all(isinstance(q, (list, tuple)) and len(q) == 4
                                                                                          for q in raw)
        for q in raw if ok else ():
            P, g1, ramp = shape_rule.check_request((q[0], q[2], q[3]), cfg, after)
            shape_rule.check_request((P, q[1], ramp), cfg, after)
            segs.append((P, float(q[1]), g1, ramp))
            after = P
        if not ok:
            raise ValueError(f"the gain segments of the snapshot are no list of at most {shape_rule.MAX_SEGMENTS} (P, g0, g1, ramp): {raw!r}")
        return cfg, segs, float(base), fed, hold, end

    def _park_tones(self, meta: Mapping) -> list:
        """the pending requests a snapshot carries as [(P, checked program)] (a snapshot without the key: none); ValueError where
        they are no requests this pool can send"""
        pend = meta.get("tones") or []
        if pend and not self.tones_on:
            raise ValueError("a session with pending tone requests into a pool built without tones=True")
        reqs, last = [], 0
        for q in pend:
            if len(q) != 2 or isinstance(q[0], bool) or not isinstance(q[0], int) or q[0] < last or q[0] % self.up:
                raise ValueError(f"the tone requests of the snapshot are no [P, program] list with anchors in order: {q!r}")
            reqs.append((q[0], self._check_tones(tone_rule.check_program(q[1], self.voc_rate), meta["rate"])))
            last = q[0]
        n = sum(tone_rule.length(p) for _, p in reqs)
        if n > self.max_tone:
            raise ValueError(f"{n} pending tone samples exceed this pool's max_tone_samples = {self.max_tone}")
        if sum(len(p) for _, p in reqs) > tone_rule.MAX_SEGMENTS:
            raise ValueError(f"more than {tone_rule.MAX_SEGMENTS} pending segments")
        return reqs

    def _park_schedule(self, meta: Mapping):
        return (DecodeSchedule if meta["lookahead"] is None else EarlyDecodeSchedule).from_state(self.geo, meta["schedule"])

    def _park_shapes(self, meta: Mapping) -> List[Tuple[str, int, int]]:
        W, rs = meta["window"][1] - meta["window"][0], meta["resampler"]
        exact = meta["schedule"] if meta["lookahead"] is None else meta["schedule"]["exact"]
        return ([(f"hist.{l}", self.C, W) for l in range(self.L + 1)] +
                [("skip", self.C, W), ("cond", meta["cond_channels"], W), ("mel", meta["n_mels"], W),
                 ("tokens", self.G, exact["tokens"] - meta["tok_origin"]), ("noise", self.C, meta["n_noise"]),
                 ("fade_tail", 1, meta["fade"] if meta["has_tail"] else 0), ("resampler", 1, rs["fill"] if rs else 0)] +
                # the shaper's row: header and hold; a session that has fed no sample owns the zeroed row: nothing
                ([("shape", 1, shape_rule.ShapeConfig.from_dict(meta["shape"]).state_words(self.voc_rate) if meta["shape_fed"] > 0 else 0)]
                 if meta.get("shape") is not None else []) +
                # the pacer's row: header and held samples, likewise
                ([("pace", 1, pace_rule.PaceConfig.from_dict(meta["pace"]).state_words(self.voc_rate) if meta["pace_ints"][3] > 0 else 0)]
                 if meta.get("pace") is not None else []))

    def _park_rows(self, s: int) -> Dict[str, torch.Tensor]:
        b = self.buf
        rows = {"skip": b["skip"][s], "cond": b["cond"][s], "mel": b["mel"][s], "tokens": b["tokens"][s], "noise": b["noise"][s]}
        for l in range(self.L + 1):
            rows[f"hist.{l}"] = b["hist"][l, s]
        if "fade_tail" in b:
            rows["fade_tail"] = b["fade_tail"][s:s + 1]
        if self.rs is not None and self.rs.buf is not None:
            rows["resampler"] = self.rs.buf["rows"][s:s + 1]
        if self.shape_on:
            rows["shape"] = b["shape"][s:s + 1]
        if self.pace_on:
            rows["pace"] = b["pace"][s:s + 1]
        return rows

    def _park_widths(self):
        dec = self.codec.decoder
        return (("cond_channels", dec.condition_channels), ("n_mels", dec.output_channels), ("up", self.up), ("voc_rate", self.voc_rate))

    def _park_fits(self, meta: Mapping, sc) -> None:
        f = self.geo.factor
        if not self.return_audios and (meta["return_audios"] or meta["sample_format"] != "f32" or meta["channels"] != 1 or
                                       meta["rate"] is not None):
            raise ValueError("a session with audio (its format, rate or channels) into a pool built with return_audios=False")
        if meta["lookahead"] is not None and not self.early_emit:
            raise ValueError("a session with lookahead_frames into a pool built without early_emit=True: it has no shadow rows to "
                             "decode ahead in")
        if meta["fade"] > self.fade_max:
            raise ValueError(f"a session with crossfade_samples={meta['fade']} into a pool built with crossfade_samples={self.fade_max}")
        if meta["fade"] < 0 or (meta["fade"] and meta["lookahead"] is None) or (meta["has_tail"] and not meta["fade"]):
            raise ValueError("a cross-fade goes with a look-ahead, and a tail with a cross-fade")
        if meta["lookahead"] is not None and sc.fade_frames != (1 if meta["fade"] else 0):
            raise ValueError("the schedule's fade_frames do not go with the session's cross-fade")
        self._park_tones(meta)
        self._park_shape(meta)
        self._park_pace(meta)
        lo = meta["window"][0]
        if sc.tokens * f - lo + self.max_push * f > self.cap:
            raise ValueError(f"the frames [{lo}, {sc.tokens * f}) and one maximal push ({self.max_push * f} frames) do not fit the "
                             f"capacity {self.cap}")
        if not 0 <= sc.tokens - meta["tok_origin"] <= self.tok_width - self.max_push:
            raise ValueError(f"a token tail of {sc.tokens - meta['tok_origin']} tokens does not fit this pool's {self.tok_width}")
        if not 0 <= meta["n_noise"] <= self.noise_width - self.max_push * f:
            raise ValueError(f"a noise tail of {meta['n_noise']} frames does not fit this pool's {self.noise_width}")

    def _park_adopt(self, s: int, meta: Mapping) -> None:
        super()._park_adopt(s, meta)
        for name in ("tok_origin", "n_noise", "fade", "has_tail"):
            getattr(self, name)[s] = meta[name]
        self.tq[s] = self._park_tones(meta)
        self.tone_samples[s] = sum(tone_rule.length(p) for _, p in self.tq[s])
        # a snapshot written without the key: what the session has handed out follows from its schedule and its fade tail
        self.handed[s] = meta.get("handed", self.sched[s].emitted * self.up - (meta["fade"] if meta["has_tail"] else 0))
        for _, p in self.tq[s]:
            self._ramps_for(p)
        cfg, segs, base, fed, hold, end = self._park_shape(meta)
        self._shape_adopt(s, cfg, segs, base, fed, hold, end)
        for sg in segs:
            if sg[3] and sg[3] not in self._sramp_off:
                self._sramp_off[sg[3]], self._sramp_floats = self._sramp_floats, self._sramp_floats + sg[3]
                if self.buf is not None:
                    self._upload_shape_ramps([sg[3]])
        self._pace_adopt(s, *self._park_pace(meta))

    def _prepare_slot(self, s: int) -> None:
        super()._prepare_slot(s)
        if self.fade[s]:                              # not state: rebuilt from F, for a fresh slot and for a restored one
            self.buf["fade_w"][s, :self.fade[s]] = crossfade.weights(self.fade[s]).to(self.buf["fade_w"].device)
        if self.shape_on:
            self.buf["shape"][s].zero_()              # the fresh shaper state
        if self.pace_on:
            self.buf["pace"][s].zero_()               # the fresh pacer state

    # -- one step ----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def push(self, ids: Mapping[int, torch.Tensor], noise: Optional[Mapping[int, torch.Tensor]] = None,
             final: Iterable[int] = ()) -> Dict[int, Tuple[Optional[torch.Tensor], torch.Tensor]]:
        """ids: {slot: (G, n) int, n >= 0}; noise: {slot: (C, n * factor)} for any of them; final: slots that end with these tokens
        -> {slot: (audio (1, m * up) | None, mel (n_mels, m))} for the m >= 0 frames of that slot that became final with this step"""
        final = set(final)
        self._validate(ids, noise, final)
        dev = next(iter(ids.values())).device
        self._ensure_buffers(dev)
        with torch.cuda.device(dev):
            steps, early = self._intake(ids, noise, final, dev)
            shadows = {s: es for s, es in early.items() if es.shadow}
            ahead = self._quantise(steps, shadows, dev)
            live = {s: st for s, st in steps.items() if st.next != st.prev}
            if shadows:
                self._fork(shadows, ahead, live)
            if live:
                self._wavenet(live)
            # a slot with a look-ahead emits by its own rule, from its shadow row when that ran ahead of the committed one
            steps = {s: early.get(s, st) for s, st in steps.items()}
            row = {s: self.S + s if s in shadows else s for s in steps}
            self._held, self._ending, self._shape_src, self._pace_src = {}, final, {}, {}
            out, pieces, wire = self._emit(steps, row, final, dev)
            self._flush_tails(steps, final, out, pieces, wire)
            if self.pace_on:
                self._pace(steps, final, out, pieces, wire, dev)
            placed = self.tones_on and self._tones(steps, final, out, pieces, wire, dev)
            if self.shape_on:
                self._shape(steps, final, out, pieces, wire, dev, placed)
            self._resample(steps, final, out, pieces, wire, dev, placed)
            self._to_wire(out, wire)
        self._release(final)
        return out

    def _intake(self, ids, noise, final, dev) -> Tuple[dict, dict]:
        """tokens and noise behind the slots' tails, the schedules stepped, the slots re-based
        -> ({slot: the step of its committed row}, {slot: EarlyDecodeStep of the slots opened with a look-ahead})"""
        b, f = self.buf, self.geo.factor
        steps, early = {}, {}
        for s, t in ids.items():
            if self._fresh[s]:
                self._prepare_slot(s)
            sch, n = self.sched[s], t.shape[1]
            if n:
                at = sch.tokens - self.tok_origin[s]
                b["tokens"][s, :, at:at + n] = t.to(torch.int32)
                z = noise.get(s) if noise else None
                if z is None:
                    z = torch.randn(self.C, n * f, dtype=torch.float32, device=dev)
                b["noise"][s, :, self.n_noise[s]:self.n_noise[s] + n * f] = z.to(dev, torch.float32)
                self.n_noise[s] += n * f
            st = sch.step(n, s in final)
            room = None
            if isinstance(sch, EarlyDecodeSchedule):
                early[s], st = st, st.step         # the committed row runs the exact schedule's step, as an exact slot's does
                room = early[s] if early[s].fade else None
            steps[s] = st
            self._rebase(s, st, room)
        return steps, early

    def _quantise(self, steps, shadows, dev) -> list:
        """quantiser: ONE call over every slot with new condition frames, whatever the lengths of their token windows, cropped per
        slot.  A slot that decodes ahead needs no item of its own: its window ends at its newest token already, so the frames the
        committed row leaves waiting for right context are the shadow row's -> [(slot, its row of z, that row's first frame)]"""
        b, codec, f = self.buf, self.codec, self.geo.factor
        members = [s for s, st in steps.items() if st.z[1] > st.z[0] or s in shadows]
        ahead = []
        if not members:
            return ahead
        tok_win = {s: shadows[s].tok_window if s in shadows else steps[s].tok_window for s in members}
        wins = [b["tokens"][s, :, tok_win[s][0] - self.tok_origin[s]:tok_win[s][1] - self.tok_origin[s]] for s in members]
        tok_batch, widths = pad_windows(wins)
        if widths is None:
            wl = torch.full((len(members),), tok_batch.shape[-1], dtype=torch.int64, device=dev)
            z, _ = codec.get_quantized_features_from_indices(tok_batch, wl)
        else:
            wl = torch.tensor(widths, dtype=torch.int64).to(dev, non_blocking=True)
            z, _ = codec.get_quantized_features_from_indices(tok_batch, wl, item_features=True)
        for i, s in enumerate(members):
            st, o = steps[s], self.origin[s]
            lo = tok_win[s][0] * f
            k = st.z[1] - st.z[0]
            if k:
                b["cond"][s, :, st.z[0] - o:st.z[1] - o] = z[i, :, st.z[0] - lo:st.z[1] - lo]
                b["hist"][0, s, :, st.z[0] - o:st.z[1] - o] = b["noise"][s, :, :k]
                rest = self.n_noise[s] - k
                if rest:
                    b["noise"][s, :, :rest] = b["noise"][s, :, k:k + rest].clone()
                self.n_noise[s] = rest
            if s in shadows:
                ahead.append((s, z[i], lo))
            drop = st.tok_keep_from - self.tok_origin[s]
            if drop > 0:
                keep = st.tokens - st.tok_keep_from
                b["tokens"][s, :, :keep] = b["tokens"][s, :, drop:drop + keep].clone()
                self.tok_origin[s] = st.tok_keep_from
        return ahead

    def _fork(self, shadows, ahead, live) -> None:
        """fork: ONE launch copies, for every slot that decodes ahead, the committed columns its shadow row reads -- every level's
        history, the partial skip sums, condition and mel -- into row S + slot.  In front of the committed step, so that the shadow
        starts from the frontiers that step starts from and both go through the one WaveNet call (the shadow rows join `live`).
        The window is widened to whole 16-byte vectors: what the copy adds in front is never read, what it adds behind is written
        next (condition, level 0) or recomputed by the shadow step (the other levels, skip, mel)"""
        b, S = self.buf, self.S
        I64 = C.c_int64 * len(shadows)
        lo = [(es.fork[0] - self.origin[s]) // 4 * 4 for s, es in shadows.items()]
        hi = [(es.fork[1] - self.origin[s] + 3) // 4 * 4 for s, es in shadows.items()]
        _lib.check(_lib.lib().dmel_stream_fork_items(
            b["hist"].data_ptr(), b["skip"].data_ptr(), b["cond"].data_ptr() if b["cond"].shape[1] else None, b["mel"].data_ptr(),
            self.L, self.N, self.C, b["cond"].shape[1], b["mel"].shape[1], self.cap, len(shadows), I64(*shadows),
            I64(*[S + s for s in shadows]), I64(*lo), I64(*hi), b["fork_tab"].data_ptr(), _lib.stream_ptr()), "stream_fork_items")
        for s, zi, lo_z in ahead:              # behind the committed frontier: the waiting frames, with the waiting noise
            es, o = shadows[s], self.origin[s]
            b["cond"][S + s, :, es.z[0] - o:es.z[1] - o] = zi[:, es.z[0] - lo_z:es.z[1] - lo_z]
            b["hist"][0, S + s, :, es.z[0] - o:es.z[1] - o] = b["noise"][s, :, :es.z[1] - es.z[0]]
            live[S + s] = es                   # prev: the committed frontiers, next: the newest frame on every level

    def _wavenet(self, live) -> None:
        """decoder WaveNet: every level of every slot advances to its own new frontier, in one layered step over all slots"""
        b, N = self.buf, self.N
        prev, nxt, org = session_rows(N, live, self.origin * (N // self.S))
        rows = C.c_int64 * (N * (self.L + 1))
        _lib.check(_lib.lib().dmel_wavenet_stream_step_items_layered(
            self.codec.decoder.native(), None, b["hist"].data_ptr(), b["skip"].data_ptr(), b["cond"].data_ptr(), b["mel"].data_ptr(),
            b["scratch"].data_ptr(), N, self.cap, rows(*prev), rows(*nxt), None, 1, (C.c_int64 * N)(*org), _lib.stream_ptr()),
            "wavenet_stream_step_items_layered")

    def _route(self, s: int, piece: torch.Tensor, out, pieces, wire) -> None:
        """a new float piece (1, n) of slot s goes to the resampler, else to the wire convert, else it is cloned out; in a pool that
        sends tones it is held where a request of the slot is due in this step: the tone launch splices and routes it"""
        if self.tones_on:
            self.handed[s] += piece.shape[1]
            if self.tq[s] and (s in self._ending or self.tq[s][0][0] <= self.handed[s]):
                self._held[s] = piece[0]
                return
        if self.pcfg[s] is not None:                  # a pacing slot's piece is the pacer's source; its route takes what that emits
            self._pace_src[s] = piece[0]
            return
        if self.scfg[s] is not None:                  # a shaping slot's piece is the shaper's source; its route takes what that emits
            self._shape_src[s] = piece[0]
            return
        if self._converts(s):
            pieces[s] = piece[0]
        elif self._wired(s):
            wire[s] = piece[0]
        else:
            out[s] = (piece.clone(), out[s][1])

    def _emit(self, steps, row, final, dev) -> Tuple[dict, dict, dict]:
        """emit: the mel frames whose vocoder context exists; ONE vocoder call over every slot that has a window -> (out, pieces: the new
        audio of the slots that leave at another rate, still in the vocoder's batch, wire: that of the non-f32 and multi-channel slots)"""
        b, up = self.buf, self.up
        out, members = {}, []
        for s, st in steps.items():
            o = self.origin[s]
            mel = b["mel"][row[s], :, st.emit[0] - o:st.emit[1] - o].clone()
            out[s] = (torch.empty((1, 0) if self.ch[s] == 1 else (0, self.ch[s]), dtype=pcm.FORMATS[self.fmt[s]][1], device=dev)
                      if self.return_audios else None, mel)
            if st.voc_window[1] > st.voc_window[0]:
                members.append(s)
        pieces, wire = {}, {}
        if not members:
            return out, pieces, wire
        wins = [b["mel"][row[s], :, steps[s].voc_window[0] - self.origin[s]:steps[s].voc_window[1] - self.origin[s]] for s in members]
        mel_batch, widths = pad_windows(wins)
        wav = self.codec.vocoder(mel_batch) if widths is None else self.codec.vocoder(mel_batch, lengths=widths)
        # ---- cross-fade: ONE launch blends, in place in the vocoder's batch, the F samples in front of every fading slot's new
        # piece with the tail the slot held back, and saves the piece's last F samples as the new tail (not on a final step).
        # The piece handed on is the view shifted by F; the two regions of a row lie a whole frame (up >= F samples) apart
        fading = [(i, s) for i, s in enumerate(members) if self.fade[s]]
        cut = {}                                                   # slot -> (samples taken in front, samples held back)
        if fading:
            rows = []
            for i, s in fading:
                st, F = steps[s], self.fade[s]
                a, e = (st.emit[0] - st.voc_window[0]) * up, (st.emit[1] - st.voc_window[0]) * up
                cut[s] = (F if self.has_tail[s] else 0, 0 if s in final else F)
                rows.append((wav[i, 0, a - F:a] if self.has_tail[s] else None, b["fade_tail"][s, :F],
                             None if s in final else wav[i, 0, e - F:e], b["fade_w"][s, :F]))
                self.has_tail[s] = s not in final
            rows = [r for r in rows if r[0] is not None or r[2] is not None]
            if rows:
                crossfade.crossfade_items(rows, table=b["fade_tab"])
        for i, s in enumerate(members):
            st, (front, back) = steps[s], cut.get(s, (0, 0))
            lo = st.voc_window[0]
            self._route(s, wav[i, :, (st.emit[0] - lo) * up - front:(st.emit[1] - lo) * up - back], out, pieces, wire)
        return out, pieces, wire

    def _flush_tails(self, steps, final, out, pieces, wire) -> None:
        """a fading slot that ends without new frames: its tail leaves as it is"""
        for s in final:
            if self.has_tail[s] and s in steps:
                self._route(s, self.buf["fade_tail"][s, :self.fade[s]][None], out, pieces, wire)
                self.has_tail[s] = False

    def _pace(self, steps, final, out, pieces, wire, dev) -> None:
        """pace: ONE dmel_pace_items launch takes, for every pacing slot of the step with a new piece or its end, the piece (as the
        vocoder, the cross-fade or the flushed fade tail left it) through the pacer, and writes the samples that leave -- advance()
        of them, known from integers -- where the slot's route reads them: its row of a staging buffer (the shaper's source where
        the session shapes; else the resampler copies it -- or the tone launch places it behind the tail with the step's other
        chunks --, or the convert launch reads it), or a fresh tensor that is handed out."""
        members = [s for s in steps if self.pcfg[s] is not None and (s in final or (s in self._pace_src and self._pace_src[s].shape[0]))]
        if not members:
            return
        b, S = self.buf, self.S
        src, dst, cfgs, reqs, fin = [None] * S, [None] * S, [None] * S, [[] for _ in range(S)], [False] * S
        ints, base = [pace_rule.FRESH] * S, [None] * S
        for s in members:
            cfg, x = self.pcfg[s], self._pace_src.get(s)
            n = 0 if x is None else x.shape[0]
            H, D = cfg.samples(self.voc_rate)
            m = pace_rule.advance(self.pints[s], self.preq[s], n, s in final, H, D, self.pbase[s])[2]
            if self.scfg[s] is not None:
                d = self._shape_src[s] = b["pace_out"][s, :m]
            elif self._converts(s):
                d = b["pace_out"][s, :m]
                if m or s in final:
                    pieces[s] = d
            elif self._wired(s):
                d = wire[s] = b["pace_out"][s, :m]
            else:
                d = torch.empty(1, m, dtype=torch.float32, device=dev)
                out[s], d = (d, out[s][1]), d[0]
            src[s], dst[s], cfgs[s], reqs[s], ints[s], base[s], fin[s] = x if n else None, d, cfg, self.preq[s], self.pints[s], self.pbase[s], s in final
        _, after, frames = pace_rule.pace_items(src, dst, cfgs, reqs, ints, fin, b["pace"], b["pace_off"], b["pace_score"], self.voc_rate,
                                                weights=b["pace_w"], weight_off=self._pw_off, table=b["pace_tab"], initial=base)
        for s in members:                             # behind the launch: a refused launch changes no count
            self.pints[s], self._pace_n[s] = after[s], frames[s]
            self.preq[s], self.pbase[s] = pace_rule.live(self.preq[s], self.pbase[s], after[s][2])

    def _tones(self, steps, final, out, pieces, wire, dev) -> bool:
        """tones: ONE dmel_tone_items launch composes, for every slot with a request that is due -- its anchor P lies at or in front
        of the end h1 of the speech the slot has handed out with this step, or the step is the slot's last --, the piece
        speech[h0:P1] | tone 1 | speech[P1:P2] | ... straight where the slot's route reads it: behind its resampler tail, in its
        row of the staging buffer the convert launch reads, or in a fresh tensor of the step that is handed out (in place of the
        clone).  The resampler takes placed chunks or copied ones, not both: where one of the spliced slots leaves at another
        rate, the launch also copies the pieces of the step's other such slots behind their tails (the copy rs.push would make)
        -> whether it did"""
        held = self._held
        for s in steps:                               # a slot without a piece in this step serves what is due all the same
            if s not in held and self.tq[s] and (s in final or self.tq[s][0][0] <= self.handed[s]):
                held[s] = torch.empty(0, dtype=torch.float32, device=dev)
        if not held:
            return False
        b, plan = self.buf, {}
        for s, x in held.items():
            due = [q for q in self.tq[s] if s in final or q[0] <= self.handed[s]]
            plan[s] = (due, x.shape[0] + sum(tone_rule.length(p) for _, p in due))
        routed = [s for s in held if self.scfg[s] is None]      # a shaping slot's splice goes to the shaper's staging row instead
        placed = any(self._converts(s) for s in routed)
        if placed:
            behind = self.rs.destinations({s: plan[s][1] if s in plan else pieces[s].shape[0]
                                           for s in list(pieces) + [s for s in routed if self._converts(s)]})
        parts = []
        for s, x in held.items():
            (due, total), h0 = plan[s], self.handed[s] - x.shape[0]
            if self.scfg[s] is not None:
                d = self._shape_src[s] = b["shape_in"][s, :total]
            elif self._converts(s):
                d = pieces[s] = behind[s]
            elif self._wired(s):
                d = wire[s] = b["tone_stage"][s, :total]
            else:
                d = torch.empty(1, total, dtype=torch.float32, device=dev)
                out[s], d = (d, out[s][1]), d[0]
            at = a = 0                                # samples of d written, samples of x consumed
            for P, program in due:
                c = min(max(P - h0, a), x.shape[0])
                if c > a:
                    parts.append((d[at:at + c - a], x[a:c]))
                    at, a = at + c - a, c
                n = tone_rule.length(program)
                parts.append((d[at:at + n], program))
                at += n
            if x.shape[0] > a:
                parts.append((d[at:at + x.shape[0] - a], x[a:]))
        if placed:
            for s, y in pieces.items():
                if s not in held:
                    if y.shape[0]:
                        parts.append((behind[s], y))
                    pieces[s] = behind[s]
        tone_rule.tone_items(parts, self.voc_rate, sine=b["tone_sine"], ramps=b["tone_ramps"], ramp_off=self._ramp_off,
                             table=b["tone_tab"])
        for s, x in held.items():                     # behind the launch: a refused launch loses no request
            due, total = plan[s]
            del self.tq[s][:len(due)]
            self.tone_samples[s] -= total - x.shape[0]
        return placed

    def _shape(self, steps, final, out, pieces, wire, dev, placed: bool) -> None:
        """shape: ONE dmel_shape_items launch takes, for every shaping slot of the step with a new piece or its end, the piece (as the
        vocoder or the tone launch left it) through commanded gain and limiter, and writes the samples that leave -- emitted() of
        them, known from integers -- where the slot's route reads them: its row of a staging buffer (the resampler copies it, the
        convert launch reads it; behind the resampler tail where the tone launch placed the step's chunks), or a fresh tensor that
        is handed out.  A slot that ends without a new piece takes part: its hold is flushed."""
        members = [s for s in steps if self.scfg[s] is not None and (s in final or (s in self._shape_src and self._shape_src[s].shape[0]))]
        if not members:
            return
        b, S = self.buf, self.S
        src, dst, cfgs, segs, base = [None] * S, [None] * S, [None] * S, [[] for _ in range(S)], [0.0] * S
        pos, hold, fin, took = [0] * S, [0] * S, [False] * S, {}
        for s in members:
            cfg, x = self.scfg[s], self._shape_src.get(s)
            n = 0 if x is None else x.shape[0]
            if self.send[s] is not None:              # a stopped session: z is cut at E
                n = max(0, min(n, self.send[s] - self.sfed[s]))
            m = shape_rule.emitted(self.shold[s], n, cfg.block(self.voc_rate), s in final, cfg.limit)
            if self._converts(s):
                d = self.rs.destinations({s: m})[s] if placed else b["shape_out"][s, :m]
                if m or s in final:
                    pieces[s] = d
            elif self._wired(s):
                d = wire[s] = b["shape_out"][s, :m]
            else:
                d = torch.empty(1, m, dtype=torch.float32, device=dev)
                out[s], d = (d, out[s][1]), d[0]
            segs[s], base[s] = shape_rule.live(self.sreq[s], self.sbase[s], self.sfed[s])
            src[s], dst[s], cfgs[s], pos[s], hold[s], fin[s], took[s] = x[:n] if n else None, d, cfg, self.sfed[s], self.shold[s], s in final, (n, m)
        shape_rule.shape_items(src, dst, cfgs, segs, base, pos, hold, fin, b["shape"], b["shape_peak"], b["shape_gain"], self.voc_rate,
                               ramps=b["shape_ramps"], ramp_off=self._sramp_off, table=b["shape_tab"])
        for s, (n, m) in took.items():                # behind the launch: a refused launch changes no count
            cfg = self.scfg[s]
            self._shape_n[s] = shape_rule.completed(self.shold[s], n, cfg.block(self.voc_rate), s in final, cfg.limit)
            self.sfed[s], self.shold[s] = self.sfed[s] + n, self.shold[s] + n - m
            self.sreq[s], self.sbase[s] = shape_rule.live(segs[s], base[s], self.sfed[s])

    def _resample(self, steps, final, out, pieces, wire, dev, placed: bool = False) -> None:
        """the playback rates: each piece goes behind its slot's resampler tail, ONE launch converts all slots; a slot without a
        new piece still takes part when it ends (the outputs that waited for the end of its signal).  placed: the tone launch of
        the step has put the pieces there already"""
        if self.rs is None:
            return
        for s in steps:
            if self._converts(s) and s not in pieces and s in final:
                pieces[s] = torch.empty(0, dtype=torch.float32, device=dev)
        if pieces:
            for s, y in self.rs.push(pieces, final & set(pieces), placed=placed).items():
                if self._wired(s):
                    wire[s] = y
                else:
                    out[s] = (y[None], out[s][1])

    def _to_wire(self, out, wire) -> None:
        """the wire's format and channels: ONE launch converts every non-f32 or multi-channel slot's new piece into one packed buffer of
        the step (pcm.convert_packed); the tensors handed out are views of it, int16 for s16, uint8 for G.711, (n, c) for c > 1 channels"""
        wire = {s: y for s, y in wire.items() if y.shape[0]}
        if wire:
            dsts = pcm.convert_packed(list(wire.values()), [self.fmt[s] for s in wire], [self.ch[s] for s in wire], self.buf["pcm_tab"])
            for s, d in zip(wire, dsts):
                out[s] = (d[None] if self.ch[s] == 1 else d, out[s][1])

    def close(self, slot: int):
        """no more tokens for this slot: its remaining (audio, mel), and the slot is free"""
        self._check_open(slot)
        return self.push({slot: torch.empty(self.G, 0, dtype=torch.int32, device=self._device())}, final=(slot,))[slot]
