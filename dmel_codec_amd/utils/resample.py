"""Sample-rate conversion on the MI355X: `torchaudio.functional.resample(x, orig_freq, new_freq)` as the reference calls it in
LogMelSpectrogram.forward(x, sample_rate=...) (utils/spectrogram.py:122-123; torchaudio's defaults: sinc_interp_hann,
lowpass_filter_width 6, rolloff 0.99).  The polyphase filter bank is built once per (orig, new, device) on the host, the filtering is
one HIP launch (csrc/small_ops.hip: resample_kernel, through torch.ops.dmel_hip.resample).  StreamResampler is the same conversion fed
chunk by chunk (torch.ops.dmel_hip.resample_window -> dmel_resample_window_f32): same kernel, same bits.  SessionResampler is a pool
of such streams, each at its own rate pair, converted by ONE launch per step (dmel_resample_window_items_f32)."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Iterable, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib
from ..models.stream_schedule import ResampleSchedule, resample_max_outputs, resample_session_rows

_banks: dict = {}


def sinc_resample_bank(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """(new_freq // gcd, 2 * width + orig_freq // gcd) float32 filter bank and `width`, torchaudio's `_get_sinc_resample_kernel` for
    resampling_method="sinc_interp_hann", evaluated in float32 like torchaudio does for float32 waveforms."""
    g = math.gcd(int(orig_freq), int(new_freq))
    orig, new = int(orig_freq) // g, int(new_freq) // g
    if lowpass_filter_width <= 0:
        raise ValueError("Low pass filter width should be positive.")
    base_freq = np.float32(min(orig, new) * rolloff)
    width = int(math.ceil(lowpass_filter_width * orig / (min(orig, new) * rolloff)))
    f32 = np.float32
    idx = (np.arange(-width, width + orig, dtype=np.float32) / f32(orig))[None, :]
    t = (np.arange(0, -new, -1, dtype=np.float32) / f32(new))[:, None] + idx
    t = t * base_freq
    t = np.clip(t, f32(-lowpass_filter_width), f32(lowpass_filter_width))
    window = np.cos(t * f32(math.pi) / f32(lowpass_filter_width) / f32(2)) ** 2
    t = t * f32(math.pi)
    scale = f32(base_freq / f32(orig))
    with np.errstate(invalid="ignore", divide="ignore"):
        kern = np.where(t == 0, f32(1.0), np.sin(t) / t)
    kern = (kern * window * scale).astype(np.float32)
    return kern, width, orig, new


@torch.library.custom_op("dmel_hip::resample", mutates_args=(), device_types="cuda")
def _resample_op(x: torch.Tensor, bank: torch.Tensor, orig: int, new: int, width: int) -> torch.Tensor:
    B, L = x.shape
    Lout = (new * L + orig - 1) // orig
    y = torch.empty(B, Lout, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().dmel_resample_f32(x.data_ptr(), y.data_ptr(), bank.data_ptr(), B, L, Lout, orig, new, width,
                                                _lib.stream_ptr()), "resample")
    return y


@_resample_op.register_fake
def _(x, bank, orig, new, width):
    return x.new_empty((x.shape[0], (new * x.shape[1] + orig - 1) // orig), dtype=torch.float32)


@torch.library.custom_op("dmel_hip::resample_window", mutates_args=(), device_types="cuda")
def _resample_window_op(x: torch.Tensor, bank: torch.Tensor, orig: int, new: int, width: int, s0: int, o0: int, n_out: int,
                        total_length: int) -> torch.Tensor:
    """x (B, n) fp32, rows contiguous (any row stride): the absolute samples [s0, s0 + n) of a stream -> its absolute outputs
    [o0, o0 + n_out), each with the bits resample() gives it on the whole clip.  total_length: the stream's length, -1 while unknown."""
    if x.ndim != 2 or x.dtype != torch.float32 or x.stride(-1) != 1:
        raise ValueError("expected a (B, n) fp32 tensor with contiguous rows")
    B, n = x.shape
    y = torch.empty(B, n_out, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().dmel_resample_window_f32(x.data_ptr(), x.stride(0) if B > 1 else max(n, x.stride(0)), n, s0, y.data_ptr(),
                                                       bank.data_ptr(), B, o0, n_out, total_length, orig, new, width,
                                                       _lib.stream_ptr()), "resample_window")
    return y


@_resample_window_op.register_fake
def _(x, bank, orig, new, width, s0, o0, n_out, total_length):
    return x.new_empty((x.shape[0], n_out), dtype=torch.float32)


def filter_bank(orig_freq: int, new_freq: int, device):
    """(bank on `device`, width, orig, new), orig / new in lowest terms; built once per (orig, new, device)"""
    key = (int(orig_freq), int(new_freq), str(device))
    if key not in _banks:
        kern, width, orig, new = sinc_resample_bank(orig_freq, new_freq)
        _banks[key] = (torch.from_numpy(kern).to(device).contiguous(), width, orig, new)
    return _banks[key]


def resample(waveform: torch.Tensor, orig_freq: int, new_freq: int) -> torch.Tensor:
    """waveform (..., L) fp32 on the GPU -> (..., ceil(new_freq * L / orig_freq))."""
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError("Original frequency and desired frequecy should be positive")
    if int(orig_freq) == int(new_freq):
        return waveform
    _lib.require_cuda(waveform, "waveform")
    bank, width, orig, new = filter_bank(orig_freq, new_freq, waveform.device)
    shape = waveform.shape
    x = waveform.float().reshape(-1, shape[-1]).contiguous()
    y = torch.ops.dmel_hip.resample(x, bank, orig, new, width)
    return y.reshape(*shape[:-1], y.shape[-1])


class StreamResampler:
    """resample() fed chunk by chunk: .push(x (B, n), final=False) -> y (B, m), the m >= 0 outputs that became final with these samples;
    .finish() flushes.  n is arbitrary (0, less than the filter's width, ...); the concatenated pieces are torch.equal to
    resample(whole, orig_freq, new_freq).  An output is final once its last tap has arrived, so mid-stream the resampler is at most
    `width + down` source samples behind (ResampleSchedule.samples_needed; 15 samples for 48 -> 24 kHz, 9 for 16 -> 24 kHz, 159 for
    44.1 -> 24 kHz), and whole phase groups are emitted.

    Carried on the device: the input tail the next outputs still read, fewer than kw = 2 width + down samples, at the front of one of
    two buffers of constant capacity (they grow only if a larger push arrives).  Per push: the chunk is copied behind the tail, ONE
    resample launch (dmel_resample_window_f32) reads the buffer, and the new tail is copied to the front of the other buffer.  No host
    synchronisation; everything runs on the current stream, so a caller keeps to one stream (or orders its streams itself).  Equal
    rates pass the chunks through untouched."""

    def __init__(self, orig_freq: int, new_freq: int, batch: int):
        self.sched = ResampleSchedule(orig_freq, new_freq)
        self.orig_freq, self.new_freq, self.B = int(orig_freq), int(new_freq), int(batch)
        self.identity = self.orig_freq == self.new_freq
        self.buf = self.spare = None      # (B, cap): buf[:, :fill] holds the absolute input samples [s0, s0 + fill)
        self.s0 = 0
        self.fill = 0
        self._dev = None                  # where the last push lived: finish() makes its empty chunk there

    @property
    def capacity(self) -> int:
        """samples per row of the carried buffer; does not grow with the stream"""
        return 0 if self.buf is None else self.buf.shape[1]

    @property
    def finished(self) -> bool:
        return self.sched.finished

    @torch.no_grad()
    def push(self, x: torch.Tensor, final: bool = False) -> torch.Tensor:
        _lib.require_cuda(x, "waveform")
        if x.ndim != 2 or x.shape[0] != self.B:
            raise ValueError(f"expected ({self.B}, n), got {tuple(x.shape)}")
        sc = self.sched
        n = x.shape[1]
        self._dev = x.device
        if self.identity:
            sc.step(n, final)
            return x
        st = sc.step(n, final)
        dev = x.device
        bank, width, orig, new = filter_bank(self.orig_freq, self.new_freq, dev)
        assert (width, orig, new) == (sc.width, sc.down, sc.up)
        if self.fill + n > self.capacity:
            cap = self.fill + n + sc.kw               # room for this chunk behind the longest tail: equal pushes never grow it again
            grown = torch.empty(self.B, cap, dtype=torch.float32, device=dev)
            if self.fill:
                grown[:, :self.fill] = self.buf[:, :self.fill]
            self.buf, self.spare = grown, torch.empty_like(grown)
        if n:
            self.buf[:, self.fill:self.fill + n] = x
            self.fill += n
        o0, o1 = st.outputs
        if o1 > o0:
            y = torch.ops.dmel_hip.resample_window(self.buf[:, :self.fill], bank, orig, new, width, self.s0, o0, o1 - o0, st.total_length)
        else:
            y = torch.empty(self.B, 0, dtype=torch.float32, device=dev)
        if final:
            self.buf = self.spare = None
            self.fill = 0
        elif st.keep_from > self.s0:
            drop = st.keep_from - self.s0
            keep = self.fill - drop
            if keep:
                self.spare[:, :keep] = self.buf[:, drop:self.fill]
            self.buf, self.spare = self.spare, self.buf
            self.s0, self.fill = st.keep_from, keep
        return y

    def finish(self) -> torch.Tensor:
        """no more samples: the outputs that were waiting for right context, computed with the true end of the signal"""
        dev = self._dev if self._dev is not None else torch.device("cuda", torch.cuda.current_device())
        return self.push(torch.empty(self.B, 0, dtype=torch.float32, device=dev), final=True)


class SessionResampler:
    """`slots` independent StreamResamplers, each at its own (orig, new) pair, served by ONE resample launch per step
    (dmel_resample_window_items_f32) whatever the number of slots and of rates among them.

        pool = SessionResampler(slots, pairs=[(48000, 24000), (16000, 24000)], max_push=n)
        pool.open(slot, 48000, 24000)                        # fresh schedule; a pair that was not declared is a ValueError
        pieces = pool.push({slot: chunk_1d, ...}, final=())  # -> {slot: the (m,) outputs that became final with this chunk}
        counts = pool.push(chunks, final, out=rows, out_off={slot: column})
                                                             # the launch stores slot s's outputs at rows[s, column:]: -> {slot: m}
        views = pool.destinations({slot: n, ...})            # where the next chunk of n samples of each slot belongs: a caller that
        pieces = pool.push(views, final=(), placed=True)     # WRITES its chunks there itself (a converting launch) spares the copy

    A slot's concatenated pieces are torch.equal to resample(its whole signal, orig, new).  A slot whose rates are equal passes through
    untouched (its chunk is returned, or copied to `out`).  A slot in `final` is flushed with its true length and closed.

    State: one ResampleSchedule, one s0 and one tail per slot; rows of constant width, sized at construction from the declared pairs
    (the longest tail any of them carries, kw - 1 samples) and `max_push`; one arena with the banks of all declared pairs.  Per step:
    every named slot's chunk is copied behind its tail, ONE launch converts all named slots, every slot's new tail moves to the front
    of its row.  No host synchronisation; everything runs on the current stream."""

    def __init__(self, slots: int, pairs: Iterable[Tuple[int, int]], max_push: int):
        if int(slots) <= 0 or int(max_push) <= 0:
            raise ValueError("slots and max_push must be positive")
        self.S, self.max_push = int(slots), int(max_push)
        self.pairs: List[Tuple[int, int]] = []
        for o, n in pairs:
            o, n = int(o), int(n)
            if o <= 0 or n <= 0:
                raise ValueError("Original frequency and desired frequecy should be positive")
            if o != n and (o, n) not in self.pairs:
                self.pairs.append((o, n))
        if not self.pairs:
            raise ValueError("no rate pair to convert: equal rates need no resampler")
        scheds = [ResampleSchedule(o, n) for o, n in self.pairs]
        self.width = max(sc.kw for sc in scheds) - 1 + self.max_push        # samples per row: the longest tail and one chunk
        self.max_out = max(resample_max_outputs(o, n, self.max_push) for o, n in self.pairs)
        # the rate descriptors of the C entry: (bank_off, down, up, width) per declared pair, banks back to back in one arena
        self.rates: List[int] = []
        off = 0
        for sc in scheds:
            self.rates += [off, sc.down, sc.up, sc.width]
            off += sc.up * sc.kw
        self.arena_floats = off
        self.sched: List[Optional[ResampleSchedule]] = [None] * self.S
        self.rate = [0] * self.S                      # index into pairs; -1: equal rates, nothing to convert
        self.pair: List[Tuple[int, int]] = [(0, 0)] * self.S     # the rates the slot was opened with, by value
        self.s0 = [0] * self.S
        self.fill = [0] * self.S                      # valid samples in the slot's row
        self.buf = None

    def allocated_bytes(self) -> int:
        return 0 if self.buf is None else sum(t.numel() * t.element_size() for t in self.buf.values())

    def open(self, slot: int, orig_freq: int, new_freq: int) -> None:
        """slot starts a fresh stream at this pair (whatever it held before is forgotten)"""
        if not 0 <= slot < self.S:
            raise ValueError(f"slot {slot!r} out of range (0 .. {self.S - 1})")
        o, n = int(orig_freq), int(new_freq)
        if o != n and (o, n) not in self.pairs:
            raise ValueError(f"{o} -> {n} Hz was not declared at construction ({self.pairs})")
        self.sched[slot] = ResampleSchedule(o, n)
        self.rate[slot] = -1 if o == n else self.pairs.index((o, n))
        self.pair[slot] = (o, n)
        self.s0[slot] = self.fill[slot] = 0

    def close(self, slot: int) -> None:
        self.sched[slot] = None

    # -- a slot's state leaves and comes back (models/stream_sessions.py: snapshot / restore) ------------------------------------
    def slot_state(self, slot: int) -> dict:
        """what an open slot carries besides the samples of its tail -- buf["rows"][slot, :fill], ONE descriptor of a pack launch --
        as plain values: the rate PAIR by value (another pool may declare its pairs in another order), s0, the length of the tail
        and the schedule's counters"""
        if not 0 <= slot < self.S or self.sched[slot] is None:
            raise RuntimeError(f"slot {slot} is not open")
        return dict(pair=list(self.pair[slot]), s0=self.s0[slot], fill=self.fill[slot], sched=self.sched[slot].state())

    def check_state(self, state: Mapping) -> None:
        """ValueError when no slot of this pool can take the state: a pair that was not declared, a tail that does not fit a row"""
        o, n = (int(v) for v in state["pair"])
        if o != n and (o, n) not in self.pairs:
            raise ValueError(f"{o} -> {n} Hz was not declared at construction ({self.pairs})")
        sc = ResampleSchedule.from_state((o, n), state["sched"])
        if not 0 <= int(state["fill"]) <= self.width - self.max_push or (o != n and int(state["fill"]) >= sc.kw):
            raise ValueError(f"a resampler tail of {state['fill']} samples does not fit a row of this pool")

    def adopt(self, slot: int, state: Mapping) -> None:
        """slot continues the stream slot_state() was taken from; the samples of its tail belong at buf["rows"][slot, :fill]"""
        if not 0 <= slot < self.S:
            raise ValueError(f"slot {slot!r} out of range (0 .. {self.S - 1})")
        self.check_state(state)
        o, n = (int(v) for v in state["pair"])
        self.sched[slot] = ResampleSchedule.from_state((o, n), state["sched"])
        self.rate[slot] = -1 if o == n else self.pairs.index((o, n))
        self.pair[slot] = (o, n)
        self.s0[slot], self.fill[slot] = int(state["s0"]), int(state["fill"])

    def is_open(self, slot: int) -> bool:
        return self.sched[slot] is not None

    def allocate(self, dev) -> None:
        """the rows, the bank arena and the table scratch, once"""
        if self.buf is not None:
            return
        arena = torch.cat([filter_bank(o, n, dev)[0].reshape(-1) for o, n in self.pairs])
        assert arena.numel() == self.arena_floats
        self.buf = dict(rows=torch.zeros(self.S, self.width, dtype=torch.float32, device=dev), arena=arena.contiguous(),
                        table=torch.empty(7 * self.S + len(self.rates), dtype=torch.int64, device=dev))

    def destinations(self, counts: Mapping[int, int]) -> Dict[int, torch.Tensor]:
        """{slot: n} -> {slot: the (n,) fp32 view of the slot's row behind its carried tail}: where push() would copy a chunk of n
        samples.  A caller fills the views (one launch for all of them) and hands THEM to push(..., placed=True) in place of the
        chunks.  Nothing changes here; the views hold until that push.  Needs allocate(); a slot at equal rates has no row."""
        if self.buf is None:
            raise RuntimeError("destinations: allocate() first")
        out = {}
        for s, n in counts.items():
            if not 0 <= s < self.S or self.sched[s] is None:
                raise RuntimeError(f"slot {s} is not open")
            if self.rate[s] < 0:
                raise ValueError(f"slot {s}: equal rates, nothing is carried for it")
            if not 0 <= n <= self.max_push:
                raise ValueError(f"slot {s}: a push of {n} samples exceeds max_push = {self.max_push}")
            out[s] = self.buf["rows"][s, self.fill[s]:self.fill[s] + n]
        return out

    @torch.no_grad()
    def push(self, chunks: Mapping[int, torch.Tensor], final: Iterable[int] = (), out: Optional[torch.Tensor] = None,
             out_off: Optional[Mapping[int, int]] = None, placed: bool = False) -> Dict[int, object]:
        """placed: every chunk is the view destinations() handed out for it and already holds its samples -- the copy is skipped"""
        final = set(final)
        for s, x in chunks.items():
            if not 0 <= s < self.S or self.sched[s] is None:
                raise RuntimeError(f"slot {s} is not open")
            if x.ndim != 1:
                raise ValueError(f"slot {s}: expected (n,) samples, got {tuple(x.shape)}")
            if x.shape[0] > self.max_push:
                raise ValueError(f"slot {s}: a push of {x.shape[0]} samples exceeds max_push = {self.max_push}")
            _lib.require_cuda(x, "waveform")
            if placed and (self.buf is None or self.rate[s] < 0 or x.dtype != torch.float32 or
                           (x.shape[0] and x.data_ptr() != self.buf["rows"][s, self.fill[s]:].data_ptr())):
                raise ValueError(f"slot {s}: placed=True takes the views destinations() handed out")
        if final - set(chunks):
            raise ValueError(f"slots {sorted(final - set(chunks))} are in `final` but not among the pushed slots")
        if out is not None and (out.ndim != 2 or out.shape[0] != self.S or out.dtype != torch.float32 or out.stride(1) != 1):
            raise ValueError(f"out must be ({self.S}, w) fp32 with contiguous rows")
        if not chunks:
            return {}
        dev = next(iter(chunks.values())).device
        self.allocate(dev)
        rows = self.buf["rows"]
        S = self.S
        steps, res = {}, {}
        y_off = [0] * S
        for s, x in chunks.items():
            n = x.shape[0]
            st = self.sched[s].step(n, s in final)
            if self.rate[s] < 0:                                 # equal rates: untouched
                if out is not None:
                    at = int(out_off[s])
                    if n:
                        out[s, at:at + n] = x
                    res[s] = n
                else:
                    res[s] = x
                continue
            if n:
                if not placed:
                    rows[s, self.fill[s]:self.fill[s] + n] = x
                self.fill[s] += n
            steps[s] = st
            if out is not None:
                y_off[s] = int(out_off[s])
        if steps:
            rs0, nv, o0, n_out, total = resample_session_rows(S, steps, self.s0, self.fill)
            m = max(n_out)
            if out is None:
                y = torch.empty(S, max(m, 1), dtype=torch.float32, device=dev)      # the pieces handed out are views of it
            else:
                y = out
            if m:
                I64 = C.c_int64 * S
                with torch.cuda.device(dev):
                    _lib.check(_lib.lib().dmel_resample_window_items_f32(
                        rows.data_ptr(), self.width, self.width, I64(*rs0), I64(*nv), y.data_ptr(), y.stride(0), I64(*y_off),
                        self.buf["arena"].data_ptr(), self.arena_floats, (C.c_int64 * len(self.rates))(*self.rates), len(self.pairs),
                        I64(*[max(r, 0) for r in self.rate]), S, I64(*o0), I64(*n_out), I64(*total), self.buf["table"].data_ptr(),
                        _lib.stream_ptr()), "resample_window_items")
            for s, st in steps.items():
                res[s] = n_out[s] if out is not None else y[s, :n_out[s]]
                if st.final:
                    self.fill[s] = 0
                elif st.keep_from > self.s0[s]:
                    drop = st.keep_from - self.s0[s]
                    keep = self.fill[s] - drop
                    if keep:
                        row = rows[s]
                        row[:keep] = row[drop:drop + keep] if drop >= keep else row[drop:drop + keep].clone()
                    self.s0[s], self.fill[s] = st.keep_from, keep
        for s in final:
            self.sched[s] = None
        return res
