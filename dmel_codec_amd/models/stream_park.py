"""Live sessions that leave their slot and come back: SessionSnapshot, the one-launch ragged copy behind it (pack_items ->
dmel_stream_pack_items) and the methods EncodeSessions and DecodeSessions share (models/stream_sessions.py):

    snaps = pool.snapshot([a, b])            # {slot: SessionSnapshot}; ONE pack launch for all named slots; the sessions go on
    pool.drop(a)                             # the slot is free, nothing is flushed, no device call (a reply's abort)
    snaps = pool.park([a, b])                # snapshot, then drop each
    slots = other.restore(snaps.values())    # free slots of any pool of the same codec; ONE pack launch for all of them

Everything a session owns is bounded: a window of columns of its state rows -- exactly the columns a re-base in front of its next
push would keep (stream_schedule.encode_live_window / decode_live_window) --, a sample or token tail, a noise tail, a resampler tail, a
cross-fade tail, and host counters.  The blob of a snapshot holds those words back to back (no padding: its size is the size of the
state) and `meta` the counters and the layout; its size does not depend on the length of the stream.  NOT state and not shipped:
the shadow rows of early sessions (every step that uses them forks them again), the cross-fade weights (rebuilt from F), every
table scratch, and torch's RNG -- a decode session pushed without noise draws from the generator of the process it runs in, at the
time of the push.  EQUAL WEIGHTS ARE THE CALLER'S CONTRACT: a snapshot carries the geometry of its codec and is refused by a pool
whose geometry, widths or depth differ, but nothing can tell two checkpoints of one architecture apart.

A snapshot moves between devices with .to(device) / .cpu() and through torch.save as plain data:

    torch.save(snap.as_dict(), f);  snap = SessionSnapshot.from_dict(torch.load(f, weights_only=True))
"""
from __future__ import annotations

import copy
import ctypes as C
import dataclasses
from typing import Dict, Iterable, List, Mapping, Optional, Sequence, Tuple

import torch

from .. import _lib
from ..utils import pcm

VERSION = 1
PACK_TABLE_WORDS = 8                                   # int64 of table scratch per descriptor of dmel_stream_pack_items


class SessionSnapshot:
    """meta: a dict of plain Python values (format version, kind, geometry, widths, rates, wire format, counters, window, layout of
    the blob: [name, rows, cols, offset in words] per segment); blob: a 1-D int32 tensor, the segments back to back."""

    def __init__(self, meta: Mapping, blob: torch.Tensor):
        if blob.ndim != 1 or blob.dtype != torch.int32:
            raise ValueError(f"the blob of a snapshot is a 1-D int32 tensor, got {tuple(blob.shape)} {blob.dtype}")
        self.meta, self.blob = dict(meta), blob.contiguous()

    @property
    def nbytes(self) -> int:
        return self.blob.numel() * self.blob.element_size()

    def to(self, device) -> "SessionSnapshot":
        return SessionSnapshot(copy.deepcopy(self.meta), self.blob.to(device))

    def cpu(self) -> "SessionSnapshot":
        return self.to("cpu")

    def as_dict(self) -> dict:
        """{"meta", "blob"}: plain data for torch.save; the blob detached from the launch's common blob, so that only its own words
        are written"""
        return dict(meta=copy.deepcopy(self.meta), blob=self.blob.clone())

    @classmethod
    def from_dict(cls, d: Mapping) -> "SessionSnapshot":
        return cls(d["meta"], d["blob"])


def pack_items(items: Sequence[Tuple[int, int, int, int, int, int]], table: torch.Tensor) -> None:
    """items of (src address, dst address, rows, cols, src pitch, dst pitch), pitches and cols in 4-byte words, all of them in ONE
    launch (dmel_stream_pack_items) on the current stream of table's device.  table: int64 device scratch of 8 * len(items)."""
    R = len(items)
    if R == 0:
        raise ValueError("no item to copy")
    if table.dtype != torch.int64 or table.numel() < PACK_TABLE_WORDS * R or not table.is_contiguous():
        raise ValueError(f"table must hold {PACK_TABLE_WORDS * R} contiguous int64")
    _lib.require_cuda(table, "table")
    P, I64 = C.c_void_p * R, C.c_int64 * R
    cols = list(zip(*items))
    with torch.cuda.device(table.device):
        _lib.check(_lib.lib().dmel_stream_pack_items(P(*[p or None for p in cols[0]]), P(*[p or None for p in cols[1]]), I64(*cols[2]),
                                                     I64(*cols[3]), I64(*cols[4]), I64(*cols[5]), R, table.data_ptr(), _lib.stream_ptr()),
                   "stream_pack_items")


def plain(v):
    """tuples of a dataclass's dict as lists, so that a meta compares equal after a trip through a file"""
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    return v


def dense_layout(shapes: Sequence[Tuple[str, int, int]]) -> Tuple[List[list], int]:
    """(name, rows, cols) of every segment -> ([name, rows, cols, offset] of the live ones, back to back, total words)"""
    layout, off = [], 0
    for name, rows, cols in shapes:
        if rows * cols:
            layout.append([name, rows, cols, off])
            off += rows * cols
    return layout, off


def _view2d(t: torch.Tensor) -> torch.Tensor:
    """(..., cols) with contiguous columns and evenly pitched rows -> (rows, cols)"""
    v = t.reshape(-1, t.shape[-1]) if t.ndim != 2 else t
    if v.numel() and (v.stride(1) != 1 or v.data_ptr() != t.data_ptr()):
        raise RuntimeError("a state segment is not a window of evenly pitched rows")
    return v


class ParkingPool:
    """What a pool of session slots is, once for EncodeSessions and DecodeSessions: which slots are open, the wire options of each
    session (rate, sample format, channels), buffers from the first use on, a slot's rows made ready for its session, and
    snapshot / drop / park / restore.  The pool says what a slot owns:

        _resamples_in                  the slot's resampler entry runs (session rate -> own rate); else (own rate -> session rate)
        _allocate(dev), _slot_views(s) the state buffers; the slot's rows of them, zeroed before its session's first step
        _park_meta(slot)               the host state of an open slot as plain values (with "window"): the shared keys, its own on top
        _park_schedule(meta)           the schedule of that state, rebuilt; _live_window(schedule): its live window
        _park_shapes(meta)             [(name, rows, cols)]: the segments of the blob, a pure function of meta and the pool's widths
        _park_rows(slot)               {name: the slot's rows of that piece of device state, (rows, row width)}; a name that starts
                                       with one of _park_windowed is a window of columns of the state buffers (it moves with the
                                       slot's origin), the others are tails that start at column 0
        _park_widths()                 ((key, the pool's value), ...): the widths besides G, C, L, in the meta and equal to restore
        _park_fits(meta, schedule)     ValueError where the pool's own keys and sizes cannot continue the session
        _park_adopt(slot, meta)        the slot continues the session (host state only): the shared lists, its own on top
    """

    _pack_tab: Optional[torch.Tensor] = None
    _park_windowed: Tuple[str, ...] = ()
    _park_addr: Optional[dict] = None
    _has_audio = True                                  # a pool that returns no audio (DecodeSessions(return_audios=False)) has no wire

    def _init_slots(self, own_rate: Optional[int], rates_option: str, rs_push: int) -> None:
        """the per-slot lists both pools keep and the slots' resamplers; own_rate: the codec's (encode) or the vocoder's (decode) rate"""
        S = self.S
        self.own_rate, self._rates_option, self.rs = own_rate, rates_option, None
        if getattr(self, rates_option):
            from ..utils.resample import SessionResampler
            self.rs = SessionResampler(S, [self._rate_pair(r) for r in getattr(self, rates_option)], rs_push)
        self.sched: List[Optional[object]] = [None] * S
        self.origin = [0] * S                          # the absolute frame in column 0 of the slot's rows
        self.rate = [own_rate] * S                     # the rate the slot's pushes arrive at (encode) / its audio leaves at (decode)
        self.fmt = ["f32"] * S                         # the sample format of that wire (utils/pcm.py: FORMATS)
        self.ch = [1] * S                              # its channels (interleaved frames when above 1)
        self._fresh = [False] * S                      # opened, rows not prepared yet (done with the slot's first push)
        self.buf = None

    # -- bookkeeping (no device call) ------------------------------------------------------------------------------------
    @property
    def capacity(self) -> int:
        """columns of the state buffers (frames); fixed at construction"""
        return self.cap

    @property
    def open_slots(self) -> List[int]:
        return [s for s in range(self.S) if self.sched[s] is not None]

    def allocated_bytes(self) -> int:
        own = 0 if self.buf is None else sum(t.numel() * t.element_size() for t in self.buf.values())
        return own + (self.rs.allocated_bytes() if self.rs is not None else 0)

    def _check_open(self, slot) -> None:
        if not isinstance(slot, int) or not 0 <= slot < self.S:
            raise ValueError(f"slot {slot!r} out of range (0 .. {self.S - 1})")
        if self.sched[slot] is None:
            raise RuntimeError(f"slot {slot} is not open")

    def _free_slots(self) -> List[int]:
        return [s for s in range(self.S) if self.sched[s] is None]

    def _first_free(self) -> int:
        free = self._free_slots()
        if not free:
            raise RuntimeError(f"all {self.S} slots are taken")
        return free[0]

    def _check_wire(self, rate, sample_format, channels, channel=None) -> int:
        """the wire options of one session, refused here for open() and for restore() alike -> the pick of `channel`"""
        if pcm.check_format(sample_format) != "f32" and not self._has_audio:
            raise ValueError(f"sample_format={sample_format!r} without audio: return_audios=False leaves nothing to convert")
        if pcm._check_channels(channels) > 1 and not self._has_audio:
            raise ValueError(f"channels={channels} without audio: return_audios=False leaves nothing to fan out")
        pick = pcm.check_channel(channel, channels)
        declared = getattr(self, self._rates_option)
        if rate != self.own_rate and rate not in declared:
            raise ValueError(f"a session at {rate} Hz: the pool was built for {(self.own_rate,) + declared} Hz "
                             f"(declare the rate in {self._rates_option}=)")
        return pick

    def _rate_pair(self, rate) -> Tuple[int, int]:
        return (rate, self.own_rate) if self._resamples_in else (self.own_rate, rate)

    def _occupy(self, s: int, sched, origin: int, rate, sample_format: str, channels: int, resampler: Optional[Mapping] = None) -> None:
        """slot s is this session's, its rows to be prepared; its resampler entry is opened, or adopted from a parked one's state"""
        self.sched[s], self.origin[s], self._fresh[s] = sched, origin, True
        self.rate[s], self.fmt[s], self.ch[s] = rate, sample_format, channels
        if self.rs is not None and resampler is not None:
            self.rs.adopt(s, resampler)
        elif self.rs is not None:
            self.rs.open(s, *self._rate_pair(rate))

    def _converts(self, slot: int) -> bool:             # the session runs at another rate than the pool's own: its resampler has work
        return self.rate[slot] != self.own_rate

    def _wired(self, slot: int) -> bool:                # the wire is not mono f32: the slot takes part in the step's convert launch
        return self.fmt[slot] != "f32" or self.ch[slot] > 1

    def _release(self, slots: Iterable[int]) -> None:
        for s in slots:
            self.sched[s] = None          # the slot is free; its rows are zeroed when it is opened and pushed to again

    # -- buffers -----------------------------------------------------------------------------------------------------------
    def _device(self):
        return next(iter(self.buf.values())).device if self.buf is not None else next(self.codec.parameters()).device

    def _ensure_buffers(self, dev) -> None:
        if self.buf is None:
            self._allocate(dev)
            if self.rs is not None:
                self.rs.allocate(dev)

    def _prepare_slot(self, s: int) -> None:
        """the slot's rows as its session's first step, or the scatter of a restore, must find them: zeroed"""
        for v in self._slot_views(s):
            v.zero_()
        self._fresh[s] = False

    # -- a session leaves its slot and comes back ------------------------------------------------------------------------
    def _park_meta(self, s: int) -> dict:
        sch = self.sched[s]
        return dict(version=VERSION, kind=self._park_kind, geometry=plain(dataclasses.asdict(self.geo)), G=self.G, C=self.C, L=self.L,
                    rate=self.rate[s], sample_format=self.fmt[s], channels=self.ch[s], channel=None, lookahead=None, fade=0,
                    has_tail=False, schedule=sch.state(), window=list(self._live_window(sch)), **dict(self._park_widths()),
                    resampler=self.rs.slot_state(s) if self.rs is not None and self._converts(s) else None)

    def _park_check(self, meta: Mapping) -> None:
        """ValueError when no slot of this pool can continue the session"""
        if plain(meta["geometry"]) != plain(dataclasses.asdict(self.geo)):
            raise ValueError(f"a session of geometry {meta['geometry']} into a pool of geometry {dataclasses.asdict(self.geo)}")
        for key, mine in (("G", self.G), ("C", self.C), ("L", self.L)) + self._park_widths():
            if meta[key] != mine:
                raise ValueError(f"a session with {key} = {meta[key]} into a pool with {key} = {mine}")
        sc = self._park_schedule(meta)
        self._park_fits(meta, sc)
        self._check_wire(meta["rate"], meta["sample_format"], meta["channels"], meta["channel"])
        if list(self._live_window(sc)) != list(meta["window"]):
            raise ValueError(f"window {meta['window']} is not the live window {self._live_window(sc)} of the session's schedule")
        if sc.finished:
            raise ValueError("the session has finished")
        rs = meta["resampler"]
        if (rs is not None) != (meta["rate"] != self.own_rate):
            raise ValueError(f"a resampler state goes with a session at another rate than the {self._own_rate_of}, and only with it")
        if rs is not None:
            if list(rs["pair"]) != list(self._rate_pair(meta["rate"])):
                raise ValueError(f"a resampler state for {rs['pair']} Hz in a session at {meta['rate']} Hz")
            self.rs.check_state(rs)

    def _park_adopt(self, s: int, meta: Mapping) -> None:
        self._occupy(s, self._park_schedule(meta), meta["window"][0], meta["rate"], meta["sample_format"], meta["channels"],
                     meta["resampler"])

    def _park_places(self, s: int) -> Dict[str, Tuple[int, int, bool]]:
        """{name: (address of column 0 of the slot's rows, pitch in words, windowed)}: plain integers, kept per slot, so that a
        snapshot or restore of many slots builds its descriptors without a tensor operation.  The addresses hold while every state
        tensor is where it was: the cache is keyed on the base address of each of them (the pools allocate them once, but a
        buffer that is ever regrown must not be packed from where it used to be)."""
        key = tuple(t.data_ptr() for t in self.buf.values())
        if self.rs is not None and self.rs.buf is not None:
            key += (self.rs.buf["rows"].data_ptr(),)
        if self._park_addr is None or self._park_addr["of"] != key:
            self._park_addr = {"of": key}
        if s not in self._park_addr:
            places = {}
            for name, t in self._park_rows(s).items():
                v = _view2d(t)
                places[name] = (v.data_ptr(), v.stride(0), name.startswith(self._park_windowed))
            self._park_addr[s] = places
        return self._park_addr[s]

    def _park_table(self, R: int, dev) -> torch.Tensor:
        t = self._pack_tab
        if t is None or t.numel() < PACK_TABLE_WORDS * R or t.device != dev:
            self._pack_tab = t = torch.empty(PACK_TABLE_WORDS * max(R, 32), dtype=torch.int64, device=dev)
        return t

    def _park_slots(self, slots) -> List[int]:
        slots = list(slots)
        for s in slots:
            self._check_open(s)
        if len(set(slots)) != len(slots):
            raise ValueError(f"a slot is named twice: {slots}")
        return slots

    @torch.no_grad()
    def snapshot(self, slots: Iterable[int]) -> Dict[int, SessionSnapshot]:
        """{slot: SessionSnapshot} of the named open slots: ONE dmel_stream_pack_items launch gathers the state of all of them into
        one blob the snapshots are views of.  The sessions stay open and untouched.  A closed or out-of-range slot is refused as
        by push, before anything is launched."""
        slots = self._park_slots(slots)
        metas, items, spans, total = {}, [], {}, 0
        for s in slots:
            meta = self._park_meta(s)
            layout, words = dense_layout(self._park_shapes(meta))
            meta["layout"] = layout
            metas[s], spans[s] = meta, (total, words)
            if words:
                places, col0 = self._park_places(s), meta["window"][0] - self.origin[s]
                for name, rows, cols, off in layout:
                    ptr, pitch, windowed = places[name]
                    items.append((ptr + 4 * col0 if windowed else ptr, 4 * (total + off), rows, cols, pitch, cols))
            total += words
        dev = self._device()
        blob = torch.empty(total, dtype=torch.int32, device=dev)
        if items:
            base = blob.data_ptr()
            pack_items([(src, base + off, r, c, sp, dp) for src, off, r, c, sp, dp in items], self._park_table(len(items), dev))
        return {s: SessionSnapshot(metas[s], blob[spans[s][0]:spans[s][0] + spans[s][1]]) for s in slots}

    def drop(self, slot: int) -> None:
        """free an open slot without flushing it: no device call, its resampler entry is closed.  What the session had not handed
        out is gone -- a reply's abort, or the second half of park()."""
        self._check_open(slot)
        self.sched[slot] = None
        if self.rs is not None:
            self.rs.close(slot)

    def park(self, slots: Iterable[int]) -> Dict[int, SessionSnapshot]:
        """snapshot(slots), then drop() of each"""
        snaps = self.snapshot(slots)
        for s in snaps:
            self.drop(s)
        return snaps

    @torch.no_grad()
    def restore(self, snapshots) -> List[int]:
        """continue the sessions of `snapshots` (SessionSnapshots, or the dict snapshot() returns) in free slots of this pool -> their
        slots, in order.  ONE dmel_stream_pack_items launch scatters all of them (the rows of each slot are zeroed first, as a
        fresh slot's are); each session's window lands at column 0 of its rows, whose origin becomes the window's first frame, so
        a pool with another capacity, slot count or maximal push is a valid target.  ValueError, no slot taken, nothing launched:
        a snapshot this pool cannot continue (see the class).  RuntimeError, no slot taken: fewer free slots than snapshots."""
        snaps = list(snapshots.values()) if isinstance(snapshots, Mapping) else list(snapshots)
        dev = self._device() if self.buf is not None else None
        for sn in snaps:
            if not isinstance(sn, SessionSnapshot):
                raise ValueError(f"restore takes SessionSnapshots, got {type(sn).__name__}")
            meta = sn.meta
            if meta.get("version") != VERSION:
                raise ValueError(f"a snapshot of format version {meta.get('version')!r}: this pool reads version {VERSION}")
            if meta.get("kind") != self._park_kind:
                raise ValueError(f"a snapshot of kind {meta.get('kind')!r} into a pool of {self._park_kind} sessions")
            self._park_check(meta)
            layout, words = dense_layout(self._park_shapes(meta))
            if plain(meta.get("layout")) != layout or sn.blob.numel() != words:
                raise ValueError(f"the layout of the snapshot ({meta.get('layout')}, {sn.blob.numel()} words) is not the layout of its "
                                 f"state ({layout}, {words} words)")
            if words:
                if not sn.blob.is_cuda:
                    raise ValueError(f"the blob of a snapshot to restore must live on the GPU (got {sn.blob.device}): .to(device) first")
                if dev is not None and sn.blob.device != dev:
                    raise ValueError(f"a blob on {sn.blob.device} into a pool whose buffers are on {dev}")
                dev = sn.blob.device
        free = self._free_slots()
        if len(free) < len(snaps):
            raise RuntimeError(f"{len(snaps)} snapshots to restore, {len(free)} of {self.S} slots are free")
        if dev is not None:
            self._ensure_buffers(dev)
        items, taken = [], free[:len(snaps)]
        for s, sn in zip(taken, snaps):
            self._park_adopt(s, sn.meta)
            if self.buf is None:                       # nothing was ever pushed, here or there: the first push zeroes the rows
                continue
            with torch.cuda.device(dev):
                self._prepare_slot(s)
            if sn.blob.numel():
                places, base = self._park_places(s), sn.blob.data_ptr()
                for name, rows, cols, off in sn.meta["layout"]:
                    ptr, pitch, _ = places[name]                 # the window lands at column 0
                    items.append((base + 4 * off, ptr, rows, cols, cols, pitch))
        if items:
            pack_items(items, self._park_table(len(items), dev))
        return taken
