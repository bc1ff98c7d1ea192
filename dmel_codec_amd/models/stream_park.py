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
from typing import Dict, Iterable, List, Mapping, Optional, Sequence, Tuple

import torch

from .. import _lib

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
    """snapshot / drop / park / restore of a pool of sessions.  The pool says what a slot owns:

        _park_meta(slot)               the host state of an open slot as plain values (with "window")
        _park_shapes(meta)             [(name, rows, cols)]: the segments of the blob, a pure function of meta and the pool's widths
        _park_rows(slot)               {name: the slot's rows of that piece of device state, (rows, row width)}; a name that starts
                                       with one of _park_windowed is a window of columns of the state buffers (it moves with the
                                       slot's origin), the others are tails that start at column 0
        _park_check(meta)              ValueError when no slot of this pool can continue the session
        _park_adopt(slot, meta)        the slot continues the session (host state only)
        _park_zero(slot)               what a fresh slot zeroes before its first push
    """

    _pack_tab: Optional[torch.Tensor] = None
    _park_windowed: Tuple[str, ...] = ()
    _park_addr: Optional[dict] = None

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
        dev = self.buf["mel"].device if self.buf is not None else next(self.codec.parameters()).device
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
        dev = self.buf["mel"].device if self.buf is not None else None
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
        free = [s for s in range(self.S) if self.sched[s] is None]
        if len(free) < len(snaps):
            raise RuntimeError(f"{len(snaps)} snapshots to restore, {len(free)} of {self.S} slots are free")
        if dev is not None and self.buf is None:
            self._allocate(dev)
            if self.rs is not None:
                self.rs.allocate(dev)
        items, taken = [], []
        for s, sn in zip(free, snaps):
            meta = sn.meta
            self._park_adopt(s, meta)
            taken.append(s)
            if self.buf is None:                       # nothing was ever pushed, here or there: the first push zeroes the rows
                self._fresh[s] = True
                continue
            with torch.cuda.device(dev):
                self._park_zero(s)
            self._fresh[s] = False
            if sn.blob.numel():
                places, base = self._park_places(s), sn.blob.data_ptr()
                for name, rows, cols, off in meta["layout"]:
                    ptr, pitch, _ = places[name]                 # the window lands at column 0
                    items.append((base + 4 * off, ptr, rows, cols, cols, pitch))
        if items:
            pack_items(items, self._park_table(len(items), dev))
        return taken
