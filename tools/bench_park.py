"""What `tools/bench_stream.py --sessions S --park` and `tools/bench_stream_encode.py --sessions S --park` share: snapshot + restore of
all S sessions of a pool in steady state (ONE dmel_stream_pack_items launch per direction) against the way a server could do it
without the entry -- one torch slice .clone() per state tensor per slot and a torch.cat into the slot's blob, and per slot the inverse,
one slice copy per tensor.  Both move the same words, zero the same rows, do the same host bookkeeping, are interleaved in one
process, and each cycle is bracketed by host synchronisations and timed on the wall clock.  The baseline is written against the
pools' private hooks (_park_meta, _park_shapes, _park_rows, _park_adopt, _prepare_slot) on purpose: it has to slice the very windows
the launch packs and to do the very bookkeeping restore() does, or the two columns of the table would not measure the same work."""
import statistics
import time

import torch

from dmel_codec_amd.models.stream_park import dense_layout


def slot_views(pool, s, meta, col0):
    """{name: the (rows, cols) tensor view of every live segment of the slot's state}, the windows from column col0 on"""
    rows_of, out = pool._park_rows(s), {}
    for name, rows, cols, _ in meta["layout"]:
        t = rows_of[name]
        c0 = col0 if name.startswith(pool._park_windowed) else 0
        out[name] = t.reshape(-1, t.shape[-1])[:rows, c0:c0 + cols]
    return out


def slice_snapshot(pool, slots):
    """{slot: (meta, blob)}: the pool's own windows (the same ones snapshot() packs), one clone per tensor, one cat per slot"""
    out = {}
    for s in slots:
        meta = pool._park_meta(s)
        meta["layout"], _ = dense_layout(pool._park_shapes(meta))
        views = slot_views(pool, s, meta, meta["window"][0] - pool.origin[s])
        parts = [views[name].clone().view(torch.int32).reshape(-1) for name, _, _, _ in meta["layout"]]
        out[s] = (meta, torch.cat(parts) if parts else torch.empty(0, dtype=torch.int32, device=pool._device()))
    return out


def slice_restore(pool, slot, meta, blob):
    """the inverse: the slot's rows zeroed as restore() zeroes them, one slice copy per tensor, the window at column 0"""
    pool._park_adopt(slot, meta)
    pool._prepare_slot(slot)
    views = slot_views(pool, slot, meta, 0)
    for name, rows, cols, off in meta["layout"]:
        v = views[name]
        v.copy_(blob[off:off + rows * cols].view(v.dtype).view(v.shape))


def measure(pool, slots, reps=40, warmup=6):
    """-> (result dict, table rows, the slots the sessions live in afterwards)"""
    ms = {"one_launch": [], "torch_slices": []}
    payload = tensors = 0
    for i in range(reps + warmup):
        for k in (("one_launch", "torch_slices") if i % 2 == 0 else ("torch_slices", "one_launch")):        # neither always goes first
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if k == "one_launch":
                snaps = pool.park(slots)
                slots = pool.restore(snaps)
            else:
                saved = slice_snapshot(pool, slots)
                for s in slots:
                    pool.drop(s)
                for s, (meta, blob) in saved.items():
                    slice_restore(pool, s, meta, blob)
            torch.cuda.synchronize()
            if i >= warmup:
                ms[k].append((time.perf_counter() - t0) * 1e6)
            if k == "one_launch":
                payload = sum(sn.nbytes for sn in snaps.values())
                tensors = sum(len(sn.meta["layout"]) for sn in snaps.values())
            else:                                                            # both carry the same words
                words = torch.cat([b for _, b in saved.values()])
                assert torch.equal(words, torch.cat([sn.blob for sn in pool.snapshot(slots).values()])), "the two ways disagree"
    pct = lambda v, q: sorted(v)[min(len(v) - 1, int(q * len(v)))]
    moved = 4 * payload                                                      # read and written once per direction
    result = {"sessions": len(slots), "cycles": reps, "snapshot_bytes": payload, "bytes_moved": moved, "state_tensors": tensors}
    rows = []
    for k, v in ms.items():
        med = statistics.median(v)
        result[k] = {"median_us": round(med, 1), "p10_us": round(pct(v, 0.1), 1), "p90_us": round(pct(v, 0.9), 1), "n": len(v),
                     "gb_per_s": round(moved / med * 1e-3, 2)}
        rows.append(f"{len(slots):8d}  {k:12s}  {med:10.1f}  {pct(v, 0.1):10.1f}  {pct(v, 0.9):10.1f}  {len(v):4d}  {moved:11d}  {moved / med * 1e-3:8.2f}")
    result["torch_slices_over_one_launch"] = round(result["torch_slices"]["median_us"] / result["one_launch"]["median_us"], 2)
    rows.append(f"{tensors} state tensors in all ({tensors // max(len(slots), 1)} per session), {payload} bytes of snapshots; "
                f"torch slices / one launch: {result['torch_slices_over_one_launch']:.2f}x at the median")
    return result, rows, slots
