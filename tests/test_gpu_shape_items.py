"""dmel_shape_items on the GPU (csrc/small_ops.hip) against the host rule (dmel_codec_amd/utils/shape.py: scan), bit for bit: the
samples handed out, the whole state rows and the per-block outputs.  Every destination lies in an arena of guard words, every state
row and every block row ends in guard words, and the wholes are compared -- the rule's bits where it writes, the guards everywhere
else."""
import numpy as np
import pytest
import torch

from dmel_codec_amd import _lib
from dmel_codec_amd.utils import shape

pytestmark = pytest.mark.gpu

GUARD = 0x7fc0dead
RATE = 24000


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def signal(n, seed, scale=0.6):
    """noise with a loud burst and a quiet stretch: the limiter attacks, holds and releases"""
    g = np.random.default_rng(seed)
    x = (g.standard_normal(n) * scale).astype(np.float32)
    x[n // 3:n // 3 + max(1, n // 7)] *= np.float32(3.0)
    x[n // 2:n // 2 + n // 5] *= np.float32(0.05)
    return x


def spec(cfg, cuts, seed=0, requests=(), final=True, end=None, so=0, do=0):
    """a slot: step k of the sequence takes cuts[k] samples (None: the slot is idle in that step); final: its last step that is
    not idle is the session's last; so, do: offsets of source and destination in floats off a 16-byte boundary"""
    return dict(cfg=cfg, cuts=list(cuts), z=signal(sum(c or 0 for c in cuts) + 3, seed), requests=list(requests), final=final, end=end,
                so=so, do=do)


def run(specs, dev, pitch_extra=5):
    """the launches of the sequence, each compared with scan() -> the number of launches"""
    S, steps = len(specs), max(len(sp["cuts"]) for sp in specs)
    words = [sp["cfg"].state_words(RATE) for sp in specs]
    pitch = max(words) + pitch_extra
    host_rows = np.full((S, pitch), GUARD, dtype=np.int64).astype(np.int32)
    for s, w in enumerate(words):
        host_rows[s, :w] = 0
    state = torch.from_numpy(host_rows.copy()).to(dev)
    at = [0] * S
    host_state = [None] * S
    for k in range(steps):
        src, dst, cfgs, segs, base, pos, hold, fin, expect = [], [], [], [], [], [], [], [], []
        bmax = 0
        for s, sp in enumerate(specs):
            n = sp["cuts"][k] if k < len(sp["cuts"]) else None
            cfg, N = sp["cfg"], sp["cfg"].block(RATE)
            last = sp["final"] and all(c is None for c in sp["cuts"][k + 1:])
            if n is None:
                src.append(None), dst.append(None), cfgs.append(None), segs.append([]), base.append(0.0), pos.append(0), hold.append(0)
                fin.append(False), expect.append(None)
                continue
            st = host_state[s]
            p, h = (0, 0) if st is None else (int(st[shape.I_IN]), int(st[shape.I_HOLD]))
            if sp["end"] is not None and p + n >= sp["end"]:           # what the pool does with an end: cut, and the step is the last
                n, last = sp["end"] - p, True
            z = sp["z"][at[s]:at[s] + n]
            y, st2, pk, gn = shape.scan(z, sp["requests"], cfg, RATE, state=st, final=last)
            assert y.shape[0] == shape.emitted(h, n, N, last, cfg.limit) and pk.shape[0] == shape.completed(h, n, N, last, cfg.limit)
            lv, b = shape.live(shape.plan(sp["requests"], cfg), cfg.initial_gain, p)
            xs = torch.zeros(n + 8, dtype=torch.float32, device=dev)
            assert xs.data_ptr() % 16 == 0
            xs[sp["so"]:sp["so"] + n] = torch.from_numpy(z)
            src.append(xs[sp["so"]:sp["so"] + n] if n else None)
            arena = torch.full((y.shape[0] + 24,), GUARD, dtype=torch.int32, device=dev)
            a = 8 + sp["do"]
            dst.append(arena.view(torch.float32)[a:a + y.shape[0]])
            want = np.full(arena.shape[0], GUARD, dtype=np.int64).astype(np.int32)
            want[a:a + y.shape[0]] = y.numpy().view(np.int32)
            cfgs.append(cfg), segs.append(lv), base.append(b), pos.append(p), hold.append(h), fin.append(last)
            expect.append((arena, want, st2, pk, gn))
            at[s] += n
            host_state[s] = st2
            host_rows[s, :words[s]] = st2.numpy()
            bmax = max(bmax, pk.shape[0])
        opk = torch.full((S, bmax + 3), GUARD, dtype=torch.int32, device=dev)
        ogn = torch.full((S, bmax + 3), GUARD, dtype=torch.int32, device=dev)
        out = shape.shape_items(src, dst, cfgs, segs, base, pos, hold, fin, state, opk.view(torch.float32), ogn.view(torch.float32), RATE)
        torch.cuda.synchronize()
        rows = state.cpu().numpy()
        for s, e in enumerate(expect):
            assert np.array_equal(rows[s], host_rows[s]), (k, s, np.nonzero(rows[s] != host_rows[s])[0][:8])
            got_pk, got_gn = opk[s].cpu().numpy(), ogn[s].cpu().numpy()
            if e is None:
                assert out[s] == 0 and (got_pk == np.int32(GUARD)).all() and (got_gn == np.int32(GUARD)).all()
                continue
            arena, want, _, pk, gn = e
            got = arena.cpu().numpy()
            assert out[s] == want.shape[0] - 24
            assert np.array_equal(got, want), (k, s, np.nonzero(got != want)[0][:8], want.shape)
            B = pk.shape[0]
            assert np.array_equal(got_pk[:B], pk.numpy().view(np.int32)) and (got_pk[B:] == np.int32(GUARD)).all(), (k, s)
            assert np.array_equal(got_gn[:B], gn.numpy().view(np.int32)) and (got_gn[B:] == np.int32(GUARD)).all(), (k, s)
    return steps


LOUD = [(0, 2.5, 0)]                                                           # +8 dB from the first sample: the limiter works


@pytest.mark.parametrize("N", [32, 120, 1024])
def test_counts_fresh_continued_and_flushed(dev, N):
    """every count of the issue, fresh, continued as one stream and flushed by a last step without samples"""
    cfg = shape.ShapeConfig(block_samples=N)
    second = (min(63, 4096 // N) + 1) * N + 7                                   # does not fit the tile of one pass
    counts = [None, 1, N - 1, N, N + 1, 2 * N, 3 * N + 5, second]
    specs = [spec(cfg, [c, counts[(i + 3) % len(counts)], 0 if c is not None else None], seed=10 * N + i, requests=LOUD, so=i % 4,
                  do=(i + 1) % 4) for i, c in enumerate(counts)]
    specs[0]["cuts"] = [None, None, None]                                       # a row that stays idle throughout: sentinels untouched
    run(specs, dev)


def test_every_alignment_of_source_and_destination(dev):
    cfg = shape.ShapeConfig(block_samples=32)
    run([spec(cfg, [3 * 32 + 5, 70, 0], seed=a, requests=LOUD, so=a % 4, do=a // 4) for a in range(16)], dev)
    off = shape.ShapeConfig(block_samples=32, limit=False)
    run([spec(off, [3 * 32 + 5, 4099], seed=a, requests=LOUD, so=a % 4, do=a // 4) for a in range(16)], dev)


def test_limit_on_and_off_two_blocks_and_idle_rows_in_one_launch(dev):
    a, b, c = shape.ShapeConfig(block_samples=48), shape.ShapeConfig(block_samples=1024), shape.ShapeConfig(limit=False)
    run([spec(a, [100, None, 50, 0], 1, LOUD), spec(a, [None] * 4, 2), spec(b, [3000, 5000, None, 0], 3, LOUD, so=1),
         spec(c, [777, 1, None, 33], 4, LOUD, do=3), spec(b, [None] * 4, 5), spec(c, [None, 5000, 1, None], 6, [(100, 3.0, 50)]),
         spec(a, [47, 1, 48, 0], 7, [(0, 4.0, 10)], so=2, do=2)], dev)


def test_segments(dev):
    cfg, N = shape.ShapeConfig(block_samples=64), 64
    across = [(90, 0.25, 200)]                                                  # begins in launch 0, ends in launch 2
    cut_short = [(10, 3.0, 400), (150, 0.5, 64), (151, 1.5, 0)]                 # a ramp interrupted twice
    eight = [(5 + 40 * k, 0.5 + 0.25 * k, 300) for k in range(8)]               # all eight unfinished in launch 1
    longest = [(0, 0.0, 0), (3, 4.0, 16384)]
    mute = [(0, 2.0, 0), (120, 0.0, 32), (400, 1.0, 32)]
    n = [100, 130, 260, 0]
    run([spec(cfg, n, 1, across), spec(cfg, n, 2, cut_short, so=1), spec(cfg, [2, 400, 88, 0], 3, eight, do=1),
         spec(cfg, [9000, 9000, 0], 4, longest, so=3), spec(cfg, n, 5, mute), spec(shape.ShapeConfig(limit=False), n, 6, mute, do=2)], dev)
    segs, base = shape.live(shape.plan(eight, cfg), 1.0, 2)
    assert len(segs) == 8 and shape.live(shape.plan(eight, cfg), 1.0, 2000)[0] == []


def test_a_stop_whose_end_falls_inside_a_block(dev):
    cfg, N = shape.ShapeConfig(block_samples=120), 120
    stop = [(0, 2.0, 0), (300, 0.0, 130)]                                       # E = 430 = 3 N + 70
    run([spec(cfg, [250, 100, 200], 1, stop, end=430), spec(cfg, [430 + 50], 2, stop, end=430, so=1, do=3),
         spec(cfg, [300, 0, 130], 3, stop, end=430), spec(shape.ShapeConfig(limit=False), [250, 500], 4, stop, end=430)], dev)


def test_one_record_per_launch_and_none_when_every_slot_is_idle(dev):
    cfg = shape.ShapeConfig(block_samples=32)
    state = torch.full((2, cfg.state_words(RATE)), GUARD, dtype=torch.int32, device=dev)
    pk = torch.full((2, 4), GUARD, dtype=torch.int32, device=dev)
    args = ([None, None], [None, None], [None, None], [[], []], [1.0, 1.0], [0, 0], [0, 0], [False, False], state,
            pk.view(torch.float32), pk.clone().view(torch.float32), RATE)
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        assert shape.shape_items(*args) == [0, 0]
        torch.cuda.synchronize()
        assert _lib.prof_read("shape")["launches"] == 0
        assert (state.cpu() == GUARD).all() and (pk.cpu() == GUARD).all()
        run([spec(cfg, [100], 1, LOUD), spec(cfg, [None], 2)], dev)
        assert _lib.prof_read("shape")["launches"] == 1
    finally:
        _lib.prof_enable(False)
        _lib.prof_reset()
