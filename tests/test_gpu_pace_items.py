"""dmel_pace_items on the GPU (csrc/small_ops.hip) against the host rule (dmel_codec_amd/utils/pace.py: scan), bit for bit: the
samples handed out, the whole state rows and the per-frame offsets and scores.  Every destination lies in an arena of guard words,
every state row and every frame row ends in guard words, and the wholes are compared -- the rule's bits where it writes, the guards
everywhere else."""
import ctypes as C

import numpy as np
import pytest
import torch

from dmel_codec_amd import _lib
from dmel_codec_amd.utils import pace

pytestmark = pytest.mark.gpu

GUARD = 0x7fc0dead
RATE = 1000                                             # at 1000 Hz a millisecond is a sample: hop_ms = H and search_ms = D
SIZES = [(64, 0), (64, 8), (64, 64), (256, 160), (512, 512)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def config(H, D, **kw):
    cfg = pace.PaceConfig(hop_ms=float(H), search_ms=float(D), **kw)
    assert cfg.samples(RATE) == (H, D)
    return cfg


def signal(n, seed, H=64):
    """a voiced-like sum of three harmonics with noise, a quiet stretch (zeros) and a very quiet one (below the floor)"""
    g = np.random.default_rng(seed)
    t = np.arange(n)
    period = 0.37 * H + seed % 5
    x = 0.3 * np.sin(2 * np.pi * t / period) + 0.15 * np.sin(4 * np.pi * t / period + 1.0) + 0.1 * np.sin(6 * np.pi * t / period + 2.0)
    x = (x + 0.02 * g.standard_normal(n)).astype(np.float32)
    x[n // 3:n // 3 + 3 * H] = 0.0
    x[n // 2:n // 2 + 3 * H] *= np.float32(1e-6)
    return x


def spec(cfg, cuts, seed=0, requests=(), final=True, so=0, do=0, x=None):
    """a slot: step k of the sequence takes cuts[k] samples (None: the slot is idle in that step); final: its last step that is
    not idle is the stream's last; so, do: offsets of source and destination in floats off a 16-byte boundary"""
    n = sum(c or 0 for c in cuts)
    return dict(cfg=cfg, cuts=list(cuts), x=signal(n + 3, seed, cfg.samples(RATE)[0]) if x is None else x, requests=list(requests),
                final=final, so=so, do=do)


def run(specs, dev, pitch_extra=5, whole=True):
    """the launches of the sequence, each compared with scan(); with `whole`, the samples of all launches of a slot also against
    ONE scan of its stream -> the searched frames seen"""
    S, steps = len(specs), max(len(sp["cuts"]) for sp in specs)
    words = [sp["cfg"].state_words(RATE) for sp in specs]
    pitch = max(words) + pitch_extra
    host_rows = np.full((S, pitch), GUARD, dtype=np.int64).astype(np.int32)
    for s, w in enumerate(words):
        host_rows[s, :w] = 0
    state = torch.from_numpy(host_rows.copy()).to(dev)
    at, host_state, ints, got_all = [0] * S, [None] * S, [pace.FRESH] * S, [[] for _ in range(S)]
    for k in range(steps):
        src, dst, cfgs, reqs, fin, expect = [], [], [], [], [], []
        fmax = 0
        for s, sp in enumerate(specs):
            n = sp["cuts"][k] if k < len(sp["cuts"]) else None
            cfg = sp["cfg"]
            last = sp["final"] and all(c is None for c in sp["cuts"][k + 1:])
            if n is None:
                src.append(None), dst.append(None), cfgs.append(None), reqs.append([]), fin.append(False), expect.append(None)
                continue
            H, D = cfg.samples(RATE)
            x = sp["x"][at[s]:at[s] + n]
            y, st2, off, sc = pace.scan(x, sp["requests"], cfg, RATE, state=host_state[s], final=last)
            nxt, frames, n_out = pace.advance(ints[s], sp["requests"], n, last, H, D, cfg.initial_permille)
            assert (n_out, frames) == (y.shape[0], off.shape[0]) and nxt == pace.ints_of(st2) and n_out <= pace.max_out(n, H, D)
            xs = torch.zeros(n + 8, dtype=torch.float32, device=dev)
            assert xs.data_ptr() % 16 == 0
            xs[sp["so"]:sp["so"] + n] = torch.from_numpy(x)
            src.append(xs[sp["so"]:sp["so"] + n] if n else None)
            arena = torch.full((y.shape[0] + 24,), GUARD, dtype=torch.int32, device=dev)
            a = 8 + sp["do"]
            dst.append(arena.view(torch.float32)[a:a + y.shape[0]])
            want = np.full(arena.shape[0], GUARD, dtype=np.int64).astype(np.int32)
            want[a:a + y.shape[0]] = y.numpy().view(np.int32)
            cfgs.append(cfg), reqs.append(sp["requests"]), fin.append(last)
            idle = n == 0 and not last
            expect.append((arena, want, off, sc, nxt, frames, idle))
            at[s] += n
            host_state[s] = st2
            if not idle:
                host_rows[s, :words[s]] = st2.numpy()
            fmax = max(fmax, off.shape[0])
            got_all[s].append(y.numpy())
        ooff = torch.full((S, fmax + 3), GUARD, dtype=torch.int32, device=dev)
        osc = torch.full((S, fmax + 3), GUARD, dtype=torch.int32, device=dev)
        out, after, frames = pace.pace_items(src, dst, cfgs, reqs, ints, fin, state, ooff, osc.view(torch.float32), RATE)
        torch.cuda.synchronize()
        rows = state.cpu().numpy()
        for s, e in enumerate(expect):
            assert np.array_equal(rows[s], host_rows[s]), (k, s, np.nonzero(rows[s] != host_rows[s])[0][:8], rows[s][:16], host_rows[s][:16])
            got_off, got_sc = ooff[s].cpu().numpy(), osc[s].cpu().numpy()
            if e is None or e[6]:
                assert out[s] == 0 and frames[s] == 0 and after[s] == ints[s]
                assert (got_off == np.int32(GUARD)).all() and (got_sc == np.int32(GUARD)).all()
                continue
            arena, want, off, sc, nxt, fr, _ = e
            got = arena.cpu().numpy()
            assert out[s] == want.shape[0] - 24 and after[s] == nxt and frames[s] == fr
            assert np.array_equal(got, want), (k, s, np.nonzero(got != want)[0][:8], want.shape)
            F = off.shape[0]
            assert np.array_equal(got_off[:F], off.numpy()) and (got_off[F:] == np.int32(GUARD)).all(), (k, s, got_off[:F], off)
            assert np.array_equal(got_sc[:F], sc.numpy().view(np.int32)) and (got_sc[F:] == np.int32(GUARD)).all(), (k, s)
            ints[s] = nxt
    searched = 0
    for s, sp in enumerate(specs):
        if host_state[s] is not None:
            searched += int(host_state[s][pace.I_SEARCHED])
        if whole and sp["final"] and got_all[s]:
            y1 = pace.scan(sp["x"][:at[s]], sp["requests"], sp["cfg"], RATE, final=True)[0].numpy()
            assert np.array_equal(np.concatenate(got_all[s]).view(np.int32), y1.view(np.int32)), s
    return searched


def bounds(H, D, requests, count, initial=1000):
    """the readiness bounds of the first `count` frames"""
    a, out = [0], [H]
    for k in range(1, count):
        r = pace.rate_at(requests, initial, a[-1])
        a.append(a[-1] + pace.analysis_hop(H, r))
        out.append(max(a[k - 1] + 2 * H, a[k] + H) + D)
    return out


@pytest.mark.parametrize("H,D", SIZES)
def test_counts_fresh_continued_and_flushed(dev, H, D):
    """every count of the issue as a first launch, continued by a second one and flushed by a last step without samples"""
    cfg = config(H, D)
    req = [(0, 1500)]
    b = bounds(H, D, req, 4)
    counts = [None, 0, 1, H - 1] + [v for e in b for v in (e - 1, e)] + [pace.WINDOW + 1]
    specs = [spec(cfg, [c, counts[(i + 5) % len(counts)] or 7, 0 if c is not None else None], seed=H + D + i, requests=req, so=i % 4,
                  do=(i + 1) % 4) for i, c in enumerate(counts)]
    specs[0]["cuts"] = [None, None, None]                                       # a row that stays idle throughout: sentinels untouched
    assert run(specs, dev) > 0


@pytest.mark.parametrize("H,D", [(64, 8), (256, 160)])
def test_rates_and_changes_inside_and_between_launches(dev, H, D):
    cfg = config(H, D)
    n = [9 * H + 3, 7 * H, 11 * H + 1, 0]
    inside = [(4 * H + 5, 1800)]                                                # takes effect inside launch 0
    between = [(9 * H + 3, 600)]                                                # at the first sample of launch 1
    many = [(0, 1900), (2 * H, 520)] + [(10 * H + 40 * k, 700 + 150 * k) for k in range(7)]
    specs = [spec(cfg, n, 10 + i, [(0, r)], so=i % 4) for i, r in enumerate((500, 999, 1000, 1001, 2000))]
    specs += [spec(cfg, n, 20, inside, do=1), spec(cfg, n, 21, between, do=2), spec(cfg, n, 22, inside + between + [(20 * H, 2000)]),
              spec(cfg, n, 23, many, so=3), spec(config(H, D, initial_permille=1250), n, 24, [(12 * H, 1000)])]
    assert run(specs, dev) > 0
    assert len(pace.live(many, 1000, 2 * H)[0]) == 7 and pace.live(many, 1000, 50 * H) == ([], 1600)


@pytest.mark.parametrize("H,D", [(64, 8), (512, 512)])
def test_the_end_of_the_stream(dev, H, D):
    cfg = config(H, D)
    fast = [(0, 2000)]                                                          # a_k = 2 H k
    specs = [spec(cfg, [H - 5], 1), spec(cfg, [1], 2), spec(cfg, [0], 3),       # L < H, L = 1, an empty stream
             spec(cfg, [3, H - 9, 0], 4),                                       # L < H in three launches, the last without samples
             spec(cfg, [6 * H + 1], 5, fast), spec(cfg, [7 * H], 6, fast),      # L - a_{K-1} = 1 and = H
             spec(cfg, [5 * H, H + 1], 7, fast), spec(cfg, [5 * H, 2 * H, 0], 8, fast, so=1, do=3),
             spec(cfg, [5 * H + 7, None, 0], 9, [(0, 700)]),                    # final with no new samples behind an idle step
             spec(cfg, [4 * H, 4 * H], 10, [(0, 1300)], final=False)]           # a stream that does not end
    assert run(specs, dev) > 0


def test_quiet_stretch_and_the_tie_rule(dev):
    H = 64
    tie24 = np.tile(signal(24, 11), 40)[:12 * H].astype(np.float32)            # candidates 24 apart see identical segments
    tie16 = np.tile(signal(16, 12), 60)[:12 * H].astype(np.float32)
    tie24[:] = np.tile(np.random.default_rng(11).standard_normal(24).astype(np.float32) * np.float32(0.3), 40)[:12 * H]
    tie16[:] = np.tile(np.random.default_rng(12).standard_normal(16).astype(np.float32) * np.float32(0.3), 60)[:12 * H]
    y, st, off, q = pace.scan(tie24, [(0, 2000)], config(H, 16), RATE, final=True)
    assert off[1] == 8                                                          # d = 8 and d = -16 tie: the smaller |d|
    y, st, off, q = pace.scan(tie16, [(0, 1375)], config(H, 8), RATE, final=True)
    assert off[1] == -8                                                         # d = -8 and d = 8 tie: the negative one
    quiet = signal(20 * H, 5)
    quiet[:6 * H] *= np.float32(1e-5)
    specs = [spec(config(H, 16), [12 * H], x=tie24, requests=[(0, 2000)]), spec(config(H, 8), [5 * H, 7 * H], x=tie16, requests=[(0, 1375)]),
             spec(config(H, 8), [20 * H], x=quiet, requests=[(0, 2000)]), spec(config(H, 8), [3 * H, 9 * H, 8 * H], x=quiet, requests=[(0, 600)]),
             spec(config(H, 8, floor=0.0), [20 * H], x=quiet, requests=[(0, 2000)]),
             spec(config(H, 8), [20 * H], x=np.zeros(20 * H, dtype=np.float32), requests=[(0, 1500)])]
    run(specs, dev)


def test_every_alignment_of_source_and_destination(dev):
    cfg = config(64, 8)
    run([spec(cfg, [5 * 64 + 5, 170, 0], seed=a, requests=[(0, 1400)], so=a % 4, do=a // 4) for a in range(16)], dev)


def test_one_slot_seventeen_slots_and_idle_rows_between_busy_ones(dev):
    a, b, c = config(64, 8), config(256, 160), config(128, 0)
    assert run([spec(b, [3000, 2000, 1000], 1, [(0, 1250)])], dev) > 0
    specs = []
    for i in range(17):
        cfg = (a, b, c)[i % 3]
        if i % 4 == 1:
            specs.append(spec(cfg, [None] * 4, i))
        else:
            cuts = [[700, None, 900, 0], [None, 2500, 1, None], [1, 1, 1, 1], [pace.WINDOW + 1, None, None, 100]][i % 4]
            specs.append(spec(cfg, cuts, i, [(0, 600 + 85 * i)], so=i % 4, do=(i + 2) % 4))
    assert run(specs, dev) > 0


def test_three_launches_in_a_row_against_one_scan_and_against_three(dev):
    """three launches on one stream without a look at the device between them: the table scratch of a launch may be overwritten as
    soon as the call returns"""
    H, D = 256, 160
    cfg = config(H, D)
    x = signal(9000, 3, H)
    req = [(0, 1250), (4000, 800)]
    cuts = [2500, 3500, 3000]
    state = torch.zeros((1, cfg.state_words(RATE)), dtype=torch.int32, device=dev)
    table = torch.empty(pace.TABLE_WORDS, dtype=torch.int32, device=dev)
    weights, woff = pace.weight_arena([H], dev)
    xd = torch.from_numpy(x).to(dev)
    ints, at, outs, frs = pace.FRESH, 0, [], []
    for i, n in enumerate(cuts):
        y = torch.full((pace.max_out(n, H, D),), float("nan"), dtype=torch.float32, device=dev)
        ooff = torch.zeros((1, 64), dtype=torch.int32, device=dev)
        osc = torch.zeros((1, 64), dtype=torch.float32, device=dev)
        out, after, frames = pace.pace_items([xd[at:at + n]], [y], [cfg], [req], [ints], [i == 2], state, ooff, osc, RATE, weights, woff, table)
        outs.append((y, out[0], ooff, osc, frames[0]))
        ints, at = after[0], at + n
    torch.cuda.synchronize()
    got = np.concatenate([y[:n].cpu().numpy() for y, n, _, _, _ in outs])
    y1, st1, off1, sc1 = pace.scan(x, req, cfg, RATE, final=True)
    assert np.array_equal(got.view(np.int32), y1.numpy().view(np.int32))
    assert np.array_equal(np.concatenate([o[0, :f].cpu().numpy() for _, _, o, _, f in outs]), off1.numpy())
    assert np.array_equal(np.concatenate([q[0, :f].cpu().numpy() for _, _, _, q, f in outs]).view(np.int32), sc1.numpy().view(np.int32))
    assert torch.equal(state[0].cpu(), st1)
    st, at = None, 0
    for i, n in enumerate(cuts):
        y3, st, _, _ = pace.scan(x[at:at + n], req, cfg, RATE, state=st, final=i == 2)
        assert np.array_equal(outs[i][0][:outs[i][1]].cpu().numpy().view(np.int32), y3.numpy().view(np.int32))
        at += n
    assert torch.equal(st, st1) and pace.report(state[0]) == pace.report(st1) and pace.report(st1).searched > 3


def test_one_record_per_launch_and_none_when_every_slot_is_idle(dev):
    cfg = config(64, 8)
    state = torch.full((2, cfg.state_words(RATE)), GUARD, dtype=torch.int32, device=dev)
    fr = torch.full((2, 4), GUARD, dtype=torch.int32, device=dev)
    args = ([None, None], [None, None], [None, None], [[], []], [pace.FRESH, pace.FRESH], [False, False], state, fr,
            fr.clone().view(torch.float32), RATE)
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        assert pace.pace_items(*args)[0] == [0, 0]
        torch.cuda.synchronize()
        assert _lib.prof_read("pace")["launches"] == 0
        assert (state.cpu() == GUARD).all() and (fr.cpu() == GUARD).all()
        run([spec(cfg, [500], 1, [(0, 1500)]), spec(cfg, [None], 2)], dev)
        assert _lib.prof_read("pace")["launches"] == 1
    finally:
        _lib.prof_enable(False)
        _lib.prof_reset()


def test_refusals_name_the_item_and_launch_nothing(dev):
    H, D, S = 64, 8, 2
    n = 5 * H
    x = torch.zeros(n, dtype=torch.float32, device=dev)
    y = torch.full((2 * n,), 7.0, dtype=torch.float32, device=dev)
    state = torch.full((S, 16 + 2 * H + 2 * D), GUARD, dtype=torch.int32, device=dev)
    ooff = torch.full((S, 8), GUARD, dtype=torch.int32, device=dev)
    osc = torch.full((S, 8), GUARD, dtype=torch.int32, device=dev)
    table = torch.zeros(pace.TABLE_WORDS * S, dtype=torch.int32, device=dev)
    weights, _ = pace.weight_arena([H], dev)
    frames = pace.advance(pace.FRESH, [(10, 1500), (10, 700)], n, False, H, D)[1]
    assert 2 <= frames <= 8

    def call(**kw):
        a = dict(dst=[None, y.data_ptr()], cap=[0, 2 * n], src=[None, x.data_ptr()], n_new=[0, n], ints=[0] * 5 + [0, 0, 0, 0, 0], flags=[0, 0],
                 H=[-1, H], D=[-1, D], fp=[0.0, 0.0, 1e-6, 1e-12], base=[0, 1000], count=[99, 2], reqs=[0] * 16 + [10, 1500, 10, 700] + [0] * 12,
                 S=S, wfloats=int(weights.numel()), woff=[0, 0], pitch=int(state.shape[1]), out_pitch=8)
        a.update(kw)
        n_s = len(a["n_new"])
        P, I64, I32 = C.c_void_p * n_s, C.c_int64 * n_s, C.c_int32 * n_s
        return _lib.lib().dmel_pace_items(P(*a["dst"]), I64(*a["cap"]), P(*a["src"]), I64(*a["n_new"]), (C.c_int64 * (5 * n_s))(*a["ints"]),
                                          I32(*a["flags"]), I32(*a["H"]), I32(*a["D"]), (C.c_float * (2 * n_s))(*a["fp"]), I32(*a["base"]),
                                          I32(*a["count"]), (C.c_int32 * (16 * n_s))(*a["reqs"]), a["S"], weights.data_ptr(), a["wfloats"],
                                          I32(*a["woff"]), state.data_ptr(), a["pitch"], ooff.data_ptr(), osc.data_ptr(), a["out_pitch"],
                                          table.data_ptr(), _lib.stream_ptr())

    def refused(what, **kw):
        rc = call(**kw)
        msg = _lib.lib().dmel_last_error().decode()
        assert rc != 0 and what in msg, (kw, rc, msg)

    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        refused("0 items", S=0)
        refused("item 1: a hop of 56", H=[-1, 56])
        refused("item 1: a hop of 520", H=[-1, 520])
        refused("item 1: a hop of 68", H=[-1, 68])
        refused("item 1: a search half-width of 513", D=[-1, 513])
        refused("item 1: a search half-width of -1", D=[-1, -1])
        refused("item 1: a rate of 499", base=[0, 499])
        refused("item 1: a rate of 2001", base=[0, 2001])
        refused("item 1: request 1: a rate of 2001", reqs=[0] * 16 + [10, 1500, 10, 2001] + [0] * 12)
        refused("item 1: request 1: position 9", reqs=[0] * 16 + [10, 1500, 9, 700] + [0] * 12)
        refused("item 1: 9 live requests", count=[99, 9])
        refused(f"item 1: {2 * H + 2 * D} held samples", ints=[0] * 5 + [3, 2 * H, 3 * H, 1000, 2 * H + 2 * D])
        refused("item 1: a state row of", pitch=16 + 2 * H + 2 * D - 1)
        refused("item 1: the step hands out", cap=[0, frames * H - 1])
        refused("item 1: the step completes", out_pitch=frames - 1)
        refused("item 1: the integers", ints=[0] * 5 + [0, 0, 5, 0, 0])
        refused("item 1: the integers", ints=[0] * 5 + [2, 64, 64 + 2 * H + 1, 1000, 10])
        refused("item 1: NULL source", src=[None, None])
        refused("item 1: NULL destination", dst=[None, None])
        refused("item 1: a pointer is not 4-byte aligned", src=[None, x.data_ptr() + 2])
        refused("item 1: floor", fp=[0.0, 0.0, -1.0, 1e-12])
        refused("item 1: weight table", woff=[0, 2])                     # the arena ends in one spare word
        refused("item 1: flags 2", flags=[0, 2])
        refused("item 1: -1 new samples", n_new=[0, -1])
        torch.cuda.synchronize()
        assert _lib.prof_read("pace")["launches"] == 0
        assert (state.cpu() == GUARD).all() and (ooff.cpu() == GUARD).all() and (y.cpu() == 7.0).all()
        state.zero_()
        assert call() == 0                                                      # the accepted call the refusals vary
        torch.cuda.synchronize()
        assert _lib.prof_read("pace")["launches"] == 1 and int(state[1, pace.I_K]) == frames and (state[0] == 0).all()
    finally:
        _lib.prof_enable(False)
        _lib.prof_reset()
