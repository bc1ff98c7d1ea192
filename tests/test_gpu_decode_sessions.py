"""Independent decode sessions on the GPU.  Every comparison is torch.equal, and every reference is a path that existed before the
per-item layered step did: dmel_wavenet_stream_step on one utterance at a time, decode() on one finished token sequence."""
import ctypes as C

import pytest
import torch

from test_gpu_parity import make_codec, randomise

pytestmark = pytest.mark.gpu

L = 5
DILS = [2 ** (i % 4) for i in range(L)]          # 1 2 4 8 1: level l runs 0 1 3 7 15 16 columns behind level 0
CAP, UPTO, SHIFT = 256, 150, 40
SENTINEL = -777.0
PRECISIONS = ["fp32_f16x2", "fp32_bf16x3"]       # the two parity decode precisions (VQGAN.set_decode_precision "fp32" / "fp32_bf16x3")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------ 1. / 2. / 3. the per-item layered step
def frontiers(prev, upto, final):
    nxt = [upto]
    for l, d in enumerate(DILS):
        nxt.append(upto if final else max(prev[l + 1], nxt[-1] - d))
    return nxt


def make_decoder(C_res, C_cond, C_out, dev, precision):
    from dmel_codec_amd.models.modules.wavenet import WaveNet
    torch.manual_seed(C_res)
    m = WaveNet(output_channels=C_out, residual_channels=C_res, residual_layers=L, dilation_cycle=4, condition_channels=C_cond)
    randomise(m, 11 + C_res)
    m = m.to(dev)
    m.set_precision(precision)
    return m


def scratch_for(m, N, R, dev):
    return torch.empty(2 * N * m.residual_channels * CAP + 2 * N + R * (2 * (L + 1) + 1), device=dev)


def step_lockstep(m, hist, skip, cond, y, prev, nxt):
    """the parent's path: dmel_wavenet_stream_step, one window for all items of the call"""
    from dmel_codec_amd import _lib
    N = skip.shape[0]
    row = C.c_int64 * (L + 1)
    with torch.cuda.device(skip.device):
        _lib.check(_lib.lib().dmel_wavenet_stream_step(m.native(), hist.data_ptr(), skip.data_ptr(), cond.data_ptr(), y.data_ptr(),
                                                       scratch_for(m, N, 1, skip.device).data_ptr(), N, CAP, row(*prev), row(*nxt),
                                                       _lib.stream_ptr()), "wavenet_stream_step")


def step_items(m, st, prev_rows, next_rows, origins, cap=CAP):
    """-> (return code, message); the host tables are overwritten right after the call (the library must not read them later)"""
    from dmel_codec_amd import _lib
    R = len(origins)
    tab = C.c_int64 * (R * (L + 1))
    p, n, o = tab(*sum(prev_rows, [])), tab(*sum(next_rows, [])), (C.c_int64 * R)(*origins)
    with torch.cuda.device(st.skip.device):
        rc = _lib.lib().dmel_wavenet_stream_step_items_layered(m.native(), None, st.hist.data_ptr(), st.skip.data_ptr(), st.cond.data_ptr(),
                                                               st.y.data_ptr(), scratch_for(m, st.N, R, st.skip.device).data_ptr(), st.N, cap,
                                                               p, n, None, st.div, o, _lib.stream_ptr())
    msg = _lib.lib().dmel_last_error().decode(errors="replace") if rc else ""
    for t in (p, n):
        for i in range(len(t)):
            t[i] = -1
    for i in range(R):
        o[i] = -1
    return rc, msg


class State:
    """Buffers of 4 utterances x `div` items each, filled by lockstep dmel_wavenet_stream_step calls up to frame UPTO."""

    def __init__(self, m, div, dev, seed):
        self.m, self.div, self.N = m, div, 4 * div
        Cr, Cc, Co = m.residual_channels, m.condition_channels, m.output_channels
        g = torch.Generator().manual_seed(seed)
        self.hist = torch.zeros(L + 1, self.N, Cr, CAP, device=dev)
        self.hist[0] = torch.randn(self.N, Cr, CAP, generator=g).to(dev)            # level 0 is the caller's: the injected noise
        self.cond = torch.randn(self.N, Cc, CAP, generator=g).to(dev)
        self.skip = torch.zeros(self.N, Cr, CAP, device=dev)
        self.y = torch.zeros(self.N, Co, CAP, device=dev)
        self.base = frontiers([0] * (L + 1), UPTO, False)
        step_lockstep(m, self.hist, self.skip, self.cond, self.y, [0] * (L + 1), self.base)

    def tensors(self):
        return self.hist, self.skip, self.cond, self.y

    def items(self, r):
        return slice(r * self.div, (r + 1) * self.div)

    def shift(self, r, by):
        """re-base utterance r: its columns move `by` to the left (its origin becomes `by`)"""
        for t in self.tensors():
            v = t[..., self.items(r), :, :]
            v[..., :CAP - by] = v[..., by:].clone()


# Column counts per level (levels 1 .. 5) of the four utterances -- idle / mid-stream behind a re-based origin / final / first push:
#   "wide":   0 / 1  / 82 84 88 96 97 / 129 127 123 115 114      largest window per level 129 .. 114: two 96-column tiles, three of 64
#   "narrow": 0 / 33 /  2  4  8 16 17 /  89  87  83  75  74      largest window per level  89 .. 74: one 96-column tile, two of 64
# so 1, 33, 97 and 130 (level 0 of the first push in "wide") all occur, next to windows that end inside every tile width.
WIDTHS = {"wide": (1, 81, 130), "narrow": (33, 1, 90)}        # mid-stream advance, final tail behind UPTO, first push


def rows_for(st, widths):
    adv, tail, first = WIDTHS[widths]
    base = st.base
    prev = [list(base), [p - SHIFT for p in base], list(base), [0] * (L + 1)]
    nxt = [list(base), [p - SHIFT for p in frontiers(base, UPTO + adv, False)], [UPTO + tail] * (L + 1), frontiers([0] * (L + 1), first, False)]
    return prev, nxt, [0, SHIFT, 0, 0]


# Tiles.  pick_tile_bf16 under a table sees (row tiles of the packed weights, largest window T of the launch, operand pieces, K steps,
# batch N = 4 div) and, of a launch, counts wgs(t) = ceil(32 mtiles / BM_t) * ceil(T / BN_t) * N workgroups.  Row tiles: the gate and
# res / skip convolutions pack 2 * ceil16(C) rows (C = 272: 17 tiles, 40: 3), skip_projection C rows (272: 9, 40: 2), output_projection
# its outputs (80: 3, 12: 1).  Fp16 split (it can return 1, 2, 3, 5, 6, 7), C = 272:
#   7 (256 x 96): mtiles >= 8 and T > 96 and wgs(7) >= 128.  "wide", div 8: gate 3 * 2 * 32 = 192, skip_projection 2 * 2 * 32 = 128.
#   1 (128 x 96): mtiles >= 4, T <= 96, wgs(1) >= 128.       "narrow", div 8: gate 5 * 1 * 32 = 160.
#   6 (128 x 64): wgs(1) < 128 <= wgs(6).                    "narrow", div 8: skip_projection at T = 74: wgs(1) = 3 * 1 * 32 = 96, wgs(6) = 3 * 2 * 32.
#   5 (128 x 32): wgs(6) < 128 too.                          "wide", div 1: gate 3 * 2 * 4 -> wgs(6) = 5 * 3 * 4 = 60.
#   2 (64 x 128): 2 <= mtiles < 4: output_projection to 80 channels; C = 40: gate, res / skip, skip_projection.
#   3 (32 x 256): mtiles = 1: C = 40's output_projection to 12 channels.
# fp32_bf16x3 (1, 2, 3 under a table): 1 for every mtiles >= 4 launch of C = 272; 2 and 3 as above.
CASES = [(272, 272, 80, 8, "wide"), (272, 272, 80, 8, "narrow"), (272, 272, 80, 1, "wide"), (40, 24, 12, 1, "wide"), (40, 24, 12, 1, "narrow")]
_RUNS = {}


def run_case(dev, case, precision):
    """state with sentinels behind every frontier -> (state before, expected from single-item steps, state after the item step, rows)"""
    key = (case, precision)
    if key in _RUNS:
        return _RUNS[key]
    Cr, Cc, Co, div, widths = case
    m = make_decoder(Cr, Cc, Co, dev, precision)
    st = State(m, div, dev, Cr + div)
    st.shift(1, SHIFT)
    prev, nxt, org = rows_for(st, widths)
    for r in range(4):
        it = st.items(r)
        st.hist[0][it, :, nxt[r][0]:] = SENTINEL           # level 0 and the condition are the caller's up to next[0]
        st.cond[it, :, nxt[r][0]:] = SENTINEL
        for l in range(1, L + 1):
            st.hist[l][it, :, prev[r][l]:] = SENTINEL
        st.skip[it, :, prev[r][1]:] = SENTINEL             # [prev[L], prev[1]) holds the partial sums of the blocks that are ahead
        st.y[it, :, prev[r][L]:] = SENTINEL
    before = [t.clone() for t in st.tensors()]
    want = [t.clone() for t in st.tensors()]
    for r in range(4):
        if prev[r] == nxt[r]:
            continue                                       # an idle utterance: nothing may change
        it = st.items(r)
        # clone(): a slice of the leading dimension is contiguous already, so contiguous() would hand the state itself to the reference step
        hist, skip, cond, y = st.hist[:, it].clone(), st.skip[it].clone(), st.cond[it].clone(), st.y[it].clone()
        step_lockstep(m, hist, skip, cond, y, prev[r], nxt[r])
        want[0][:, it], want[1][it], want[3][it] = hist, skip, y
    rc, msg = step_items(m, st, prev, nxt, org)
    assert rc == 0, msg
    torch.cuda.synchronize()
    _RUNS.clear()                                          # one case's buffers at a time
    _RUNS[key] = (before, want, st, (prev, nxt))
    return _RUNS[key]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"C{c[0]}-div{c[3]}-{c[4]}")
def test_item_step_equals_single_item_steps(dev, case, precision):
    """Four utterances, four different rows -- idle, mid-stream behind a re-based origin, the final step, the first push from frame 0 --
    in one per-item layered step, against the same rows one utterance at a time through dmel_wavenet_stream_step on clones."""
    before, want, st, _ = run_case(dev, case, precision)
    bad = [l for l in range(L + 1) if not torch.equal(st.hist[l], want[0][l])]
    assert not bad, f"history levels {bad} differ"
    assert torch.equal(st.skip, want[1])
    assert torch.equal(st.cond, want[2])
    assert torch.equal(st.y, want[3])
    assert not torch.equal(st.y, before[3])                # the step did something


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"C{c[0]}-div{c[3]}-{c[4]}")
def test_nothing_outside_the_windows(dev, case, precision):
    """every column outside [prev[l], next[l]) of its own item is what it was: the sentinel behind the frontier, the history in front"""
    before, _, st, (prev, nxt) = run_case(dev, case, precision)
    assert torch.equal(st.hist[0], before[0][0]) and torch.equal(st.cond, before[2])
    for r in range(4):
        it = st.items(r)
        for l in range(1, L + 1):
            h = st.hist[l][it]
            assert torch.equal(h[..., :prev[r][l]], before[0][l][it][..., :prev[r][l]])
            assert bool((h[..., nxt[r][l]:] == SENTINEL).all()), f"utterance {r} level {l}: a column behind next was written"
            assert not bool((h[..., prev[r][l]:nxt[r][l]] == SENTINEL).any())
        assert torch.equal(st.skip[it][..., :prev[r][L]], before[1][it][..., :prev[r][L]])
        lo = nxt[r][1] if nxt[r] != prev[r] else prev[r][1]
        assert bool((st.skip[it][..., lo:] == SENTINEL).all())
        assert torch.equal(st.y[it][..., :prev[r][L]], before[3][it][..., :prev[r][L]])
        assert bool((st.y[it][..., nxt[r][L]:] == SENTINEL).all())
        assert not bool((st.y[it][..., prev[r][L]:nxt[r][L]] == SENTINEL).any())
    it = st.items(0)                                       # the idle utterance, whole
    for a, b in zip(st.tensors(), before):
        assert torch.equal(a[..., it, :, :], b[..., it, :, :])


def test_refusals_leave_every_buffer_alone(dev):
    m = make_decoder(40, 24, 12, dev, "fp32_f16x2")
    st = State(m, 1, dev, 5)
    st.shift(1, SHIFT)
    prev, nxt, org = rows_for(st, "narrow")
    before = [t.clone() for t in st.tensors()]

    def refused(p, n, o, code, *words, cap=CAP):
        rc, msg = step_items(m, st, p, n, o, cap)
        torch.cuda.synchronize()
        assert rc == code, (rc, msg)
        for w in words:
            assert w in msg, msg
        for a, b in zip(st.tensors(), before):
            assert torch.equal(a, b)

    ahead = [list(r) for r in nxt]
    ahead[2] = list(frontiers(st.base, UPTO + 20, False))
    ahead[2][3] = ahead[2][2]                              # level 3 as far as its input, mid-stream
    refused(prev, ahead, org, -1, "utterance 2", "runs ahead of its input")
    refused(prev, nxt, [0, SHIFT, 0, 7], -1, "utterance 3", "needs history in front of the buffer")      # a re-based row whose first push starts at column 0
    over = [list(r) for r in nxt]
    over[2] = [CAP + 1] * (L + 1)
    refused(prev, over, org, -1, "utterance 2", "cap")
    refused(prev, nxt, org, -1, "utterance 2", cap=UPTO)                        # good rows, but the final one ends behind this capacity
    m.set_precision("fp32_mfma")                            # a forced native fp32 MFMA has no per-item windows
    refused(prev, nxt, org, -2, "split kernels")
    m.set_precision("fp32_f16x2")
    rc, msg = step_items(m, st, prev, nxt, org)
    assert rc == 0, msg


# ------------------------------------------------------------------------------------ 4. / 5. / 6. the pool
@pytest.fixture(scope="module")
def codec(dev):
    return make_codec(700, n_mels=80, dmel_groups=8, encoder_layers=2).to(dev)


def clip(codec, seed, T, dev):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 175, (8, T), generator=g, dtype=torch.int32).to(dev)
    noise = torch.randn(codec.decoder.residual_channels, T * 4, generator=g).to(dev)
    return ids, noise


def whole(codec, ids, noise):
    T = ids.shape[1]
    audio, mel = codec.decode(ids[None], torch.tensor([T], device=ids.device), return_audios=True, noise=noise[None])
    return audio[0], mel[0]


class Feeder:
    """one session: its clip, how far it has been pushed, the pieces that came back"""

    def __init__(self, pool, ids, noise):
        self.slot, self.ids, self.noise, self.pos, self.audio, self.mel = pool.open(), ids, noise, 0, [], []

    def take(self, n):
        a = self.pos
        self.pos += n
        return self.ids[:, a:self.pos], self.noise[:, 4 * a:4 * self.pos]

    def got(self, out):
        audio, mel = out
        assert audio.shape == (1, mel.shape[1] * 256) and mel.shape[0] == 80
        self.audio.append(audio)
        self.mel.append(mel)

    def check(self, codec):
        assert self.pos == self.ids.shape[1]
        audio, mel = whole(codec, self.ids, self.noise)
        assert torch.equal(torch.cat(self.mel, dim=1), mel)
        assert torch.equal(torch.cat(self.audio, dim=1), audio)


def step(pool, feeders, plan, final=()):
    """plan: {feeder index: tokens}; final: feeder indices that end with this push"""
    ids, noise = {}, {}
    for i, n in plan.items():
        f = feeders[i]
        ids[f.slot], noise[f.slot] = f.take(n)
    out = pool.push(ids, noise=noise, final=[feeders[i].slot for i in final])
    assert set(out) == set(ids)
    for i in plan:
        feeders[i].got(out[feeders[i].slot])


@pytest.mark.parametrize("precision", ["fp32", "fp32_bf16x3"])
def test_sessions_equal_decode_of_each_clip(dev, codec, precision):
    """3 slots, 4 sessions (one slot is reused): staggered opens, ragged pushes with 0- and 1-token pushes, one session shorter than
    the lookahead, one closing with tokens in its final push and one without; injected noise."""
    codec.set_decode_precision(precision)
    try:
        pool = codec.decode_sessions(3, max_push_tokens=64)
        lengths = [150, 3, 97, 60]
        clips = [clip(codec, 40 + i, T, dev) for i, T in enumerate(lengths)]
        f = [Feeder(pool, *clips[0])]
        step(pool, f, {0: 37})
        f.append(Feeder(pool, *clips[1]))
        step(pool, f, {0: 1, 1: 2})
        f.append(Feeder(pool, *clips[2]))
        step(pool, f, {0: 64, 1: 1, 2: 30}, final=(1,))                   # session 1 ends after 3 tokens: shorter than the lookahead
        assert pool.open_slots == [f[0].slot, f[2].slot]
        f.append(Feeder(pool, *clips[3]))                                  # takes over session 1's slot
        assert f[3].slot == f[1].slot
        step(pool, f, {0: 0, 2: 50, 3: 60})
        step(pool, f, {2: 17}, final=(2,))                                 # closes with tokens in its final push
        step(pool, f, {0: 48, 3: 0})
        f[0].got(pool.close(f[0].slot))                                    # closes without
        f[3].got(pool.close(f[3].slot))
        assert pool.open_slots == []
        for s in f:
            s.check(codec)
    finally:
        codec.set_decode_precision("fp32")


def test_slot_reuse_and_bounded_state(dev, codec):
    long_clip, short_clip = clip(codec, 61, 130, dev), clip(codec, 62, 45, dev)

    def serve(pool, c, sizes):
        f = [Feeder(pool, *c)]
        for n in sizes[:-1]:
            step(pool, f, {0: n})
        step(pool, f, {0: sizes[-1]}, final=(0,))
        return torch.cat(f[0].audio, dim=1), torch.cat(f[0].mel, dim=1)

    used = codec.decode_sessions(1, max_push_tokens=64)
    serve(used, long_clip, [64, 64, 2])
    a_used, m_used = serve(used, short_clip, [20, 25])
    a_fresh, m_fresh = serve(codec.decode_sessions(1, max_push_tokens=64), short_clip, [20, 25])
    assert torch.equal(m_used, m_fresh) and torch.equal(a_used, a_fresh)
    # 600 tokens in pushes of 16 through one slot: the state neither grows nor moves
    pool = codec.decode_sessions(1, max_push_tokens=16)
    ids, noise = clip(codec, 63, 600, dev)
    f = [Feeder(pool, ids, noise)]
    step(pool, f, {0: 16})
    size, ptrs = pool.allocated_bytes(), {k: t.data_ptr() for k, t in pool.buf.items()}
    assert size > 0 and pool.capacity < 600                        # far fewer columns than the stream's 2400 frames
    for _ in range(36):
        step(pool, f, {0: 16})
    step(pool, f, {0: 8}, final=(0,))
    assert pool.allocated_bytes() == size and {k: t.data_ptr() for k, t in pool.buf.items()} == ptrs
    assert sum(m.shape[1] for m in f[0].mel) == 2400
    f[0].check(codec)


def test_pool_refusals(dev, codec):
    pool = codec.decode_sessions(2, max_push_tokens=8)
    ids, _ = clip(codec, 70, 20, dev)
    with pytest.raises(RuntimeError, match="not open"):
        pool.push({0: ids[:, :4]})
    a, b = pool.open(), pool.open()
    with pytest.raises(RuntimeError, match="taken"):
        pool.open()
    with pytest.raises(ValueError, match="max_push_tokens"):
        pool.push({a: ids[:, :9]})
    with pytest.raises(ValueError):
        pool.push({a: ids[:, :4]}, final=(b,))
    with pytest.raises(ValueError, match="noise"):
        pool.push({a: ids[:, :4]}, noise={a: torch.zeros(560, 4, device=dev)})
    assert pool.buf is None and pool.allocated_bytes() == 0          # refused before any state changed
    for opt in (dict(overlap_vocoder=True), dict(graph_chunk_tokens=8), dict(output_sample_rate=16000)):
        with pytest.raises(NotImplementedError):
            codec.decode_sessions(2, **opt)
    out = pool.push({a: ids[:, :8], b: ids[:, :0]}, final=(b,))
    assert out[b][1].shape == (80, 0) and out[b][0].shape == (1, 0) and pool.open_slots == [a]
    audio, mel = pool.close(a)
    assert mel.shape == (80, 32) and audio.shape == (1, 32 * 256)
