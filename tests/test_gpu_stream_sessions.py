"""Independent encode sessions on the GPU.  Every comparison is torch.equal, and every reference is a path that existed before the
per-item entries did: dmel_wavenet_stream_step_ex on one utterance at a time, dmel_stft_window_f32 on one clip at a time, encode() on
one finished clip."""
import ctypes as C

import pytest
import torch

from test_gpu_parity import make_codec
from test_gpu_stream_encode import make_encoder

pytestmark = pytest.mark.gpu

L, G, CIN = 20, 2, 10
DILS = [2 ** (i % 4) for i in range(L)]
SENTINEL = -777.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------ 1. / 2. / 7. the per-item encoder step
def frontiers(prev, upto, final):
    nxt = [upto]
    for l, d in enumerate(DILS):
        nxt.append(upto if final else max(prev[l + 1], nxt[-1] - d))
    return nxt


class State:
    """Buffers of R utterances x G groups, filled by lockstep dmel_wavenet_stream_step_ex calls (the parent's path) up to frame `upto`."""

    def __init__(self, m, R, cap, upto, dev, seed):
        self.m, self.R, self.N, self.cap, self.C = m, R, R * G, cap, m.residual_channels
        N = self.N
        self.x = torch.zeros(N, CIN, cap, device=dev)
        self.x[:] = torch.randn(N, CIN, cap, generator=torch.Generator().manual_seed(seed)).to(dev)
        self.hist = torch.zeros(L + 1, N, self.C, cap, device=dev)
        self.skip = torch.zeros(N, self.C, cap, device=dev)
        self.y = torch.zeros(N, self.C, cap, device=dev)
        self.prev = frontiers([0] * (L + 1), upto, False)
        step_ex(m, self.x, self.hist, self.skip, self.y, cap, [0] * (L + 1), self.prev, None, 0)

    def tensors(self):
        return self.x, self.hist, self.skip, self.y

    def shift(self, r, by):
        """re-base utterance r: its columns move `by` to the left (its origin becomes `by`)"""
        for t in self.tensors():
            v = t[..., r * G:(r + 1) * G, :, :]
            v[..., :self.cap - by] = v[..., by:].clone()


def step_ex(m, x, hist, skip, y, cap, prev, nxt, out_len, origin):
    from dmel_codec_amd import _lib
    N = x.shape[0]
    scratch = torch.empty(2 * N * m.residual_channels * cap + 2 * N, device=x.device)
    row = C.c_int64 * (L + 1)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().dmel_wavenet_stream_step_ex(m.native(), x.data_ptr(), hist.data_ptr(), skip.data_ptr(), None, y.data_ptr(),
                                                          scratch.data_ptr(), N, cap, row(*prev), row(*nxt), _lib.ptr(out_len), G, origin,
                                                          _lib.stream_ptr()), "wavenet_stream_step_ex")


def step_items(m, x, hist, skip, y, cap, prev_rows, next_rows, out_len, origins, cond=None):
    """-> return code; the host tables are overwritten right after the call (the library must not read them later)"""
    from dmel_codec_amd import _lib
    N, R = x.shape[0], len(origins)
    scratch = torch.empty(2 * N * m.residual_channels * cap + 2 * N + R * (2 * (L + 1) + 1), device=x.device)
    tab = C.c_int64 * (R * (L + 1))
    p, n, o = tab(*sum(prev_rows, [])), tab(*sum(next_rows, [])), (C.c_int64 * R)(*origins)
    with torch.cuda.device(x.device):
        rc = _lib.lib().dmel_wavenet_stream_step_items(m.native(), x.data_ptr(), hist.data_ptr(), skip.data_ptr(), _lib.ptr(cond), y.data_ptr(),
                                                       scratch.data_ptr(), N, cap, p, n, _lib.ptr(out_len), G, o, _lib.stream_ptr())
    for t in (p, n):
        for i in range(len(t)):
            t[i] = -1
    for i in range(R):
        o[i] = -1
    return rc


def items_against_single_calls(st, prev_rows, next_rows, out_len, origins):
    """one per-item step on the state against one dmel_wavenet_stream_step_ex call per utterance at N = G on copies of it"""
    m, cap = st.m, st.cap
    want = [t.clone() for t in st.tensors()]
    for r in range(st.R):
        if prev_rows[r] == next_rows[r]:
            continue                                             # an idle utterance: nothing may change
        sl = slice(r * G, (r + 1) * G)
        # clone(): a slice of the leading dimension is contiguous already, so contiguous() would hand the state itself to the reference step
        x, hist, skip, y = st.x[sl].clone(), st.hist[:, sl].clone(), st.skip[sl].clone(), st.y[sl].clone()
        step_ex(m, x, hist, skip, y, cap, prev_rows[r], next_rows[r], out_len[r:r + 1].contiguous(), origins[r])
        want[1][:, sl], want[2][sl], want[3][sl] = hist, skip, y
    rc = step_items(m, st.x, st.hist, st.skip, st.y, cap, prev_rows, next_rows, out_len, origins)
    assert rc == 0
    assert torch.equal(st.x, want[0])
    bad = [l for l in range(L + 1) if not torch.equal(st.hist[l], want[1][l])]
    assert not bad, f"history levels {bad} differ"
    assert torch.equal(st.skip, want[2])
    assert torch.equal(st.y, want[3])


@pytest.mark.parametrize("C_res", [70, 40])
def test_item_step_equals_single_item_steps(dev, C_res):
    """Three utterances, three different rows: mid-stream behind a re-based origin, the final step, idle."""
    cap, upto = 256, 150
    m = make_encoder(C_res, 40 + C_res, dev)
    st = State(m, 3, cap, upto, dev, C_res)
    base = st.prev
    st.shift(0, 40)
    rows_p = [[p - 40 for p in base], list(base), list(base)]
    rows_n = [[p - 40 for p in frontiers(base, 190, False)], [170] * (L + 1), list(base)]
    # the idle utterance: a sentinel wherever a step would have written
    for l in range(L + 1):
        st.hist[l, 2 * G:, :, base[l]:base[l] + 40] = SENTINEL
    st.skip[2 * G:, :, base[L]:] = SENTINEL
    st.y[2 * G:, :, base[L]:] = SENTINEL
    out_len = torch.tensor([1000, 160, 1000], device=dev)        # utterance 1 ends at 160: y is masked behind it
    items_against_single_calls(st, rows_p, rows_n, out_len, [40, 0, 0])
    assert float(st.y[G:2 * G, :, 160:170].abs().max()) == 0.0 and float(st.y[G:2 * G, :, base[L]:160].abs().min()) > 0.0
    assert bool((st.hist[L, 2 * G:, :, base[L]:base[L] + 40] == SENTINEL).all()) and bool((st.y[2 * G:, :, base[L]:] == SENTINEL).all())


@pytest.mark.parametrize("C_res", [70, 40])
def test_item_step_is_cut_into_sub_steps_per_row(dev, C_res):
    """200 new columns (three sub-steps) next to 20 (one: idle in the later ones), then both take their final step at different ends."""
    cap, upto = 512, 120
    m = make_encoder(C_res, 60 + C_res, dev)
    st = State(m, 2, cap, upto, dev, 100 + C_res)
    base = st.prev
    nxt = [frontiers(base, 320, False), frontiers(base, 140, False)]
    out_len = torch.tensor([1000, 1000], device=dev)
    items_against_single_calls(st, [list(base), list(base)], nxt, out_len, [0, 0])
    items_against_single_calls(st, nxt, [[333] * (L + 1), [270] * (L + 1)], out_len, [0, 0])       # last level: 88 final columns against 205


def test_item_step_refusals_leave_every_buffer_alone(dev):
    from dmel_codec_amd import _lib
    from dmel_codec_amd.models.modules.wavenet import WaveNet
    from test_gpu_parity import randomise
    cap = 256
    m = make_encoder(70, 7, dev)
    st = State(m, 3, cap, 150, dev, 3)
    base = st.prev
    for t in st.tensors()[1:]:
        t[..., 100:] = SENTINEL
    before = [t.clone() for t in st.tensors()]
    good = frontiers(base, 180, False)
    out_len = torch.tensor([1000, 1000, 1000], device=dev)

    def refused(rows_p, rows_n, origins, what):
        rc = step_items(m, st.x, st.hist, st.skip, st.y, cap, rows_p, rows_n, out_len, origins)
        msg = _lib.lib().dmel_last_error().decode()
        torch.cuda.synchronize()
        assert rc == -1 and "utterance 1" in msg and what in msg, (rc, msg)
        assert all(torch.equal(a, b) for a, b in zip(st.tensors(), before))

    ahead = list(good)
    ahead[3] = good[2]                                           # level 3 would run ahead of its input
    refused([list(base)] * 3, [good, ahead, good], [0, 0, 0], "runs ahead of its input")
    front = [[p - base[L] for p in base] for _ in range(3)]      # column 0 = the last level's frontier: no history in front of it
    refused(front, [front[0], [p - base[L] for p in good], front[2]], [0, base[L], 0], "history in front of the buffer")
    wide = list(good)
    wide[0] = cap + 1
    refused([list(base)] * 3, [good, wide, good], [0, 0, 0], "cap")
    # a conditioned stack is outside the one-launch kernel: unsupported, nothing touched
    torch.manual_seed(1)
    cm = WaveNet(input_channels=10, residual_channels=70, residual_layers=L, dilation_cycle=4, condition_channels=8)
    randomise(cm, 1)
    cm = cm.to(dev)
    cond = torch.zeros(st.N, 8, cap, device=dev)
    rc = step_items(cm, st.x, st.hist, st.skip, st.y, cap, [list(base)] * 3, [good] * 3, out_len, [0, 0, 0], cond=cond)
    torch.cuda.synchronize()
    assert rc == -2 and "one-launch" in _lib.lib().dmel_last_error().decode()
    assert all(torch.equal(a, b) for a, b in zip(st.tensors(), before))


# ------------------------------------------------------------------------------------ 3. per-item STFT windows
def test_stft_items_equal_the_window_call(dev):
    from dmel_codec_amd import _lib
    from dmel_codec_amd.torch_ops import _stft_plan
    from dmel_codec_amd.utils.spectrogram import LinearSpectrogram
    n_fft, hop, Ls = 1024, 256, 6000
    pad = (n_fft - hop) // 2
    spec = LinearSpectrogram(n_fft=n_fft, win_length=n_fft, hop_length=hop, num_mels=80, sample_rate=24000)
    y = (torch.randn(3, Ls, generator=torch.Generator().manual_seed(2)) * 0.3).to(dev)
    T = Ls // hop
    # (first frame, frames, s0, end of the buffer, total length): head with the left reflection; mid-stream with a slack sample in front,
    # the length not known; tail with the right reflection
    wins = [(0, 5, 0, 4 * hop - pad + n_fft, -1),
            (6, 7, 6 * hop - pad - 1, 12 * hop - pad + n_fft, -1),
            (T - 4, 4, (T - 4) * hop - pad, Ls, Ls)]
    width = max(e - s for _, _, s, e, _ in wins) + 3
    buf = torch.full((3, width), 1e30, device=dev)               # whatever lies behind an item's valid samples must not be read
    for b, (_, _, s, e, _) in enumerate(wins):
        buf[b, :e - s] = y[b, s:e]
    want = [spec.forward_window(y[b:b + 1, s:e].contiguous(), s, f, n, total) for b, (f, n, s, e, total) in enumerate(wins)]
    tmax = max(n for _, n, _, _, _ in wins)
    tab = torch.empty(12, dtype=torch.int64, device=dev)
    I = C.c_int64 * 3

    def call(s0, valid, first, frames, total):
        """-> (return code, output (3, 80, max frames) pre-filled with the sentinel)"""
        out = torch.full((3, 80, max(frames)), SENTINEL, device=dev)
        tabs = [I(*v) for v in (s0, valid, first, frames, total)]
        with torch.cuda.device(dev):
            plan = _stft_plan(dev, spec.sample_rate, n_fft, n_fft, hop, 80, float(spec.f_min or 0.0), float(spec.f_max) if spec.f_max else 0.0)
            rc = _lib.lib().dmel_stft_window_items_f32(plan, buf.data_ptr(), width, width, tabs[0], tabs[1], None, out.data_ptr(), None, 3,
                                                       tabs[2], tabs[3], tabs[4], tab.data_ptr(), _lib.stream_ptr())
        for t in tabs:                                           # the caller may overwrite its tables at once
            for i in range(3):
                t[i] = -5
        return rc, out

    cols = [[w[i] for w in wins] for i in range(5)]
    rc, out = call(cols[2], [e - s for _, _, s, e, _ in wins], cols[0], cols[1], cols[4])
    assert rc == 0 and out.shape[2] == tmax
    for b, (f, n, s, e, total) in enumerate(wins):
        assert torch.equal(out[b, :, :n], want[b][0]), b
        assert bool((out[b, :, n:] == SENTINEL).all()), b        # the columns behind an item's frames are not written
    # an idle item (no frames) is left alone entirely
    rc, out = call(cols[2], [e - s for _, _, s, e, _ in wins], cols[0], [5, 0, 4], cols[4])
    assert rc == 0
    assert torch.equal(out[0, :, :5], want[0][0]) and torch.equal(out[2, :, :4], want[2][0]) and bool((out[1] == SENTINEL).all())
    # an item whose frames read a sample its row does not hold is refused and named; nothing is launched
    valid = [e - s for _, _, s, e, _ in wins]
    valid[1] -= 1
    rc, out = call(cols[2], valid, cols[0], cols[1], cols[4])
    assert rc == -1
    msg = _lib.lib().dmel_last_error().decode()
    torch.cuda.synchronize()
    assert "item 1" in msg and "buffer holds" in msg and bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------ 4. / 5. / 6. sessions = encode() per clip
SR, HOP = 24000, 256
LENGTHS = {"a": int(2.3 * SR) + 13, "b": int(1.5 * SR) + 7, "c": int(0.9 * SR) + 1, "d": int(1.1 * SR) + 3}
# clip -> (step of its open(), push sizes in turn, steps in which it is not named); the last push of a clip carries final
WALKS = {"a": (0, [7680, 5000, 7680, 0, 7680, 2560, 7001], {4}),
         "b": (2, [3001, 7680, 7680, 1, 7680], set()),
         "c": (3, [7680, 7000, 6921], set()),
         "d": (6, [7680], set())}              # opened after c has closed: it takes over c's slot
_runs = {}


def plan(total, start, sizes, idle):
    out, pos, step, i = {}, 0, start, 0
    while pos < total:
        if step not in idle:
            n = min(sizes[i % len(sizes)], total - pos)
            out[step] = (pos, n, pos + n == total)
            pos, i = pos + n, i + 1
        step += 1
    return out


def session_run(dev, C_res):
    """the whole scenario once per encoder width: three slots, four clips, ragged pushes; encode() of every clip alone as reference"""
    if C_res not in _runs:
        codec = make_codec(500 + C_res, n_mels=80, dmel_groups=8, vocoder=None, decoder_layers=1, residual_channels=C_res).to(dev)
        clips = {k: (torch.randn(n, generator=torch.Generator().manual_seed(n)) * 0.2).to(dev) for k, n in LENGTHS.items()}
        ref = {k: codec.encode(c[None], torch.tensor([c.shape[0]], device=dev)) for k, c in clips.items()}
        plans = {k: plan(LENGTHS[k], *WALKS[k]) for k in clips}
        pool = codec.encode_sessions(slots=3, max_push_samples=7680)
        slot, got, closed_at, sizes = {}, {k: [] for k in clips}, {}, []
        for step in range(max(max(p) for p in plans.values()) + 1):
            for k in clips:
                if WALKS[k][0] == step:
                    slot[k] = pool.open()
            named = {k: plans[k][step] for k in clips if step in plans[k]}
            audio = {slot[k]: clips[k][pos:pos + n] for k, (pos, n, _) in named.items()}
            ids = pool.push(audio, final=[slot[k] for k, (_, _, fin) in named.items() if fin])
            assert set(ids) == set(audio)
            for k, (_, _, fin) in named.items():
                piece = ids[slot[k]]
                assert piece.dtype == torch.int32 and piece.ndim == 2 and piece.shape[0] == 8
                got[k].append(piece)
                if fin:
                    closed_at[k] = step
            if step == 0:
                sizes.append((pool.capacity, pool.allocated_bytes()))
        sizes.append((pool.capacity, pool.allocated_bytes()))
        _runs[C_res] = dict(codec=codec, pool=pool, slot=slot, got=got, ref=ref, closed_at=closed_at, sizes=sizes, plans=plans)
    return _runs[C_res]


@pytest.mark.parametrize("C_res", [70, 40])
def test_sessions_equal_encode_of_each_clip(dev, C_res):
    r = session_run(dev, C_res)
    assert r["slot"]["a"] != r["slot"]["b"] != r["slot"]["c"] and len(set(r["closed_at"].values())) == 4
    assert any(n == 0 for _, n, _ in r["plans"]["a"].values()) and 4 not in r["plans"]["a"]       # a 0-sample push, an unnamed step
    for k in ("a", "b", "c"):
        ids, lens = r["ref"][k]
        mine = torch.cat(r["got"][k], dim=1)
        assert mine.shape[1] == int(lens[0]) == LENGTHS[k] // HOP // 4, k
        assert torch.equal(mine, ids[0, :, :int(lens[0])]), k
    # c is shorter than the lookahead (25216 samples): every token of it comes with the final push
    assert LENGTHS["c"] < 25216 and all(p.shape[1] == 0 for p in r["got"]["c"][:-1]) and r["got"]["c"][-1].shape[1] > 0
    # a mid-stream session emits exactly what the documented lookahead promises
    assert sum(p.shape[1] for p in r["got"]["a"][:5]) == (7680 * 3 + 5000 - 25216) // (4 * HOP) + 1


def test_a_reused_slot_reads_nothing_of_its_previous_occupant(dev):
    r = session_run(dev, 70)
    assert r["slot"]["d"] == r["slot"]["c"] and WALKS["d"][0] > r["closed_at"]["c"]
    ids, lens = r["ref"]["d"]
    mine = torch.cat(r["got"]["d"], dim=1)
    assert mine.shape[1] == int(lens[0]) and torch.equal(mine, ids[0, :, :int(lens[0])])
    # every slot is free again, and a closed slot takes no push
    pool = r["pool"]
    assert pool.open_slots == []
    with pytest.raises(RuntimeError, match="not open"):
        pool.push({0: r["got"]["a"][0].new_zeros(10, dtype=torch.float32)})


def test_session_state_is_bounded(dev):
    r = session_run(dev, 70)
    assert r["sizes"][0] == r["sizes"][1]                        # the scenario above: nothing grew after the first step
    pool = r["codec"].encode_sessions(slots=3, max_push_samples=7680)
    g = torch.Generator().manual_seed(4)
    slots = [pool.open() for _ in range(3)]
    first = None
    total = 0
    for i in range(40):                                          # 12.8 s per slot, starts staggered by a third of a push
        audio = {s: (torch.randn(7680 if i else 2560 * (s + 1), generator=g) * 0.1).to(dev) for s in slots}
        total += sum(v.shape[1] for v in pool.push(audio).values())
        if first is None:
            first = (pool.capacity, pool.allocated_bytes())
    assert (pool.capacity, pool.allocated_bytes()) == first and first[1] > 0
    assert min(pool.origin) > 0 and max(pool.tail) < 1024      # re-based, and a tail is shorter than one window
    assert total > 3 * 100
    for s in slots:
        pool.close(s)
