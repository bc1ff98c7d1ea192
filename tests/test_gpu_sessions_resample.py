"""Sessions at each sound card's rate on the GPU.  Every comparison is torch.equal, and every reference is a path that existed before
the per-item resample entry did: dmel_resample_window_f32 on one stream at a time, encode(..., sample_rate=r) and
resample(decode() audio) on one finished clip."""
import ctypes as C

import pytest
import torch

from test_gpu_parity import make_codec

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
SR = 24000


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------ the items launch against single-item launches
# (orig, new, signal length, window (s0, s1) or None for "what the outputs read", outputs (o0, o1) with o1 None = the clip's last,
#  length known)
ITEMS = [(48000, 24000, 4000, None, (0, 200), False),          # the head: taps in front of sample 0; fewer than 256 outputs
         (16000, 24000, 3000, None, (1001, 1801), False),      # mid-stream, o0 = 1001 is no multiple of up = 3; 800 = 3 * 256 + 32 outputs
         (44100, 24000, 4000, None, (1500, None), True),       # the end: taps behind total_length; an 80 x 171 bank staged in LDS
         (44100, 48000, 3000, None, (700, 1007), False),       # a 160 x 161 bank read from global memory; mid-stream, 307 outputs
         None]                                                 # idle


def _single(bank, width, orig, new, buf, s0, o0, n_out, total):
    from dmel_codec_amd import _lib
    y = torch.full((1, n_out), SENTINEL, device=buf.device)
    with torch.cuda.device(buf.device):
        _lib.check(_lib.lib().dmel_resample_window_f32(buf.data_ptr(), buf.shape[1], buf.shape[1], s0, y.data_ptr(), bank.data_ptr(), 1, o0,
                                                       n_out, total, orig, new, width, _lib.stream_ptr()), "resample_window")
    return y[0]


class Launch:
    """five items in one buffer, one arena, one sentinel-filled y; .call() overwrites its host tables right after the entry returns"""

    def __init__(self, dev):
        from dmel_codec_amd.models.stream_schedule import ResampleSchedule
        from dmel_codec_amd.utils.resample import filter_bank
        self.dev, B = dev, len(ITEMS)
        self.rates, banks, off = [], [], 0
        self.want, rows = {}, {}
        self.s0, self.nv, self.o0, self.n_out, self.total, self.rate = ([0] * B for _ in range(6))
        self.total = [-1] * B
        for b, it in enumerate(ITEMS):
            if it is None:
                continue
            of, nf, n, _, (o0, o1), known = it
            bank, width, orig, new = filter_bank(of, nf, dev)
            sc = ResampleSchedule(of, nf)
            assert (sc.down, sc.up, sc.width) == (orig, new, width)
            x = (torch.randn(n, generator=torch.Generator().manual_seed(100 + b)) * 0.3).to(dev)
            o1 = sc.total_outputs(n) if o1 is None else o1
            lo, hi = max(0, sc.first_read(o0)), min(n, sc.first_read(o1 - 1) + sc.kw)
            rows[b] = x[lo:hi]
            self.s0[b], self.nv[b], self.o0[b], self.n_out[b], self.total[b] = lo, hi - lo, o0, o1 - o0, n if known else -1
            self.rate[b] = len(banks)
            self.rates += [off, orig, new, width]
            banks.append(bank.reshape(-1))
            off += bank.numel()
            self.want[b] = _single(bank, width, orig, new, rows[b][None].contiguous(), lo, o0, o1 - o0, self.total[b])
        self.arena = torch.cat(banks).contiguous()
        self.width = max(self.nv) + 5
        self.x = torch.full((B, self.width), float("nan"), device=dev)          # what no item may read is NaN
        for b, r in rows.items():
            self.x[b, :r.shape[0]] = r
        self.y_stride = max(self.n_out) + 40
        self.y_off = [17, 0, 40, 3, 9]
        self.table = torch.empty(7 * B + len(self.rates), dtype=torch.int64, device=dev)

    def call(self, **change):
        from dmel_codec_amd import _lib
        B = len(ITEMS)
        t = {k: list(getattr(self, k)) for k in ("s0", "nv", "o0", "n_out", "total", "rate", "y_off")}
        for k, (b, v) in change.items():
            t[k][b] = v
        I64 = C.c_int64 * B
        host = {k: I64(*v) for k, v in t.items()}
        rates = (C.c_int64 * len(self.rates))(*self.rates)
        y = torch.full((B, self.y_stride), SENTINEL, device=self.dev)
        with torch.cuda.device(self.dev):
            rc = _lib.lib().dmel_resample_window_items_f32(
                self.x.data_ptr(), self.width, self.width, host["s0"], host["nv"], y.data_ptr(), self.y_stride, host["y_off"],
                self.arena.data_ptr(), self.arena.numel(), rates, len(self.rates) // 4, host["rate"], B, host["o0"], host["n_out"],
                host["total"], self.table.data_ptr(), _lib.stream_ptr())
        for arr in list(host.values()) + [rates]:                # the library must not read its host tables after it has returned
            for i in range(len(arr)):
                arr[i] = -1
        msg = _lib.lib().dmel_last_error().decode() if rc else ""
        torch.cuda.synchronize()
        return rc, msg, y


@pytest.fixture(scope="module")
def launch(dev):
    return Launch(dev)


def test_items_launch_equals_single_item_launches(launch):
    n = launch.n_out
    assert n[0] < 256 and n[1] > 512 and n[1] % 256 and n[4] == 0          # whole workgroups of item 0 leave early while item 1 runs
    assert launch.s0[0] == 0 and launch.o0[0] == 0 and launch.s0[1] > 0 and launch.o0[1] % 3 and launch.total[2] == 4000
    assert 80 * 171 <= 15 * 1024 < 160 * 161                                # item 2's bank is staged in LDS, item 3's is not
    rc, _, y = launch.call()
    assert rc == 0
    for b in range(len(ITEMS)):
        a, m = launch.y_off[b], launch.n_out[b]
        if m:
            assert not bool(torch.isnan(launch.want[b]).any()) and float(launch.want[b].abs().max()) > 0
            assert torch.equal(y[b, a:a + m], launch.want[b]), f"item {b}"
        assert bool((y[b, :a] == SENTINEL).all()) and bool((y[b, a + m:] == SENTINEL).all()), f"item {b} wrote outside its outputs"


def test_items_outputs_are_the_whole_clip_bits(launch, dev):
    """the single-item reference is itself the whole-clip conversion: item 2's outputs are the tail of resample() of its clip"""
    from dmel_codec_amd.utils.resample import resample
    x = (torch.randn(4000, generator=torch.Generator().manual_seed(102)) * 0.3).to(dev)
    whole = resample(x[None], 44100, 24000)[0]
    assert torch.equal(whole[1500:], launch.want[2])


def test_items_refusals_leave_y_alone(launch):
    rc, msg, y = launch.call(nv=(1, launch.nv[1] - 1))                     # item 1's last output reads a sample its row does not hold
    assert rc == -1 and "item 1" in msg and "buffer holds" in msg and bool((y == SENTINEL).all())
    rc, msg, y = launch.call(y_off=(3, launch.y_stride - launch.n_out[3] + 1))
    assert rc == -1 and "item 3" in msg and "do not fit" in msg and bool((y == SENTINEL).all())
    from dmel_codec_amd import _lib
    B = len(ITEMS)
    I64 = C.c_int64 * B
    y = torch.full((B, launch.y_stride), SENTINEL, device=launch.dev)
    zeros = I64(*([0] * B))
    with torch.cuda.device(launch.dev):                                    # every item idle: DMEL_OK, nothing launched
        rc = _lib.lib().dmel_resample_window_items_f32(
            launch.x.data_ptr(), launch.width, launch.width, I64(*launch.s0), I64(*launch.nv), y.data_ptr(), launch.y_stride,
            I64(*launch.y_off), launch.arena.data_ptr(), launch.arena.numel(), (C.c_int64 * len(launch.rates))(*launch.rates),
            len(launch.rates) // 4, I64(*launch.rate), B, I64(*launch.o0), zeros, I64(*launch.total), launch.table.data_ptr(),
            _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and bool((y == SENTINEL).all())


# ------------------------------------------------------------------------------------ encode sessions = encode(..., sample_rate=r)
# clip -> (rate, seconds, step of its open(), push sizes in its own samples, steps in which it is not named)
ENC = {"a": (48000, 1.9, 0, [15360, 0, 9, 15360, 11111, 15360], {3}),
       "b": (16000, 1.6, 1, [5120, 3, 5120, 4097], set()),
       "c": (SR, 1.2, 2, [7680, 5000, 1], set()),
       "d": (44100, 1.3, 3, [14112, 100, 14112], set()),
       "e": (16000, 1.1, 12, [5120], set())}                   # opened after a (48 kHz) has closed: it takes over a's slot at another rate
_enc = {}


def _plan(total, start, sizes, idle):
    out, pos, step, i = {}, 0, start, 0
    while pos < total:
        if step not in idle:
            n = min(sizes[i % len(sizes)], total - pos)
            out[step] = (pos, n, pos + n == total)
            pos, i = pos + n, i + 1
        step += 1
    return out


def encode_run(dev):
    if not _enc:
        codec = make_codec(570, n_mels=80, dmel_groups=8, vocoder=None, decoder_layers=1, residual_channels=70).to(dev)
        clips = {k: (torch.randn(int(v[1] * v[0]) + 7, generator=torch.Generator().manual_seed(ord(k))) * 0.2).to(dev) for k, v in ENC.items()}
        ref = {k: codec.encode(c[None], torch.tensor([c.shape[0]], device=dev), sample_rate=ENC[k][0]) for k, c in clips.items()}
        plans = {k: _plan(clips[k].shape[0], *ENC[k][2:]) for k in clips}
        pool = codec.encode_sessions(slots=4, max_push_samples=15360, sample_rates=(48000, 16000, 44100))
        slot, got, closed_at, sizes = {}, {k: [] for k in clips}, {}, []
        for step in range(max(max(p) for p in plans.values()) + 1):
            for k in clips:
                if ENC[k][2] == step:
                    slot[k] = pool.open(sample_rate=ENC[k][0])
            named = {k: plans[k][step] for k in clips if step in plans[k]}
            if not named:
                continue
            audio = {slot[k]: clips[k][pos:pos + n] for k, (pos, n, _) in named.items()}
            ids = pool.push(audio, final=[slot[k] for k, (_, _, fin) in named.items() if fin])
            assert set(ids) == set(audio)
            for k, (_, _, fin) in named.items():
                got[k].append(ids[slot[k]])
                if fin:
                    closed_at[k] = step
            sizes.append(pool.allocated_bytes())
        _enc.update(pool=pool, slot=slot, got=got, ref=ref, closed_at=closed_at, sizes=sizes, plans=plans)
    return _enc


@pytest.mark.parametrize("clip", ["a", "b", "c", "d"])
def test_encode_sessions_equal_encode_at_each_rate(dev, clip):
    """four slots at 48 kHz, 16 kHz, the codec's rate and 44.1 kHz; staggered opens, ragged pushes with 0 samples and fewer samples
    than the filter's width (9 < 13 at 48 kHz, 3 < 6 at 16 kHz, 100 < 159 at 44.1 kHz), an unnamed step"""
    r = encode_run(dev)
    ids, lens = r["ref"][clip]
    mine = torch.cat(r["got"][clip], dim=1)
    assert int(lens[0]) > 20 and mine.dtype == torch.int32
    assert mine.shape[1] == int(lens[0]) and torch.equal(mine, ids[0, :, :int(lens[0])])
    sizes = [n for _, n, _ in r["plans"]["a"].values()]
    assert 0 in sizes and 9 in sizes and 3 not in r["plans"]["a"]


def test_encode_slot_reopened_at_another_rate_and_fixed_memory(dev):
    r = encode_run(dev)
    assert r["slot"]["e"] == r["slot"]["a"] and ENC["e"][2] > r["closed_at"]["a"] and ENC["e"][0] != ENC["a"][0]
    ids, lens = r["ref"]["e"]
    mine = torch.cat(r["got"]["e"], dim=1)
    assert mine.shape[1] == int(lens[0]) > 0 and torch.equal(mine, ids[0, :, :int(lens[0])])
    assert r["pool"].open_slots == []
    assert len(set(r["sizes"])) == 1 and r["sizes"][0] > 0                 # constant from the first push on
    assert r["pool"].rs.allocated_bytes() > 0


# ------------------------------------------------------------------------------------ decode sessions = resample(decode() audio)
@pytest.fixture(scope="module")
def dcodec(dev):
    return make_codec(700, n_mels=80, dmel_groups=8, encoder_layers=2).to(dev)


def _clip(codec, seed, T, dev):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 175, (8, T), generator=g, dtype=torch.int32).to(dev)
    noise = torch.randn(codec.decoder.residual_channels, T * 4, generator=g).to(dev)
    return ids, noise


class Feeder:
    def __init__(self, pool, ids, noise, rate):
        self.slot, self.ids, self.noise, self.rate, self.pos, self.audio, self.mel = pool.open(output_sample_rate=rate), ids, noise, rate, 0, [], []

    def take(self, n):
        a = self.pos
        self.pos += n
        return self.ids[:, a:self.pos], self.noise[:, 4 * a:4 * self.pos]

    def got(self, out):
        audio, mel = out
        assert audio.ndim == 2 and audio.shape[0] == 1 and audio.dtype == torch.float32 and mel.shape[0] == 80
        self.audio.append(audio.clone())                          # a piece must survive the steps that follow
        self.mel.append(mel)

    def check(self, codec):
        from dmel_codec_amd.utils.resample import resample
        assert self.pos == self.ids.shape[1]
        T = self.ids.shape[1]
        audio, mel = codec.decode(self.ids[None], torch.tensor([T], device=self.ids.device), return_audios=True, noise=self.noise[None])
        want = audio[0] if self.rate is None else resample(audio[0], SR, self.rate)
        assert torch.equal(torch.cat(self.mel, dim=1), mel[0])
        mine = torch.cat(self.audio, dim=1)
        assert mine.shape == want.shape and torch.equal(mine, want)


def _step(pool, feeders, plan, final=()):
    ids, noise = {}, {}
    for i, n in plan.items():
        f = feeders[i]
        ids[f.slot], noise[f.slot] = f.take(n)
    out = pool.push(ids, noise=noise, final=[feeders[i].slot for i in final])
    assert set(out) == set(ids)
    for i in plan:
        feeders[i].got(out[feeders[i].slot])


@pytest.mark.parametrize("precision", ["fp32", "fp32_bf16x3"])
def test_decode_sessions_equal_resampled_decode(dev, dcodec, precision):
    """3 slots at 48 kHz, 16 kHz and the vocoder's rate, 4 sessions (one slot reused, at another rate): staggered opens, ragged pushes
    with 0- and 1-token pushes, one session shorter than the lookahead; state bounded."""
    codec = dcodec
    assert int(codec.vocoder.h.get("sampling_rate", SR)) == SR
    codec.set_decode_precision(precision)
    try:
        pool = codec.decode_sessions(3, max_push_tokens=32, output_sample_rates=(48000, 16000))
        lengths, rates = [70, 3, 45, 28], [48000, 16000, None, 48000]
        clips = [_clip(codec, 80 + i, T, dev) for i, T in enumerate(lengths)]
        f = [Feeder(pool, *clips[0], rates[0])]
        _step(pool, f, {0: 27})
        size = pool.allocated_bytes()
        f.append(Feeder(pool, *clips[1], rates[1]))
        _step(pool, f, {0: 1, 1: 2})
        f.append(Feeder(pool, *clips[2], rates[2]))
        _step(pool, f, {0: 32, 1: 1, 2: 30}, final=(1,))                   # session 1 ends after 3 tokens: shorter than the lookahead
        f.append(Feeder(pool, *clips[3], rates[3]))                        # takes over session 1's slot, 16 -> 48 kHz
        assert f[3].slot == f[1].slot
        _step(pool, f, {0: 0, 2: 15, 3: 28})
        _step(pool, f, {0: 10, 2: 0}, final=(2,))
        f[0].got(pool.close(f[0].slot))                                    # closes without tokens: the flush alone
        f[3].got(pool.close(f[3].slot))
        assert pool.open_slots == [] and pool.allocated_bytes() == size and pool.rs.allocated_bytes() > 0
        assert max(pool.rs.fill) == 0
        for s in f:
            s.check(codec)
    finally:
        codec.set_decode_precision("fp32")
