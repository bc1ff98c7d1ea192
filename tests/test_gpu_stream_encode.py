"""Streaming encode on the GPU: every piece is held to the BITS of the whole-clip path it replaces -- the window STFT to the whole-clip
STFT, the layered incremental WaveNet step (with input projection) to the whole-sequence forward, the one-launch step to the layered
step, and encode_stream() to encode()."""
import ctypes as C

import pytest
import torch

from test_gpu_parity import make_codec, randomise

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------ 1. window STFT = whole-clip STFT
@pytest.mark.parametrize("n_fft", [512, 1024])
def test_window_stft_equals_whole_clip(dev, n_fft):
    from dmel_codec_amd.utils.spectrogram import LinearSpectrogram
    hop, Ls = n_fft // 4, 6000
    pad = (n_fft - hop) // 2
    spec = LinearSpectrogram(n_fft=n_fft, win_length=n_fft, hop_length=hop, num_mels=80, sample_rate=24000)
    g = torch.Generator().manual_seed(n_fft)
    y = (torch.randn(2, Ls, generator=g) * 0.3).to(dev)
    lengths = torch.tensor([Ls, 4100], device=dev)
    whole = spec(y, lengths=lengths)
    T = Ls // hop
    assert whole.shape == (2, 80, T)

    def window(f0, f1, s0, s1, total):
        return spec.forward_window(y[:, s0:s1].contiguous(), s0, f0, f1 - f0, total, lengths)

    def need(f0, f1):              # samples the frames [f0, f1) read when no reflection is involved
        return max(0, f0 * hop - pad), (f1 - 1) * hop - pad + n_fft

    # head: left reflection, the end of the signal not known yet
    lo, hi = need(0, 5)
    assert torch.equal(window(0, 5, 0, hi, -1), whole[:, :, 0:5])
    # interior: the buffer starts mid-signal, exactly at the first sample the first frame reads; length unknown, then known
    f0, f1 = 6, 6 + 7
    lo, hi = need(f0, f1)
    assert lo > 0 and hi < Ls
    for total in (-1, Ls):
        assert torch.equal(window(f0, f1, lo, hi, total), whole[:, :, f0:f1])
    # ... without lengths (nothing is masked) ...
    plain = spec(y)
    assert torch.equal(spec.forward_window(y[:, lo:hi].contiguous(), lo, f0, f1 - f0, -1), plain[:, :, f0:f1])
    # ... and with slack on both sides of the buffer
    assert torch.equal(window(f0, f1, lo - 17, hi + 5, -1), whole[:, :, f0:f1])
    # tail: right reflection; item 1's frames lie behind its length and are masked, as in the whole clip
    lo, _ = need(T - 4, T)
    out = window(T - 4, T, lo, Ls, Ls)
    assert torch.equal(out, whole[:, :, T - 4:T])
    assert float(out[1].abs().max()) == 0.0 and float(out[0].abs().min()) > 0.0
    # a window that spans the mask boundary of item 1
    fb = 4100 // hop
    lo, hi = need(fb - 2, fb + 2)
    assert torch.equal(window(fb - 2, fb + 2, lo, hi, -1), whole[:, :, fb - 2:fb + 2])
    # a buffer that misses a sample the frames read is refused, not read out of bounds
    lo, hi = need(f0, f1)
    with pytest.raises(RuntimeError, match="buffer holds"):
        window(f0, f1, lo + 1, hi, -1)
    with pytest.raises(RuntimeError, match="buffer holds"):
        window(f0, f1, lo, hi - 1, -1)


# ------------------------------------------------------------------------------------ 2. / 3. incremental WaveNet steps
def make_encoder(C_res, seed, dev, layers=20):
    from dmel_codec_amd.models.modules.wavenet import WaveNet
    torch.manual_seed(seed)
    m = WaveNet(input_channels=10, residual_channels=C_res, residual_layers=layers, dilation_cycle=4)
    randomise(m, seed)
    return m.to(dev)


class StepDriver:
    """One set of absolute-time buffers for dmel_wavenet_stream_step_ex, with the re-basing the streaming encoder does."""

    def __init__(self, m, x, cap, lengths, group_repeat):
        self.m, self.cap, self.G = m, cap, group_repeat
        self.N, self.Cin, _ = x.shape
        self.L, self.C = len(m.residual_layers), m.residual_channels
        dev = x.device
        self.x_abs = x
        self.lengths = lengths
        self.origin = 0
        self.x = torch.zeros(self.N, self.Cin, cap, device=dev)
        self.hist = torch.zeros(self.L + 1, self.N, self.C, cap, device=dev)
        self.skip = torch.zeros(self.N, self.C, cap, device=dev)
        self.y = torch.zeros(self.N, self.C, cap, device=dev)
        self.scratch = torch.empty(2 * self.N * self.C * cap + 2 * self.N, device=dev)
        self.prev = [0] * (self.L + 1)
        self.dils = [2 ** (i % 4) for i in range(self.L)]

    def frontiers(self, upto, final):
        nxt = [upto]
        for l, d in enumerate(self.dils):
            nxt.append(upto if final else max(self.prev[l + 1], nxt[-1] - d))
        return nxt

    def rebase(self):
        """drop every column the next steps cannot read: the last level's window reaches back max-dilation columns"""
        new_origin = max(0, self.prev[self.L] - 8)
        shift = new_origin - self.origin
        if shift > 0:
            for t in (self.x, self.hist, self.skip, self.y):
                t[..., :self.cap - shift] = t[..., shift:].clone()
                t[..., self.cap - shift:] = 0
            self.origin = new_origin

    def step(self, upto, final=False):
        from dmel_codec_amd import _lib
        o = self.origin
        nxt = self.frontiers(upto, final)
        assert upto - o <= self.cap
        self.x[:, :, self.prev[0] - o:upto - o] = self.x_abs[:, :, self.prev[0]:upto]
        prev = (C.c_int64 * (self.L + 1))(*[p - o for p in self.prev])
        new = (C.c_int64 * (self.L + 1))(*[p - o for p in nxt])
        ol = (self.lengths - o).clamp(min=0).contiguous() if self.lengths is not None else None
        with torch.cuda.device(self.x.device):
            h = self.m.native()
            _lib.check(_lib.lib().dmel_wavenet_stream_step_ex(h, self.x.data_ptr(), self.hist.data_ptr(), self.skip.data_ptr(), None,
                                                              self.y.data_ptr(), self.scratch.data_ptr(), self.N, self.cap, prev, new,
                                                              _lib.ptr(ol), self.G, o, _lib.stream_ptr()), "wavenet_stream_step_ex")
        out = (self.prev[self.L], nxt[self.L])
        self.prev = nxt
        return out


def test_layered_step_with_input_projection_equals_whole_forward(dev, monkeypatch):
    """10 -> 70 channels, 20 blocks: the layered incremental step (forced) over ragged steps against dmel_wavenet_forward on the whole
    input (itself layered at T > 96), with group_repeat and an item shorter than T."""
    N, T = 4, 230
    m = make_encoder(70, 11, dev)
    x = torch.randn(N, 10, T, generator=torch.Generator().manual_seed(5)).to(dev)
    lengths = torch.tensor([T, 181], device=dev)
    with torch.no_grad():              # the inference path: dmel_wavenet_forward
        whole = m(x, out_lengths=lengths, group_repeat=2)
    assert float(whole[2:, :, 181:].abs().max()) == 0.0 and float(whole[2:, :, :181].abs().min()) > 0.0
    monkeypatch.setenv("DMEL_WAVENET_STREAM_FUSED", "0")
    d = StepDriver(m, x, 256, lengths, 2)
    got = 0
    for upto in (40, 41, 100, 103, 190):
        a, b = d.step(upto)
        assert a == got
        got = b
    assert 0 < got < T
    a, b = d.step(T, final=True)
    assert (a, b) == (got, T)
    assert torch.equal(d.y[:, :, :T], whole)
    # the old entry point still refuses a stack with an input projection
    from dmel_codec_amd import _lib
    z = (C.c_int64 * 21)()
    rc = _lib.lib().dmel_wavenet_stream_step(m.native(), d.hist.data_ptr(), d.skip.data_ptr(), None, d.y.data_ptr(), d.scratch.data_ptr(),
                                             N, 256, z, z, None)
    assert rc == -2


@pytest.mark.parametrize("C_res", [70, 64, 48])        # five, four and three 16-channel chunks: every instantiation of the kernel
def test_one_launch_step_equals_layered_step_bit_for_bit(dev, monkeypatch, C_res):
    """Same handle, same (prev, next) sequence, two buffer sets: after every step all L + 1 history levels, the skip buffer and y are
    equal.  New columns per step 96, 95, 33, 200 (cut into sub-steps), 32, 31, 1, then the final step; the buffers are re-based after
    the fourth step so that the later windows start inside dropped history (origin > 0); the first step has the left padding at frame 0."""
    N, T, cap = 4, 500, 512
    m = make_encoder(C_res, 20 + C_res, dev)
    x = torch.randn(N, 10, T, generator=torch.Generator().manual_seed(C_res)).to(dev)
    lengths = torch.tensor([T, 333], device=dev)
    one, lay = StepDriver(m, x, cap, lengths, 2), StepDriver(m, x, cap, lengths, 2)
    upto, steps = 0, []
    for n in (96, 95, 33, 200, 32, 31, 1):
        upto += n
        steps.append((upto, False))
    steps.append((T, True))
    for i, (upto, final) in enumerate(steps):
        monkeypatch.setenv("DMEL_WAVENET_STREAM_FUSED", "0")
        r0 = lay.step(upto, final)
        monkeypatch.delenv("DMEL_WAVENET_STREAM_FUSED")
        r1 = one.step(upto, final)
        assert r0 == r1
        assert torch.equal(one.hist, lay.hist), (i, [l for l in range(21) if not torch.equal(one.hist[l], lay.hist[l])])
        assert torch.equal(one.skip, lay.skip), i
        assert torch.equal(one.y, lay.y), i
        if i == 3:
            one.rebase()
            lay.rebase()
            assert one.origin == lay.origin > 0
    o = one.origin
    with torch.no_grad():              # the inference path: dmel_wavenet_forward
        whole = m(x, out_lengths=lengths, group_repeat=2)
    assert torch.equal(one.y[:, :, :T - o], whole[:, :, o:])
    # a step whose window would reach in front of a re-based buffer is refused
    bad = StepDriver(m, x, cap, lengths, 2)
    bad.origin, bad.prev = 100, [100] * 21
    bad.x_abs = torch.cat([torch.zeros(N, 10, 100, device=dev), x], dim=2)
    with pytest.raises(RuntimeError, match="history in front of the buffer"):
        bad.step(140)


# ------------------------------------------------------------------------------------ 4. encode_stream = encode()
SR, HOP = 24000, 256
CLIP = int(2.6 * SR) + 37          # 62437 samples: no multiple of 4 * hop, nor of the hop
_codecs = {}


def codec_and_reference(dev, n_mels, G):
    if (n_mels, G) not in _codecs:
        codec = make_codec(300 + G, n_mels=n_mels, dmel_groups=G, vocoder=None, decoder_layers=1).to(dev)
        audio = (torch.randn(2, CLIP, generator=torch.Generator().manual_seed(G)) * 0.2).to(dev)
        lens = torch.tensor([CLIP, 41000], device=dev)
        ref = {"ragged": codec.encode(audio, lens), "full": codec.encode(audio, torch.tensor([CLIP, CLIP], device=dev)),
               "short": codec.encode(audio[:, :9600], torch.tensor([9600, 9600], device=dev))}
        _codecs[(n_mels, G)] = (codec, audio, lens, ref)
    return _codecs[(n_mels, G)]


def chunks_of(total, pattern):
    out, left = [], total
    for n in pattern:
        n = min(n, left)
        out.append(n)
        left -= n
    while left:
        n = min(left, pattern[-1])
        out.append(n)
        left -= n
    return out


@pytest.mark.parametrize("layered", [False, True])
@pytest.mark.parametrize("n_mels,G", [(80, 8), (100, 10)])
def test_encode_stream_equals_encode(dev, monkeypatch, n_mels, G, layered):
    codec, audio, lens, ref = codec_and_reference(dev, n_mels, G)
    if layered:
        monkeypatch.setenv("DMEL_WAVENET_STREAM_FUSED", "0")
    geo = codec.streaming_encoder(2).geo
    assert geo.lookahead_samples == 25216

    def run(clip, lengths, pattern, final_push=False):
        enc = codec.streaming_encoder(clip.shape[0], lengths)
        pieces, pos = [], 0
        sizes = chunks_of(clip.shape[1], pattern)
        for i, n in enumerate(sizes):
            last = final_push and i == len(sizes) - 1
            piece = clip[:, None, pos:pos + n] if i % 2 else clip[:, pos:pos + n]          # both accepted layouts
            ids = enc.push(piece, final=last)
            pos += n
            assert ids.dtype == torch.int32 and ids.shape[:2] == (clip.shape[0], G)
            pieces.append(ids)
            # the emission bound of the documented lookahead
            promised = (pos - geo.lookahead_samples) // (4 * HOP) + 1 if pos >= geo.lookahead_samples else 0
            assert enc.tokens_emitted >= promised, (i, pos, enc.tokens_emitted, promised)
            assert last or enc.tokens_emitted == promised
        if not final_push:
            pieces.append(enc.finish())
        with pytest.raises(RuntimeError, match="finished"):
            enc.push(clip[:, :10])
        return torch.cat(pieces, dim=2), pieces

    ragged = [100, 0, 1, 3001, 7680, 0, 12345, 255, 257, 20000]
    for pattern, final_push in (([7680], False), (ragged, False), ([CLIP], True)):
        ids, _ = run(audio, lens, pattern, final_push)
        want, want_len = ref["ragged"]
        assert ids.shape == want.shape
        for b in range(2):
            assert torch.equal(ids[b, :, :int(want_len[b])], want[b, :, :int(want_len[b])]), (pattern[:3], b)
        enc = codec.streaming_encoder(2, lens)
        assert torch.equal(enc.indices_lengths_for(lens), want_len)
        ids, _ = run(audio, None, pattern, final_push)
        assert torch.equal(ids, ref["full"][0]), pattern[:3]
    # a clip shorter than the lookahead: nothing before finish(), everything with it
    ids, pieces = run(audio[:, :9600], None, [4000], False)
    assert all(p.shape[2] == 0 for p in pieces[:-1]) and torch.equal(ids, ref["short"][0])
    # the generator form, tensor and iterable input
    got = torch.cat(list(codec.encode_stream(audio, lens, chunk_samples=7680)), dim=2)
    assert torch.equal(got[0], ref["ragged"][0][0])
    got = torch.cat(list(codec.encode_stream(iter([audio[:, :30001], audio[:, 30001:]]))), dim=2)
    assert torch.equal(got, ref["full"][0])


# ------------------------------------------------------------------------------------ 5. bounded state
def test_state_is_bounded_by_the_chunk_not_the_stream(dev):
    codec, _, _, _ = codec_and_reference(dev, 80, 8)
    enc = codec.streaming_encoder(1)
    g = torch.Generator().manual_seed(9)
    cap2 = tail2 = None
    total = 0
    for i in range(63):                                   # 20 s in 0.32 s pushes
        total += enc.push((torch.randn(1, 7680, generator=g) * 0.1).to(dev)).shape[2]
        if i == 6:                                        # the 2nd second is in
            cap2, tail2 = enc.capacity, enc.samples.shape[1]
    assert cap2 is not None and enc.capacity == cap2 and enc.samples.shape[1] <= tail2 + HOP
    assert enc.origin > 0
    total += enc.finish().shape[2]
    assert total == 63 * 7680 // HOP // 4
