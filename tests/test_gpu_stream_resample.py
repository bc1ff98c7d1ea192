"""Streaming at the sound card's sample rate: the window resampling launch is held to the BITS of the whole-clip launch, StreamResampler
to resample(), streaming encode from 48 / 16 / 44.1 kHz to encode(..., sample_rate=...), and streaming decode to 48 kHz to the resampled
decode() audio.  (Float parity of resample() itself against the oracle is test_gpu_fullsize's.)"""
import pytest
import torch

from test_gpu_parity import make_codec

pytestmark = pytest.mark.gpu

PAIRS = [(48000, 24000), (16000, 24000), (44100, 24000), (24000, 48000)]
RAGGED = [0, 7, 1, 300, 0, 4097]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


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


_clips = {}


def clip_and_reference(dev, orig, new, L=2037):
    """random (2, L) audio and resample() of the whole rows, computed once per rate pair"""
    from dmel_codec_amd.utils.resample import resample
    if (orig, new, L) not in _clips:
        x = (torch.randn(2, L, generator=torch.Generator().manual_seed(orig // 100 + L)) * 0.3).to(dev)
        _clips[(orig, new, L)] = (x, resample(x, orig, new))
    return _clips[(orig, new, L)]


# ------------------------------------------------------------------------------------ 5. window launch = whole-clip launch
@pytest.mark.parametrize("orig,new", PAIRS)
def test_window_kernel_equals_whole_clip(dev, orig, new):
    from dmel_codec_amd import _lib
    from dmel_codec_amd.models.stream_schedule import ResampleSchedule
    from dmel_codec_amd.utils.resample import filter_bank
    L = 2000 + 37
    x, whole = clip_and_reference(dev, orig, new, L)
    sc = ResampleSchedule(orig, new)
    down, up, w = sc.down, sc.up, sc.width
    Lout = sc.total_outputs(L)
    assert whole.shape == (2, Lout)
    bank, width, o, n = filter_bank(orig, new, dev)
    assert (width, o, n) == (w, down, up)

    def reads(o0, o1):             # input samples the outputs [o0, o1) read inside the signal
        return max(0, (o0 // up) * down - w), min(L, ((o1 - 1) // up) * down + w + down)

    def window(o0, o1, s0, s1, total):
        return torch.ops.dmel_hip.resample_window(x[:, s0:s1], bank, down, up, w, s0, o0, o1 - o0, total)

    # head: the zero padding in front of the signal, the end not known yet; 300 outputs straddle the first 256-output block boundary
    lo, hi = reads(0, 300)
    assert lo == 0
    assert torch.equal(window(0, 300, 0, hi, -1), whole[:, :300])
    # interior windows: o0 and n_out no multiples of `up` nor of 256, cut so that 256-output blocks of the launch straddle the whole
    # clip's own block boundaries; the buffer starts mid-signal exactly at the first sample read; length unknown, then known
    def cut(o0, n_out):
        while up > 1 and o0 % up == 0:
            o0 += 1
        while n_out % 256 == 0 or (up > 1 and n_out % up == 0):
            n_out += 1
        return o0, o0 + n_out

    cuts = [cut(258, 522), cut(511, 259), cut(Lout // 2 + 3, 301)]
    for o0, o1 in cuts:
        assert o1 <= Lout and (o1 - o0) % 256 and o0 // 256 != (o1 - 1) // 256 and (up == 1 or (o0 % up and (o1 - o0) % up))
        lo, hi = reads(o0, o1)
        if hi < L and lo > 0:
            for total in (-1, L):
                assert torch.equal(window(o0, o1, lo, hi, total), whole[:, o0:o1]), (o0, o1, total)
            # slack on both sides of the buffer
            assert torch.equal(window(o0, o1, max(0, lo - 17), min(L, hi + 5), -1), whole[:, o0:o1])
        else:
            assert torch.equal(window(o0, o1, lo, L, L), whole[:, o0:o1]), (o0, o1)
    # tail: the zero padding behind the end, known at the last window only
    o0 = Lout - 263
    lo, hi = reads(o0, Lout)
    assert lo > 0 and hi == L
    assert torch.equal(window(o0, Lout, lo, L, L), whole[:, o0:])
    # the windows tile the clip: every output, each from a buffer that starts at s0 > 0 where it can
    pieces, o0 = [], 0
    for n_out in chunks_of(Lout, [100, 257, 1, 511, 300]):
        lo, hi = reads(o0, o0 + n_out)
        known = o0 + n_out == Lout or hi == L
        pieces.append(window(o0, o0 + n_out, lo, L if known else hi, L if known else -1))
        o0 += n_out
    assert torch.equal(torch.cat(pieces, dim=1), whole)
    # a window whose taps are not covered is refused by the host check: an error code, nothing launched, y untouched
    o0, o1 = cuts[1]
    lo, hi = reads(o0, o1)
    assert lo > 0 and hi < L
    y = torch.full((2, o1 - o0), 7.0, device=dev)
    for s0, s1, total in ((lo + 1, hi, -1), (lo, hi - 1, -1), (lo, hi - 1, L)):
        buf = x[:, s0:s1].contiguous()
        with torch.cuda.device(dev):
            rc = _lib.lib().dmel_resample_window_f32(buf.data_ptr(), buf.stride(0), s1 - s0, s0, y.data_ptr(), bank.data_ptr(), 2, o0, o1 - o0,
                                                     total, down, up, w, _lib.stream_ptr())
        assert rc == -1 and b"buffer holds" in _lib.lib().dmel_last_error()
        torch.cuda.synchronize()
        assert bool((y == 7.0).all())
        with pytest.raises(RuntimeError, match="buffer holds"):
            window(o0, o1, s0, s1, total)
    # outputs behind the whole clip's last one, and a buffer that runs past the stated end
    with pytest.raises(RuntimeError, match="outputs past"):
        window(Lout - 10, Lout + 1, reads(Lout - 10, Lout)[0], L, L)
    with pytest.raises(RuntimeError, match="past the end"):
        window(o0, o1, lo, hi, hi - 1)


# ------------------------------------------------------------------------------------ 6. StreamResampler = resample()
@pytest.mark.parametrize("orig,new", PAIRS)
def test_stream_resampler_equals_resample(dev, orig, new):
    from dmel_codec_amd.utils.resample import StreamResampler, resample
    x, whole = clip_and_reference(dev, orig, new, 5000 + 37)
    L = x.shape[1]
    short, short_whole = clip_and_reference(dev, orig, new, 600)
    for clip, want, pattern, final_push in ((short, short_whole, [1], False), (x, whole, RAGGED, False), (x, whole, [L], True),
                                            (x, whole, [L], False)):
        rs = StreamResampler(orig, new, 2)
        pieces, pos = [], 0
        sizes = chunks_of(clip.shape[1], pattern)
        for i, n in enumerate(sizes):
            last = final_push and i == len(sizes) - 1
            y = rs.push(clip[:, pos:pos + n], final=last)
            pos += n
            assert y.dtype == torch.float32 and y.shape[0] == 2
            assert last or (y.shape[1] % rs.sched.up == 0 and rs.sched.emitted == rs.sched.outputs_ready(pos))
            assert rs.fill < rs.sched.max_tail or last
            pieces.append(y)
        if not final_push:
            pieces.append(rs.finish())
        assert torch.equal(torch.cat(pieces, dim=1), want), (pattern[:3], final_push)
        with pytest.raises(RuntimeError, match="finished"):
            rs.push(clip[:, :3])
    # constant capacity after the second push of a steady stream
    rs = StreamResampler(orig, new, 1)
    n = int(0.32 * orig)
    g = torch.Generator().manual_seed(3)
    cap2 = None
    for i in range(12):
        rs.push((torch.randn(1, n, generator=g) * 0.1).to(dev))
        if i == 1:
            cap2 = rs.capacity
    assert cap2 is not None and rs.capacity == cap2 and rs.s0 > 0
    # equal rates: the chunks pass through untouched
    same = StreamResampler(new, new, 2)
    piece = x[:, :100]
    assert same.push(piece) is piece and same.finish().shape == (2, 0)
    assert resample(piece, new, new) is piece


# ------------------------------------------------------------------------------------ 7. / 8. streaming encode from another rate
CODEC_SR, HOP = 24000, 256
_codecs = {}


def codec_of(dev, n_mels, G):
    if (n_mels, G) not in _codecs:
        _codecs[(n_mels, G)] = make_codec(300 + G, n_mels=n_mels, dmel_groups=G, vocoder=None, decoder_layers=1).to(dev)
    return _codecs[(n_mels, G)]


_sources = {}


def source_and_reference(dev, n_mels, G, sr):
    """a 2.6 s + 37 samples source clip at `sr`, ragged lengths, and encode(..., sample_rate=sr) of it -- once per (codec, rate)"""
    if (n_mels, G, sr) not in _sources:
        codec = codec_of(dev, n_mels, G)
        clip = int(2.6 * sr) + 37
        audio = (torch.randn(2, clip, generator=torch.Generator().manual_seed(G + sr // 1000)) * 0.2).to(dev)
        lens = torch.tensor([clip, int(1.7 * sr) + 11], device=dev)
        _sources[(n_mels, G, sr)] = (audio, lens, codec.encode(audio, lens, sample_rate=sr))
    return _sources[(n_mels, G, sr)]


def run_stream_encode(codec, G, sr, audio, lens, pattern, final_push):
    enc = codec.streaming_encoder(2, lens, sample_rate=sr)
    assert enc.geo.lookahead_samples == 25216                                  # unchanged at the codec's rate
    assert enc.lookahead_source_samples == enc.resampler.sched.samples_needed(25216) == enc.token_ready_source_samples(0)
    # ... which is the same time at the source rate plus at most the filter's right context
    exact = 25216 * sr / CODEC_SR
    assert exact <= enc.lookahead_source_samples <= exact + enc.resampler.sched.width + enc.resampler.sched.down
    pieces, pos = [], 0
    sizes = chunks_of(audio.shape[1], pattern)
    for i, n in enumerate(sizes):
        last = final_push and i == len(sizes) - 1
        piece = audio[:, None, pos:pos + n] if i % 2 else audio[:, pos:pos + n]
        ids = enc.push(piece, final=last)
        pos += n
        assert ids.dtype == torch.int32 and ids.shape[:2] == (2, G)
        pieces.append(ids)
        # the emission bound of the lookahead, in source samples: token j is out once token_ready_source_samples(j) samples are in
        promised = 0
        while enc.token_ready_source_samples(promised) <= pos:
            promised += 1
        assert enc.tokens_emitted >= promised, (i, pos, enc.tokens_emitted, promised)
        assert last or enc.tokens_emitted == promised
    if not final_push:
        pieces.append(enc.finish())
    return torch.cat(pieces, dim=2), enc


def check_ids(ids, enc, lens, want, want_len, what):
    assert ids.shape == want.shape, what
    assert torch.equal(enc.indices_lengths_for(lens), want_len)
    for b in range(2):
        n = int(want_len[b])
        assert torch.equal(ids[b, :, :n], want[b, :, :n]), (what, b)


@pytest.mark.parametrize("sr", [48000, 16000])
@pytest.mark.parametrize("n_mels,G", [(80, 8), (100, 10)])
def test_encode_stream_from_another_rate_equals_encode(dev, n_mels, G, sr):
    codec = codec_of(dev, n_mels, G)
    audio, lens, (want, want_len) = source_and_reference(dev, n_mels, G, sr)
    clip = audio.shape[1]
    ragged = [100, 0, 1, 3001, int(0.32 * sr), 0, 12345, HOP * sr // CODEC_SR - 1, 257, 20000]
    for pattern, final_push in (([int(0.32 * sr)], False), (ragged, False), ([clip], True)):
        ids, enc = run_stream_encode(codec, G, sr, audio, lens, pattern, final_push)
        check_ids(ids, enc, lens, want, want_len, (sr, pattern[:3]))
    # the generator form
    got = torch.cat(list(codec.encode_stream(audio, lens, chunk_samples=int(0.32 * sr), sample_rate=sr)), dim=2)
    assert torch.equal(got[0], want[0])


def test_encode_stream_from_44100(dev):
    codec = codec_of(dev, 80, 8)
    audio, lens, (want, want_len) = source_and_reference(dev, 80, 8, 44100)
    ids, enc = run_stream_encode(codec, 8, 44100, audio, lens, [int(0.32 * 44100)], False)
    check_ids(ids, enc, lens, want, want_len, 44100)


def test_encode_with_sample_rate_is_resample_then_encode(dev):
    from dmel_codec_amd.utils.resample import resample
    codec = codec_of(dev, 80, 8)
    sr = 16000
    audio, lens, (ids, ids_len) = source_and_reference(dev, 80, 8, sr)
    by_hand = codec.encode(resample(audio, sr, CODEC_SR), (lens * CODEC_SR + sr - 1) // sr)
    assert torch.equal(ids, by_hand[0]) and torch.equal(ids_len, by_hand[1])
    assert int(ids_len[0]) > int(ids_len[1]) > 0                               # ragged, and the lengths were converted
    assert int(ids_len[1]) == ((int(lens[1]) * 3 + 1) // 2) // HOP // 4
    # the (B, 1, L) layout and the codec's own rate given explicitly
    assert torch.equal(codec.encode(audio[:, None], lens, sample_rate=sr)[0], ids)
    a24 = resample(audio, sr, CODEC_SR)
    assert torch.equal(codec.encode(a24, (lens * 3 + 1) // 2, sample_rate=CODEC_SR)[0], ids)


# ------------------------------------------------------------------------------------ 9. streaming decode to another rate
TINY_VOCODER = dict(num_mels=80, upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], upsample_initial_channel=64, resblock="1",
                    resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3, activation="snakebeta", snake_logscale=True)


@pytest.fixture(scope="module")
def decode_case(dev):
    from dmel_codec_amd.utils.resample import resample
    codec = make_codec(730, n_mels=80, dmel_groups=8, encoder_layers=2, decoder_layers=1, vocoder=TINY_VOCODER).to(dev)
    g = torch.Generator().manual_seed(19)
    B, T4 = 2, 150
    ids = torch.randint(0, 175, (B, 8, T4), generator=g, dtype=torch.int32).to(dev)
    flen = torch.tensor([T4, 101], device=dev)
    noise = torch.randn(B, codec.decoder.input_channels, T4 * 4, generator=g).to(dev)
    audio, mel = codec.decode(ids, flen, return_audios=True, noise=noise)
    return codec, ids, flen, noise, audio, mel, resample(audio, 24000, 48000)


@pytest.mark.parametrize("pipeline", [False, True])
@pytest.mark.parametrize("pattern", ["64", "ragged"])
def test_decode_stream_to_another_rate(dev, decode_case, pattern, pipeline):
    codec, ids, flen, noise, audio, mel, want = decode_case
    B, T4 = ids.shape[0], ids.shape[2]
    up = audio.shape[-1] // mel.shape[-1]
    assert want.shape == (B, 1, 2 * audio.shape[-1])
    sizes = [64, 64, 22] if pattern == "64" else [1, 7, 30, 70, 3, 39]
    assert sum(sizes) == T4
    dec = codec.streaming_decoder(B, flen, return_audios=True, overlap_vocoder=pipeline, output_sample_rate=48000)
    wavs, mels, pos = [], [], 0
    for n in sizes:
        a, m = dec.push(ids[:, :, pos:pos + n], noise=noise[:, :, pos * 4:(pos + n) * 4])
        ev = dec.audio_event
        pos += n
        a = dec.wait_audio(a, ev) if pipeline else a
        assert a.shape[:2] == (B, 1) and a.shape[-1] % 2 == 0 and a.shape[-1] <= 2 * up * m.shape[-1]
        wavs.append(a); mels.append(m)
    a, m = dec.finish()
    wavs.append(dec.wait_audio(a) if pipeline else a); mels.append(m)
    assert torch.equal(torch.cat(mels, dim=-1), mel)                           # the mel pieces are unchanged
    assert torch.equal(torch.cat(wavs, dim=-1), want)
    # the generator form
    got = list(codec.decode_stream(ids, flen, chunk_tokens=64, noise=noise, pipeline=pipeline, output_sample_rate=48000))
    assert torch.equal(torch.cat([p[0] for p in got], dim=-1), want) and torch.equal(torch.cat([p[1] for p in got], dim=-1), mel)


def test_decode_stream_output_rate_arguments(dev, decode_case):
    codec, ids, flen, noise, audio, mel, want = decode_case
    with pytest.raises(ValueError, match="exclude"):
        codec.streaming_decoder(2, None, True, graph_chunk_tokens=32, output_sample_rate=48000)
    # the vocoder's own rate given explicitly is today's path: no resampler, the decode() bits
    dec = codec.streaming_decoder(2, flen, True, output_sample_rate=24000)
    assert dec._rs is None
    a0, _ = dec.push(ids, noise=noise)
    a1, _ = dec.finish()
    assert torch.equal(torch.cat([a0, a1], dim=-1), audio)
