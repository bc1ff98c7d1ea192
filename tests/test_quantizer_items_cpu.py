"""The host side of the one-pass quantiser over windows of different lengths, without a GPU: what
DownsampleFiniteScalarQuantize.encode(z, lengths=) / .decode(ids, lengths=) refuse before they touch the device, pad_windows on token
and feature windows, and a float64 statement of the contract through the oracle: the items form IS the item-alone result, and the plain
call on the right-padded batch differs from it in the last frames of a shorter item -- so the GPU tests are not vacuous."""
import ctypes as C

import pytest
import torch

from oracle import ref_cpu
from dmel_codec_amd.models.stream_sessions import pad_windows

G, CG = 2, 6


@pytest.fixture(scope="module")
def quantizer():
    from dmel_codec_amd.models.modules.dowmsample_fsq import DownsampleFiniteScalarQuantize
    return DownsampleFiniteScalarQuantize(input_dim=G * CG, n_codebooks=1, n_groups=G, levels=[7, 5, 5], downsample_factor=(2, 2),
                                          is_dmel=True)


BAD = [[12], [1, 2, 3], [13, 1], [-1, 4], [1.5, 2], [True, 2], "ab", torch.tensor([[1, 2]]), torch.tensor([1.0, 2.0]),
       torch.tensor([1, 13]), torch.tensor([True, False])]


@pytest.mark.parametrize("bad", BAD, ids=repr)
def test_bad_lengths_are_refused_before_any_device_call(quantizer, bad):
    z = torch.zeros(2 * G, CG, 12)                     # CPU tensors: reaching the device check would raise RuntimeError instead
    with pytest.raises(ValueError, match="lengths"):
        quantizer.encode(z, lengths=bad)
    ids = torch.zeros(2, G, 12, dtype=torch.int32)
    with pytest.raises(ValueError, match="lengths"):
        quantizer.decode(ids, lengths=bad)


def test_good_lengths_reach_the_device_check_and_side_outputs_are_refused(quantizer):
    z = torch.zeros(2 * G, CG, 12)
    ids = torch.zeros(2, G, 12, dtype=torch.int32)
    for good in ([12, 0], (3, 4), torch.tensor([0, 12]), torch.tensor([5, 6], dtype=torch.int32)):
        with pytest.raises(RuntimeError, match="GPU"):  # the lengths passed; the CPU tensor is what is refused (no CPU path)
            quantizer.encode(z, lengths=good)
        with pytest.raises(RuntimeError, match="GPU"):
            quantizer.decode(ids, lengths=good)
    for kw in (dict(return_prequant=True), dict(return_latents=True)):
        with pytest.raises(ValueError, match="return_prequant"):
            quantizer.encode(z, lengths=[12, 12], **kw)
    with pytest.raises(ValueError, match="expected"):
        quantizer.encode(torch.zeros(CG, 12), lengths=[12])
    with pytest.raises(ValueError, match="expected"):
        quantizer.decode(torch.zeros(G, 12, dtype=torch.int32), lengths=[12])


def test_the_new_entry_points_are_bound():
    from dmel_codec_amd import _lib
    for name, nargs in (("dmel_quantizer_encode_items", 9), ("dmel_quantizer_decode_items", 9), ("dmel_quantizer_items_workspace_bytes", 3),
                        ("dmel_convnext_forward_items", 9)):
        res, args = _lib.PROTOTYPES[name]
        assert len(args) == nargs and res is (C.c_size_t if name.endswith("bytes") else C.c_int)
        assert callable(getattr(_lib.lib(), name))
    # a NULL handle sizes nothing, as dmel_quantizer_workspace_bytes
    assert _lib.lib().dmel_quantizer_items_workspace_bytes(None, 4, 64) == 0


def test_pad_windows_on_token_and_feature_windows():
    g = torch.Generator().manual_seed(1)
    toks = [torch.randint(0, 175, (8, w), generator=g, dtype=torch.int32) for w in (9, 1, 4)]
    batch, widths = pad_windows(toks)
    assert widths == [9, 1, 4] and batch.shape == (3, 8, 9) and batch.dtype == torch.int32 and batch.is_contiguous()
    for i, w in enumerate(toks):
        assert torch.equal(batch[i, :, :w.shape[1]], w) and not bool(batch[i, :, w.shape[1]:].any())
    feats = [torch.randn(8, 5, w, generator=g) for w in (11, 12, 3)]                   # (G, C, W): the encode pool's windows
    batch, widths = pad_windows(feats)
    assert widths == [11, 12, 3] and batch.shape == (3, 8, 5, 12) and batch.is_contiguous()
    for i, w in enumerate(feats):
        assert torch.equal(batch[i, ..., :w.shape[-1]], w) and not bool(batch[i, ..., w.shape[-1]:].any())
    rows = batch.view(3 * 8, 5, 12)                                                    # what quantizer.encode takes: item b at rows b*G ..
    assert torch.equal(rows[8:16], feats[1])
    same = [torch.randn(8, 5, 6, generator=g) for _ in range(3)]
    batch, widths = pad_windows(same)                                                  # one length: the plain call, no lengths
    assert widths is None and torch.equal(batch.view(24, 5, 6), torch.cat(same, dim=0)) and batch.is_contiguous()


def oracle_quantizer(seed):
    from dmel_codec_amd.models.modules.dowmsample_fsq import DownsampleFiniteScalarQuantize
    torch.manual_seed(seed)
    q = DownsampleFiniteScalarQuantize(input_dim=G * CG, n_codebooks=1, n_groups=G, levels=[7, 5, 5], downsample_factor=(2, 2),
                                       is_dmel=True)
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in q.state_dict().items():
        scale = 0.5 if k.endswith("gamma") else 1.0 if v.ndim >= 2 else 0.3
        sd[k] = torch.randn(v.shape, generator=gen, dtype=torch.float64) * scale
        if k.endswith("norm.weight"):
            sd[k] = sd[k] + 1.0
    return sd


def decode_items_oracle(sd, ids, lens):
    """the contract, stated in float64: item b is decode() of its own ids alone, zeros behind"""
    out = torch.zeros(ids.shape[0], G * CG, 4 * ids.shape[2], dtype=torch.float64)
    for b, n in enumerate(lens):
        if n:
            out[b, :, :4 * n] = ref_cpu.quantizer_decode(sd, "", ids[b:b + 1, :, :n], G, [7, 5, 5], (2, 2))[0]
    return out


def test_the_contract_in_float64_and_why_the_padded_call_does_not_meet_it():
    sd = oracle_quantizer(3)
    g = torch.Generator().manual_seed(4)
    lens = [9, 1, 2, 0, 7]
    ids = torch.randint(0, 175, (5, G, 9), generator=g, dtype=torch.int32)
    a, b = ids.clone(), ids.clone()
    for i, n in enumerate(lens):
        a[i, :, n:], b[i, :, n:] = 0, 174
    items = decode_items_oracle(sd, a, lens)
    assert torch.equal(items, decode_items_oracle(sd, b, lens))                        # by construction: the padding is not an input
    pa = ref_cpu.quantizer_decode(sd, "", a, G, [7, 5, 5], (2, 2))
    pb = ref_cpu.quantizer_decode(sd, "", b, G, [7, 5, 5], (2, 2))
    same = lambda x, y: torch.allclose(x, y, rtol=1e-12, atol=1e-13)                   # float64: a call over another batch shape may round differently
    assert same(pa[0], items[0])                                                       # the longest item has no padding behind it
    for i in (1, 2, 4):
        n = 4 * lens[i]
        # the depthwise k = 7 convolutions reach 3 columns across the end at the token rate x2 and 3 at the feature rate: the last
        # 3 * 2 + 3 = 9 frames of a shorter item depend on what stands behind it, the frames in front of them do not
        for padded in (pa, pb):
            assert same(padded[i, :, :max(n - 9, 0)], items[i, :, :max(n - 9, 0)])
            assert not torch.allclose(padded[i, :, max(n - 9, 0):n], items[i, :, max(n - 9, 0):n], rtol=1e-6, atol=1e-9), i
        assert not torch.allclose(pa[i, :, max(n - 9, 0):n], pb[i, :, max(n - 9, 0):n], rtol=1e-6, atol=1e-9)


def test_encode_floors_in_float64():
    """feature lengths 7, 5, 3 give 1, 1, 0 tokens (7 -> 3 -> 1, 5 -> 2 -> 1, 3 -> 1 -> 0), and the ids of an item do not move when
    frames that its floors drop are appended"""
    sd = oracle_quantizer(8)
    g = torch.Generator().manual_seed(9)
    z = torch.randn(G, CG, 7, generator=g, dtype=torch.float64)
    for n in (7, 5, 4):
        ids = ref_cpu.quantizer_encode(sd, "", z[:, :, :n], G, [7, 5, 5], (2, 2))
        assert ids.shape == (1, G, n // 4) == (1, G, 1)
    with pytest.raises(RuntimeError):
        ref_cpu.quantizer_encode(sd, "", z[:, :, :3], G, [7, 5, 5], (2, 2))            # no token: the items form writes zeros instead
    assert torch.equal(ref_cpu.quantizer_encode(sd, "", z[:, :, :7], G, [7, 5, 5], (2, 2)),
                       ref_cpu.quantizer_encode(sd, "", z[:, :, :6], G, [7, 5, 5], (2, 2)))
