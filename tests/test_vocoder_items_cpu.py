"""The host side of the one-pass vocoder over windows of different lengths, without a GPU: what BigVGAN.forward(x, lengths) refuses
before it touches the device, and the padding / cropping arithmetic of DecodeSessions' single vocoder call (stream_sessions.pad_windows
+ DecodeSchedule's windows) with a stub vocoder whose output at a window's edge depends on where the window ends."""
import random

import pytest
import torch

from dmel_codec_amd.models.stream_schedule import DecodeGeometry, DecodeSchedule
from dmel_codec_amd.models.stream_sessions import pad_windows

UP = 8
TINY = dict(num_mels=80, upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], upsample_initial_channel=32, resblock="1",
            resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1, 3, 5]], activation="snakebeta", snake_logscale=True)


@pytest.fixture(scope="module")
def vocoder():
    from dmel_codec_amd.models.modules.bigvgan.bigvgan import BigVGAN
    from dmel_codec_amd.models.modules.bigvgan.env import AttrDict
    return BigVGAN(AttrDict(dict(TINY)))


@pytest.mark.parametrize("bad", [[12], [1, 2, 3], [13, 1], [-1, 4], [1.5, 2], [True, 2], "ab", torch.tensor([[1, 2]]), torch.tensor([1.0, 2.0]),
                                 torch.tensor([1, 13]), torch.tensor([True, False])], ids=repr)
def test_bad_lengths_are_refused_before_any_device_call(vocoder, bad):
    mel = torch.zeros(2, 80, 12)                       # a CPU mel: reaching the device check would raise RuntimeError instead
    with pytest.raises(ValueError, match="lengths"):
        vocoder(mel, lengths=bad)


def test_gradient_over_items_is_refused_and_good_lengths_reach_the_device_check(vocoder):
    mel = torch.zeros(2, 80, 12)
    with pytest.raises(NotImplementedError, match="gradient"):
        vocoder(mel.clone().requires_grad_(), lengths=[12, 0])
    for good in ([12, 0], (3, 4), torch.tensor([0, 12]), torch.tensor([5, 6], dtype=torch.int32)):
        with pytest.raises(RuntimeError, match="GPU"):  # the lengths passed; the CPU mel is what is refused (no CPU path)
            vocoder(mel, lengths=good)
    with pytest.raises(ValueError, match="mel"):
        vocoder(torch.zeros(80, 12), lengths=[12])


def test_the_new_entry_points_are_bound():
    from dmel_codec_amd import _lib
    import ctypes as C
    for name, nargs in (("dmel_aa_snake_items_f32", 12), ("dmel_conv_post_items_f32", 11), ("dmel_bigvgan_forward_items", 9),
                        ("dmel_bigvgan_items_workspace_bytes", 3)):
        res, args = _lib.PROTOTYPES[name]
        assert len(args) == nargs and res is (C.c_size_t if name.endswith("bytes") else C.c_int)
        assert callable(getattr(_lib.lib(), name))
    assert _lib.lib().dmel_abi_version() == 2
    import dmel_codec_amd.torch_ops  # noqa: F401
    y = torch.ops.dmel_hip.bigvgan_forward_items(0, torch.empty(3, 80, 7, device="meta"), torch.empty(3, dtype=torch.int64, device="meta"), 8,
                                                 torch.empty(0, dtype=torch.uint8, device="meta"))
    assert y.shape == (3, 1, 56) and y.dtype == torch.float32


# ------------------------------------------------------------------------------------ padding and cropping
def test_pad_windows():
    g = torch.Generator().manual_seed(1)
    wins = [torch.randn(5, w, generator=g) for w in (7, 1, 4)]
    batch, widths = pad_windows(wins)
    assert widths == [7, 1, 4] and batch.shape == (3, 5, 7) and batch.is_contiguous()
    for i, w in enumerate(wins):
        assert torch.equal(batch[i, :, :w.shape[1]], w) and bool((batch[i, :, w.shape[1]:] == 0).all())
    same = [torch.randn(5, 6, generator=g) for _ in range(3)]
    batch, widths = pad_windows(same)                  # one length: the plain call, no lengths
    assert widths is None and torch.equal(batch, torch.stack(same)) and batch.is_contiguous()
    batch, widths = pad_windows(wins[:1])
    assert widths is None and torch.equal(batch[0], wins[0])


def stub_vocoder(mel, lengths=None):
    """(n, C, W) -> (n, 1, W * UP): a 3-frame filter over channel 0 with ZERO padding at each item's own ends, zeros behind an item's
    length, NaN-proof only if the padding is never read -- the contract of BigVGAN.forward(x, lengths), with one frame of context"""
    n, _, W = mel.shape
    lengths = [W] * n if lengths is None else lengths
    out = torch.zeros(n, 1, W * UP)
    for b, m in enumerate(lengths):
        x = torch.nn.functional.pad(mel[b, 0, :m], (1, 1))
        y = x[:-2] + 2 * x[1:-1] + 3 * x[2:]
        out[b, 0, :m * UP] = (y[:, None] * torch.arange(1, UP + 1)).reshape(-1)
    return out


def test_one_padded_call_per_step_reassembles_every_session():
    ragged, equal = 0, 0
    for seed in range(6):
        r, e = serve_three_sessions(seed)
        ragged, equal = ragged + r, equal + e
    assert ragged > 10 and equal > 10                  # both kinds of step took part


def serve_three_sessions(seed):
    """Three sessions with their own push sizes (0- and 1-token pushes, one shorter than the lookahead): per step, the windows
    DecodeSchedule names go through pad_windows and ONE stub call, are cropped as DecodeSessions.push crops, and concatenate to the stub
    on each whole clip.  The padding is NaN-filled after pad_windows, so an item that read beyond its length would show."""
    rng = random.Random(seed)
    geo = DecodeGeometry(factor=4, dilations=(1, 2, 4), voc_halo=3)
    lengths = [rng.randint(20, 60), 3, rng.randint(5, 40)]
    g = torch.Generator().manual_seed(seed)
    mels = [torch.randn(2, 4 * T, generator=g) for T in lengths]
    scheds, pos, got = [DecodeSchedule(geo) for _ in lengths], [0] * 3, [[] for _ in lengths]
    ragged_steps = equal_steps = 0
    while any(not s.finished for s in scheds):
        steps = {}
        for i, s in enumerate(scheds):
            if s.finished:
                continue
            n = min(rng.choice([0, 1, rng.randint(0, 16), 16]), lengths[i] - pos[i])
            pos[i] += n
            steps[i] = s.step(n, pos[i] == lengths[i])
        members = [i for i, st in steps.items() if st.voc_window[1] > st.voc_window[0]]
        if not members:
            continue
        batch, widths = pad_windows([mels[i][:, steps[i].voc_window[0]:steps[i].voc_window[1]] for i in members])
        equal_steps += widths is None
        if widths is not None:
            ragged_steps += 1
            for j, w in enumerate(widths):
                assert w == steps[members[j]].voc_window[1] - steps[members[j]].voc_window[0] <= batch.shape[2]
                batch[j, :, w:] = float("nan")
        wav = stub_vocoder(batch) if widths is None else stub_vocoder(batch, widths)
        for j, i in enumerate(members):
            st = steps[i]
            lo = st.voc_window[0]
            got[i].append(wav[j, :, (st.emit[0] - lo) * UP:(st.emit[1] - lo) * UP])
    for i, T in enumerate(lengths):
        audio = torch.cat(got[i], dim=1)
        assert audio.shape == (1, 4 * T * UP) and torch.equal(audio, stub_vocoder(mels[i][None])[0])
    return ragged_steps, equal_steps
