"""dmel_denoise_items on the GPU against the host rule (dmel_codec_amd/utils/denoise.py: scan), bit for bit: the samples re-written
in place, the state rows compared as int32, and both output rows.  Frames from the shortest to the longest; counts on both sides of a
hop and over several; row offsets on and off the 16-byte grid; launches that continue mid-hop; an idle item between two live ones;
two configs and two frame lengths in one launch; a silent item, one whose squares are subnormal, one still learning.  Idle rows, the
columns around an item's range and the words behind a row's frames carry sentinels."""
import numpy as np
import pytest
import torch

from dmel_codec_amd.utils import denoise
from dmel_codec_amd.utils.denoise import DenoiseConfig

pytestmark = pytest.mark.gpu

SENTINEL_WORD, SENTINEL_OUT, SENTINEL_SAMPLE, GUARD = 0x7FC00123, -7.5, 3.0e38, 9
# learn_frames = 3: the counts below pass through learning, the creep and the tracker
CONFIGS = {64: DenoiseConfig(frame_samples=64, learn_frames=3, alpha=0.9), 256: DenoiseConfig(frame_samples=256, learn_frames=3),
           1024: DenoiseConfig(frame_samples=1024, learn_frames=2, track=0.2, floor_gain=0.05)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def transform(dev):
    return denoise.transform_table().to(dev)


def bits(t):
    return t.contiguous().view(torch.int32)


class Bank:
    """S slots on the device next to the host rule: every launch is checked on the spot"""

    def __init__(self, dev, transform, cfgs, idle=()):
        self.dev, self.transform, self.cfgs, self.S = dev, transform, list(cfgs), len(cfgs)
        self.state = torch.zeros(self.S, denoise.STATE_WORDS, dtype=torch.int32, device=dev)
        for s in idle:
            self.state[s] = SENTINEL_WORD
        self.idle = set(idle)
        self.ref = [denoise.fresh_state() for _ in range(self.S)]
        self.table = torch.empty(denoise.TABLE_WORDS * self.S, dtype=torch.int32, device=dev)
        self.out = [[] for _ in range(self.S)]
        self.y = [[] for _ in range(self.S)]

    def launch(self, pieces, first):
        """pieces[s]: the new samples of slot s (None or empty: idle), placed at column first[s] of its row between sentinels"""
        S = self.S
        n_new = [0 if p is None else int(p.shape[0]) for p in pieces]
        width = max(f + n for f, n in zip(first, n_new)) + GUARD
        pitch = max([denoise.max_frames(n, c.frame_samples) for n, c in zip(n_new, self.cfgs) if n] + [0]) + 3
        rows = torch.full((S, width), SENTINEL_SAMPLE, dtype=torch.float32)
        for s in range(S):
            if n_new[s]:
                rows[s, first[s]:first[s] + n_new[s]] = torch.from_numpy(pieces[s])
        drows = rows.to(self.dev)
        pi = torch.full((S, pitch), SENTINEL_OUT, dtype=torch.float32, device=self.dev)
        po = torch.full((S, pitch), SENTINEL_OUT, dtype=torch.float32, device=self.dev)
        denoise.denoise_items(drows, first, n_new, [c if n else None for c, n in zip(self.cfgs, n_new)], self.state, pi, po,
                              self.transform, table=self.table)
        got, state, pi, po = drows.cpu(), self.state.cpu(), pi.cpu(), po.cpu()
        for s in range(S):
            f, n = first[s], n_new[s]
            if n:
                y, self.ref[s], p, q = denoise.scan(pieces[s], self.cfgs[s], self.ref[s])
                bad = (bits(got[s, f:f + n]) != bits(y)).nonzero().flatten().tolist()
                assert not bad, (s, n, f, bad[:8], got[s, f:f + n][bad[:8]].tolist(), y[bad[:8]].tolist())
                rows[s, f:f + n] = y
                self.y[s].append(y)
            else:
                p = q = torch.zeros(0)
            assert torch.equal(bits(got[s]), bits(rows[s])), (s, n, f)          # the guard columns, and a whole idle row, unchanged
            B = p.shape[0]
            assert torch.equal(bits(pi[s, :B]), bits(p)) and torch.equal(bits(po[s, :B]), bits(q)), (s, n, pi[s, :B].tolist(), p.tolist())
            assert (pi[s, B:] == SENTINEL_OUT).all() and (po[s, B:] == SENTINEL_OUT).all(), (s, n)
            if s in self.idle:
                assert (state[s] == SENTINEL_WORD).all(), s
            else:
                diff = (state[s] != self.ref[s]).nonzero().flatten().tolist()
                assert not diff, (s, n, diff[:8], state[s][diff[:8]].tolist(), self.ref[s][diff[:8]].tolist())
            self.out[s].append((p, q))


def clip_for(seed, n, scale=0.05):
    """noise whose level moves, with a tone that starts abruptly: bins on both sides of the tracker's ratio, gains above the floor"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * scale
    x[n // 2:] += 0.3 * np.sin(2 * np.pi * 0.07 * np.arange(n - n // 2))
    x[2 * n // 3:] *= 0.3
    return x.astype(np.float32)


@pytest.mark.parametrize("first", [0, 1, 3, 4])
@pytest.mark.parametrize("N", sorted(CONFIGS))
def test_counts_around_a_hop_at_every_alignment(dev, transform, N, first):
    cfg, H = CONFIGS[N], N // 2
    counts = [1, H - 1, H, H + 1, 3 * H + 5, 7 * H + 3]
    # every count from a fresh state in a launch of S = 3 whose middle item is idle (n_new = 0: its sample row, state row and
    # outputs keep their sentinels), and the same counts as one stream, so that every launch but the first continues mid-hop
    x = clip_for(N + first, sum(counts))
    stream, at = Bank(dev, transform, [cfg]), 0
    for n in counts:
        piece = x[at:at + n]
        Bank(dev, transform, [cfg, cfg, cfg], idle=(1,)).launch([piece, None, piece], [first, first, first + 2])
        stream.launch([piece], [first])
        at += n
    assert int(stream.ref[0][denoise.I_FRAMES]) == sum(counts) // H and int(stream.ref[0][denoise.I_LEARNED]) == cfg.learn_frames
    whole = denoise.scan(x, cfg)
    assert torch.equal(bits(torch.cat(stream.y[0])), bits(whole[0])) and torch.equal(stream.ref[0], whole[1])


@pytest.mark.parametrize("N", [64, 256])
def test_a_second_launch_continues_the_first_mid_hop(dev, transform, N):
    cfg, H = CONFIGS[N], N // 2
    x = clip_for(7 * N, 9 * N)
    bank = Bank(dev, transform, [cfg, cfg])
    cut = 5 * H + H // 3
    bank.launch([x, x[:cut]], [2, 5])
    assert int(bank.ref[1][denoise.I_FILL]) == H // 3
    bank.launch([None, x[cut:]], [0, 3])
    assert torch.equal(bank.ref[0], bank.ref[1]) and torch.equal(bank.state[0], bank.state[1])
    assert torch.equal(bits(torch.cat(bank.y[1])), bits(bank.y[0][0]))
    assert torch.equal(torch.cat([p for p, _ in bank.out[1]]), bank.out[0][0][0])
    assert torch.equal(torch.cat([q for _, q in bank.out[1]]), bank.out[0][0][1])


def test_two_configs_two_frames_silence_subnormal_squares_and_a_learning_item(dev, transform):
    other = DenoiseConfig(frame_samples=128, alpha=0.5, track=1.0, track_ratio=2.0, creep=1.05, floor_gain=0.3, eps=1e-12, learn_frames=1)
    learning = DenoiseConfig(frame_samples=256, learn_frames=64)
    n = 2600
    x = clip_for(11, n)
    rng = np.random.default_rng(5)
    quiet = (rng.standard_normal(n) * 1e-20).astype(np.float32)               # squares around 1e-40: subnormal
    bank = Bank(dev, transform, [DenoiseConfig(), other, DenoiseConfig(), DenoiseConfig(frame_samples=64), learning])
    bank.launch([x, x, np.zeros(n, dtype=np.float32), quiet, x], [1, 2, 3, 0, 5])
    silent = denoise.report(bank.state[2])
    assert silent.frames == n // 256 and silent.learned == 0 and silent.power_in == 0.0
    assert not bank.state[2, denoise.O_RAW:].any() and not bank.y[2][0].any()
    assert torch.isfinite(bank.y[3][0]).all() and denoise.report(bank.state[3], 64).frames == n // 32
    rep = denoise.report(bank.state[4], 256, learn_frames=64)
    assert rep.learning and rep.learned == n // 128
    assert denoise.report(bank.state[1], 128, learn_frames=1) == denoise.report(bank.ref[1], 128, learn_frames=1)
    # a second launch of all five, each from its own offset
    bank.launch([x[:700], x[:3], np.zeros(5, dtype=np.float32), quiet[:100], x[:129]], [4, 3, 2, 1, 0])
