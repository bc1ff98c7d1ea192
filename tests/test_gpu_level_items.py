"""dmel_level_items on the GPU against the host rule (dmel_codec_amd/utils/level.py: scan), bit for bit: the samples re-written in
place, the state rows compared as int32, and both output rows.  Block lengths from the shortest to the longest; counts on both sides
of a block and above what one pass of the workgroup takes; row offsets on and off the 16-byte grid; a second launch that continues an
open block; an idle item between two live ones; an input that clamps and one that never locks; two configs in one launch.  Idle
rows, the columns around an item's range and the words behind a row's blocks carry sentinels."""
import numpy as np
import pytest
import torch

from dmel_codec_amd.utils import level
from dmel_codec_amd.utils.level import LevelConfig
from test_level_cpu import RATE, burst_clip, sine

pytestmark = pytest.mark.gpu

SENTINEL_WORD, SENTINEL_OUT, SENTINEL_SAMPLE, GUARD = 0x7FC00123, -7.5, 3.0e38, 9
CONFIGS = {32: LevelConfig(block_samples=32, release=0.25), 240: LevelConfig(), 4096: LevelConfig(block_samples=4096, release=0.5)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32)


class Bank:
    """S slots on the device next to the host rule: every launch is checked on the spot"""

    def __init__(self, dev, cfgs, idle=(), rate=RATE):
        self.dev, self.rate, self.cfgs, self.S = dev, rate, list(cfgs), len(cfgs)
        self.state = torch.zeros(self.S, level.STATE_WORDS, dtype=torch.int32, device=dev)
        for s in idle:
            self.state[s] = SENTINEL_WORD
        self.idle = set(idle)
        self.ref = [level.fresh_state() for _ in range(self.S)]
        self.table = torch.empty(level.TABLE_WORDS * self.S, dtype=torch.int32, device=dev)
        self.out = [[] for _ in range(self.S)]

    def launch(self, pieces, first):
        """pieces[s]: the new samples of slot s (None or empty: idle), placed at column first[s] of its row between sentinels"""
        S = self.S
        n_new = [0 if p is None else int(p.shape[0]) for p in pieces]
        width = max(f + n for f, n in zip(first, n_new)) + GUARD
        Ns = [c.block(self.rate) if c else 0 for c in self.cfgs]
        pitch = max([level.max_blocks(n, N) for n, N in zip(n_new, Ns) if n] + [0]) + 3
        rows = torch.full((S, width), SENTINEL_SAMPLE, dtype=torch.float32)
        for s in range(S):
            if n_new[s]:
                rows[s, first[s]:first[s] + n_new[s]] = torch.from_numpy(pieces[s])
        drows = rows.to(self.dev)
        pk = torch.full((S, pitch), SENTINEL_OUT, dtype=torch.float32, device=self.dev)
        gn = torch.full((S, pitch), SENTINEL_OUT, dtype=torch.float32, device=self.dev)
        level.level_items(drows, first, n_new, [c if n else None for c, n in zip(self.cfgs, n_new)], self.state, pk, gn,
                          sample_rate=self.rate, table=self.table)
        got, state, pk, gn = drows.cpu(), self.state.cpu(), pk.cpu(), gn.cpu()
        for s in range(S):
            f, n = first[s], n_new[s]
            if n:
                y, self.ref[s], p, g = level.scan(pieces[s], self.cfgs[s], self.ref[s], self.rate)
                bad = (bits(got[s, f:f + n]) != bits(y)).nonzero().flatten().tolist()
                assert not bad, (s, n, f, bad[:8], got[s, f:f + n][bad[:8]].tolist(), y[bad[:8]].tolist())
                rows[s, f:f + n] = y
            else:
                p = g = torch.zeros(0)
            assert torch.equal(bits(got[s]), bits(rows[s])), (s, n, f)          # the guard columns, and a whole idle row, unchanged
            B = p.shape[0]
            assert torch.equal(bits(pk[s, :B]), bits(p)) and torch.equal(bits(gn[s, :B]), bits(g)), (s, n, pk[s, :B].tolist(), p.tolist())
            assert (pk[s, B:] == SENTINEL_OUT).all() and (gn[s, B:] == SENTINEL_OUT).all(), (s, n)
            if s in self.idle:
                assert (state[s] == SENTINEL_WORD).all(), s
            else:
                diff = (state[s] != self.ref[s]).nonzero().flatten().tolist()
                assert not diff, (s, n, diff, state[s][diff].tolist(), self.ref[s][diff].tolist())
            self.out[s].append((p, g))


def clip_for(seed, n, scale=0.05):
    """noise whose level moves: quiet, loud, quieter -- so that the envelope attacks, releases and the gain ramps"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * scale
    x[n // 3:n // 2] *= 6.0
    x[n // 2:] *= 0.3
    return x.astype(np.float32)


@pytest.mark.parametrize("first", [0, 1, 3, 4])
@pytest.mark.parametrize("N", sorted(CONFIGS))
def test_counts_around_a_block_and_a_pass_at_every_alignment(dev, N, first):
    cfg = CONFIGS[N]
    assert cfg.block(RATE) == N
    PB = level.pass_blocks(N)
    counts = [1, N - 1, N, N + 1, 3 * N + 5, (PB + 1) * N + 3]             # the last: the pass loop turns twice
    # every count from a fresh state in a launch of S = 3 whose middle item is idle (n_new = 0: its sample row, state row and
    # outputs keep their sentinels), and the same counts as one stream, so that every launch but the first continues an open block
    x = clip_for(N + first, sum(counts))
    stream, at = Bank(dev, [cfg]), 0
    for n in counts:
        piece = x[at:at + n]
        Bank(dev, [cfg, cfg, cfg], idle=(1,)).launch([piece, None, piece], [first, first, first + 2])
        stream.launch([piece], [first])
        at += n
    assert int(stream.ref[0][level.I_BLOCKS]) == sum(counts) // N and int(stream.ref[0][level.I_LOCKED]) == 1


@pytest.mark.parametrize("N", [32, 240])
def test_a_second_launch_continues_the_first_mid_block(dev, N):
    cfg = CONFIGS[N]
    x = clip_for(7 * N, 9 * N)
    bank = Bank(dev, [cfg, cfg])
    cut = 2 * N + N // 3
    bank.launch([x, x[:cut]], [2, 5])
    assert int(bank.ref[1][level.I_FILL]) == N // 3
    bank.launch([None, x[cut:]], [0, 3])
    assert torch.equal(bank.ref[0], bank.ref[1]) and torch.equal(bank.state[0], bank.state[1])
    assert torch.equal(torch.cat([p for p, _ in bank.out[1]]), bank.out[0][0][0])
    assert torch.equal(torch.cat([g for _, g in bank.out[1]]), bank.out[0][0][1])


def test_an_input_that_clamps_one_that_never_locks_and_two_configs_in_one_launch(dev):
    loud, quiet = burst_clip(), sine(1e-3, 4800)
    other = LevelConfig(block_samples=100, target_peak=0.25, max_gain=4.0, release=0.3, attack=0.5, ceiling=0.4, initial_gain=2.0)
    bank = Bank(dev, [LevelConfig(), LevelConfig(), other])
    bank.launch([loud, quiet, loud], [1, 2, 3])
    assert int(bank.ref[0][level.I_CLAMPED]) == 265 and int(bank.state[0][level.I_CLAMPED]) == 265
    rep = level.report(bank.state[1], 240, RATE)
    assert not rep.locked and rep.clamped == 0 and rep.blocks == 20           # its samples came back bit-equal (checked in launch)
    assert torch.equal(bits(level.scan(quiet, LevelConfig(), None, RATE)[0]), bits(torch.from_numpy(quiet)))
    assert int(bank.ref[2][level.I_CLAMPED]) > 0 and int(bank.ref[2][level.I_BLOCKS]) == 50
    assert level.report(bank.state[2], 100, RATE, 2.0) == level.report(bank.ref[2], 100, RATE, 2.0)
