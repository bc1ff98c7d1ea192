"""dmel_dtmf_items on the GPU against the host rule (dmel_codec_amd/utils/dtmf.py: scan), bit for bit: the state rows compared as
int32, and both byte rows.  One launch with an idle item, an item that only extends the open block, one that ends exactly on a block
boundary and one with a carried partial block, whole blocks and a tail, at every block length from the shortest to the longest and
at row offsets that are not 16-byte aligned; more blocks than one pass of the workgroup takes (28); one clip in one launch and in
the cuts of the host test; all-zero input, a tone pair in noise and pure noise; the event ring wrapping inside one launch.  Idle
rows, the samples around a slot's columns and the bytes behind a row's blocks carry sentinels."""
import numpy as np
import pytest
import torch

from dmel_codec_amd.utils import dtmf
from dmel_codec_amd.utils.dtmf import DtmfConfig
from test_dtmf_cpu import cuts_of, keyed_clip, tone

pytestmark = pytest.mark.gpu

SENTINEL_WORD, SENTINEL_BYTE, SENTINEL_SAMPLE = 0x7FC00123, 0xEE, 3.0e38
LOOSE = dict(rel=0.01, max_col_over_row=100.0, max_row_over_col=100.0, purity=0.05)       # what a block of 32 samples can decide
# rate, N, config: the shortest block, the defaults at the three rates of the host test, the longest block
SHAPES = {32: (4000, DtmfConfig(block_samples=32, hits=1, misses=1, **LOOSE)), 102: (8000, DtmfConfig()), 307: (24000, DtmfConfig()),
          564: (44100, DtmfConfig()), 4096: (24000, DtmfConfig(block_samples=4096, hits=1, misses=1))}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


class Bank:
    """S slots on the device next to the host rule: every launch is checked on the spot"""

    def __init__(self, dev, rate, cfgs, idle=()):
        self.dev, self.rate, self.cfgs, self.S = dev, rate, list(cfgs), len(cfgs)
        self.state = torch.zeros(self.S, dtmf.STATE_WORDS, dtype=torch.int32, device=dev)
        for s in idle:
            self.state[s] = SENTINEL_WORD
        self.idle = set(idle)
        self.ref = [dtmf.fresh_state() for _ in range(self.S)]
        self.table = torch.empty(dtmf.TABLE_WORDS * self.S, dtype=torch.int32, device=dev)
        self.decided, self.pressed = [[] for _ in range(self.S)], [[] for _ in range(self.S)]

    def launch(self, pieces, first):
        """pieces[s]: the new samples of slot s (None or empty: idle), placed at column first[s] of its row between sentinels"""
        S = self.S
        n_new = [0 if p is None else int(p.shape[0]) for p in pieces]
        width = max(f + n for f, n in zip(first, n_new)) + 7
        Ns = [c.block(self.rate) if c else 0 for c in self.cfgs]
        pitch = max([dtmf.max_blocks(n, N) for n, N in zip(n_new, Ns) if n] + [0]) + 3
        rows = torch.full((S, width), SENTINEL_SAMPLE, dtype=torch.float32)
        for s in range(S):
            if n_new[s]:
                rows[s, first[s]:first[s] + n_new[s]] = torch.from_numpy(pieces[s])
        dec = torch.full((S, pitch), SENTINEL_BYTE, dtype=torch.uint8, device=self.dev)
        prs = torch.full((S, pitch), SENTINEL_BYTE, dtype=torch.uint8, device=self.dev)
        dtmf.dtmf_items(rows.to(self.dev), first, n_new, [c if n else None for c, n in zip(self.cfgs, n_new)], self.state, dec, prs,
                        sample_rate=self.rate, table=self.table)
        state, dec, prs = self.state.cpu(), dec.cpu(), prs.cpu()
        for s in range(S):
            if n_new[s]:
                self.ref[s], d, p = dtmf.scan(pieces[s], self.cfgs[s], self.ref[s], self.rate)
            else:
                d = p = torch.zeros(0, dtype=torch.uint8)
            B = d.shape[0]
            assert torch.equal(dec[s, :B], d) and torch.equal(prs[s, :B], p), (s, n_new[s], dec[s, :B].tolist(), d.tolist())
            assert (dec[s, B:] == SENTINEL_BYTE).all() and (prs[s, B:] == SENTINEL_BYTE).all(), (s, n_new[s])
            if s in self.idle:
                assert (state[s] == SENTINEL_WORD).all(), s
            else:
                diff = (state[s] != self.ref[s]).nonzero().flatten().tolist()
                assert not diff, (s, n_new[s], diff, state[s][diff].tolist(), self.ref[s][diff].tolist())
            self.decided[s].append(d), self.pressed[s].append(p)


def clip_for(rate, N, cfg, seed, blocks):
    """keys in noise, long enough for `blocks` blocks"""
    rng = np.random.default_rng(seed)
    x = keyed_clip(rate, N, [int(k) for k in rng.permutation(16)[:6]], rng)
    while x.shape[0] < blocks * N:
        x = np.concatenate([x, keyed_clip(rate, N, [int(k) for k in rng.permutation(16)[:6]], rng)])
    return x


@pytest.mark.parametrize("first", [0, 1, 3, 5])
@pytest.mark.parametrize("N", sorted(SHAPES))
def test_the_four_kinds_of_item_in_one_launch(dev, N, first):
    rate, cfg = SHAPES[N]
    assert cfg.block(rate) == N
    bank = Bank(dev, rate, [cfg] * 4, idle=(0,))
    clips = [None] + [clip_for(rate, N, cfg, 10 * N + s, 12) for s in (1, 2, 3)]
    # launch 1 leaves an open block in every live slot; launch 2: idle | the open block only grows | ends exactly on a block
    # boundary | a carried partial block, nine whole blocks and a tail
    plan = [[0, N // 3, N // 2, N - 5], [0, N // 3, (N - N // 2) + 2 * N, 5 + 9 * N + 17], [0, 1, 1, N - 17]]
    at = [0] * 4
    for j, sizes in enumerate(plan):
        pieces = [None if not n else clips[s][at[s]:at[s] + n] for s, n in enumerate(sizes)]
        assert all(p is None or p.shape[0] == n for p, n in zip(pieces, sizes))
        bank.launch(pieces, [first + s for s in range(4)] if j == 1 else [first] * 4)
        at = [a + n for a, n in zip(at, sizes)]
        fills = [int(r[dtmf.I_FILL]) for r in bank.ref]
        if j == 1:
            assert fills[1] == 2 * (N // 3) and int(bank.ref[1][dtmf.I_BLOCKS]) == 0 and bank.ref[1][:17].any()
            assert fills[2] == 0 and int(bank.ref[2][dtmf.I_BLOCKS]) == 3 and not bank.ref[2][:18].any()
            assert fills[3] == 17 and int(bank.ref[3][dtmf.I_BLOCKS]) == 10
    assert fills[3] == 0 and int(bank.ref[3][dtmf.I_BLOCKS]) == 11              # the last launch closed the open block of slot 3


@pytest.mark.parametrize("N", [32, 102, 307])
def test_more_blocks_than_one_pass_takes(dev, N):
    rate, cfg = SHAPES[N]
    bank = Bank(dev, rate, [cfg] * 3)
    clips = [clip_for(rate, N, cfg, 77 * N + s, 90) for s in range(3)]
    # 27, 28 and 29 blocks with and without a carry and a tail: on both sides of the pass, then two and a bit passes
    plan = [[27 * N, 28 * N - 1, 7], [N + 3, 29 * N, 28 * N - 7], [57 * N + 1 - (N + 3), 1, 61 * N]]
    at = [0] * 3
    for sizes in plan:
        bank.launch([clips[s][at[s]:at[s] + n] for s, n in enumerate(sizes)], [2, 0, 1])
        at = [a + n for a, n in zip(at, sizes)]
    assert all(sum(d.shape[0] for d in bank.decided[s]) == at[s] // N for s in range(3))
    assert any(int(r[dtmf.I_EVENTS]) > 0 for r in bank.ref)


@pytest.mark.parametrize("N", [102, 307])
def test_one_clip_in_one_launch_and_in_the_cuts_of_the_host_test(dev, N):
    rate, cfg = SHAPES[N]
    x = clip_for(rate, N, cfg, 5 * N, 40)
    sizes = cuts_of(x.shape[0], N, np.random.default_rng(N))
    bank = Bank(dev, rate, [cfg, cfg])
    at = 0
    for j, k in enumerate(sizes):
        bank.launch([x if j == 0 else None, x[at:at + k] if k else None], [3, j % 7])
        at += k
    assert at == x.shape[0] and torch.equal(bank.ref[0], bank.ref[1]) and int(bank.ref[0][dtmf.I_EVENTS]) >= 6
    assert torch.equal(torch.cat(bank.decided[0]), torch.cat(bank.decided[1])) and torch.equal(torch.cat(bank.pressed[0]), torch.cat(bank.pressed[1]))
    assert dtmf.report(bank.state[1], N, rate) == dtmf.report(bank.ref[0], N, rate)


def test_zeros_a_tone_pair_in_noise_and_pure_noise(dev):
    rate, N, cfg = 8000, 102, DtmfConfig()
    rng = np.random.default_rng(5)
    n = 20 * N + 31
    pair = (tone(n, rate, 941.0, 0.1, 0.4) + tone(n, rate, 1336.0, 0.08, 2.0) + rng.standard_normal(n) * 0.0126).astype(np.float32)
    noise = (rng.standard_normal(n) * 0.1).astype(np.float32)
    bank = Bank(dev, rate, [cfg] * 3)
    bank.launch([np.zeros(n, np.float32), pair, noise], [1, 2, 3])
    # all-zero input: ties in both argmaxes and E == 0 decide nothing, and the carry of the open block is the zeroed one
    assert not bank.ref[0][:17].any() and not bank.decided[0][0].any() and int(bank.ref[0][dtmf.I_BLOCKS]) == 20
    assert bank.decided[1][0].tolist() == [14] * 20 and bank.pressed[1][0].tolist() == [0] + [14] * 19     # "0": row 3, column 1
    assert not bank.pressed[2][0].any() and dtmf.report(bank.state[1], N, rate).down == "0"
    bank.launch([np.zeros(N, np.float32), np.zeros(3 * N - 31, np.float32), noise[:5]], [0, 0, 0])          # the key goes up
    rep = dtmf.report(bank.state[1], N, rate)
    assert rep == dtmf.report(bank.ref[1], N, rate) and rep.down is None and rep.events[0][:3] == (0, "0", 0)
    assert rep.events[0][3] in (20 * N, 21 * N)                             # the block that is part tone, part silence may decide either way


def test_the_ring_wraps_inside_one_launch(dev):
    rate, (_, cfg) = 4000, SHAPES[32]
    parts = []
    for i, k in enumerate([0, 15] * 20):                                    # two blocks of the key, two of silence, as on the host
        parts.append(tone(64, rate, dtmf.ROWS_HZ[k // 4], 0.2, 0.1 * i) + tone(64, rate, dtmf.COLS_HZ[k % 4], 0.2, 0.2 * i))
        parts.append(np.zeros(64))
    x = np.concatenate(parts).astype(np.float32)
    bank = Bank(dev, rate, [cfg, cfg])
    bank.launch([x, x[:1000]], [5, 0])
    bank.launch([None, x[1000:]], [0, 9])
    rep = dtmf.report(bank.state[0], 32, rate)
    assert rep.total == 40 and len(rep.events) == 32 and rep.digits == "1D" * 16 and rep == dtmf.report(bank.state[1], 32, rate)
