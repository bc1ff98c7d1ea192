"""dmel_echo_items on the GPU against the host rule (dmel_codec_amd/utils/echo.py: scan), bit for bit: the samples re-written in
place, the whole state rows compared as int32 -- taps, open block and the ring of far samples -- and both output rows.  Filters
from the shortest to the longest; counts on both sides of a block and above what one pass of the workgroup takes; a row offset off
the 16-byte grid; launches that continue an open block; a far end that is level with the samples, ahead by less than a block, by
the ring's whole room, behind (missing samples), and pushed alone; both delays; a frozen block of each kind; an idle item between
two live ones.  Idle rows, the columns around an item's range and the words behind a row's blocks carry sentinels."""
import numpy as np
import pytest
import torch

from dmel_codec_amd.utils import echo
from dmel_codec_amd.utils.echo import EchoConfig
from test_echo_cpu import echo_path, echoed, far_end

pytestmark = pytest.mark.gpu

SENTINEL_WORD, SENTINEL_OUT, SENTINEL_SAMPLE, GUARD = 0x7FC00123, -7.5, 3.0e38, 9
f32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32)


class Bank:
    """S slots on the device next to the host rule: every launch is checked on the spot"""

    def __init__(self, dev, cfgs, idle=()):
        self.dev, self.cfgs, self.S = dev, list(cfgs), len(cfgs)
        self.state = torch.zeros(self.S, echo.ROW_WORDS, dtype=torch.int32, device=dev)
        for s in idle:
            self.state[s] = SENTINEL_WORD
        self.idle = set(idle)
        self.ref = [echo.fresh_state() for _ in range(self.S)]
        self.table = torch.empty(echo.TABLE_WORDS * self.S, dtype=torch.int32, device=dev)
        self.out = [[] for _ in range(self.S)]
        self.e = [[] for _ in range(self.S)]

    def launch(self, pieces, fars, first):
        """pieces[s]: the new samples of slot s (None: none), placed at column first[s] of its row between sentinels; fars[s]: its
        new far samples (None: none)"""
        S = self.S
        n_new = [0 if p is None else int(p.shape[0]) for p in pieces]
        width = max(f + n for f, n in zip(first, n_new)) + GUARD
        pitch = max([echo.max_blocks(n, c.block_samples) for n, c in zip(n_new, self.cfgs) if n] + [0]) + 3
        rows = torch.full((S, width), SENTINEL_SAMPLE, dtype=torch.float32)
        for s in range(S):
            if n_new[s]:
                rows[s, first[s]:first[s] + n_new[s]] = torch.from_numpy(pieces[s])
        drows = rows.to(self.dev)
        dfar = [None if x is None else torch.from_numpy(x).to(self.dev) for x in fars]
        bi = torch.full((S, pitch), SENTINEL_OUT, dtype=torch.float32, device=self.dev)
        br = torch.full((S, pitch), SENTINEL_OUT, dtype=torch.float32, device=self.dev)
        live = [n > 0 or x is not None for n, x in zip(n_new, fars)]
        echo.echo_items(drows, first, n_new, dfar, [c if on else None for c, on in zip(self.cfgs, live)], self.state, bi, br,
                        table=self.table)
        got, state, bi, br = drows.cpu(), self.state.cpu(), bi.cpu(), br.cpu()
        for s in range(S):
            f, n = first[s], n_new[s]
            p = r = torch.zeros(0)
            if live[s]:
                e, self.ref[s], p, r = echo.scan(pieces[s] if n else np.zeros(0, f32), fars[s], self.cfgs[s], self.ref[s])
                bad = (bits(got[s, f:f + n]) != bits(e)).nonzero().flatten().tolist()
                assert not bad, (s, n, f, bad[:8], got[s, f:f + n][bad[:8]].tolist(), e[bad[:8]].tolist())
                rows[s, f:f + n] = e
                self.e[s].append(e)
            assert torch.equal(bits(got[s]), bits(rows[s])), (s, n, f)          # the guard columns, and a whole idle row, unchanged
            B = p.shape[0]
            assert torch.equal(bits(bi[s, :B]), bits(p)) and torch.equal(bits(br[s, :B]), bits(r)), (s, n, bi[s, :B].tolist(), p.tolist())
            assert (bi[s, B:] == SENTINEL_OUT).all() and (br[s, B:] == SENTINEL_OUT).all(), (s, n)
            if s in self.idle:
                assert (state[s] == SENTINEL_WORD).all(), s
            else:
                diff = (state[s] != self.ref[s]).nonzero().flatten().tolist()
                assert not diff, (s, n, len(diff), diff[:8], state[s][diff[:8]].tolist(), self.ref[s][diff[:8]].tolist())
            self.out[s].append((p, r))


def clip_for(seed, n, kind="ar1"):
    """a far end and its echo through a short decaying path, with a little near-end noise"""
    x = far_end(kind, n, seed=seed)
    d = echoed(x, echo_path(seed=seed + 1, taps=48, delay=6)) + (np.random.default_rng(seed + 2).standard_normal(n) * 0.002).astype(f32)
    return d, x


@pytest.mark.parametrize("L,N,delay,lead", [(64, 16, 0, 0), (128, 32, 37, 5), (192, 24, 0, 1000), (1024, 32, 37, 0)])
def test_counts_around_a_block_and_a_pass_off_the_grid(dev, L, N, delay, lead):
    """lead: how far the far end is pushed ahead of the samples of its launch (0: level, 5: less than a block)"""
    cfg = EchoConfig(taps=L, block_samples=N, delay_samples=delay, far_floor=1e-4)
    counts = [1, N - 1, N, N + 1, 3 * N + 5, echo.PASS_SAMPLES + N + 3]    # the last: the pass loop turns twice
    d, x = clip_for(L + N, sum(counts) + lead)
    # every count from a fresh state in a launch of S = 3 whose middle item is idle (its sample row, state row and outputs keep
    # their sentinels), and the same counts as one stream, so that every launch but the first continues an open block
    stream, at, fa = Bank(dev, [cfg]), 0, 0
    for n in counts:
        piece = d[at:at + n]
        Bank(dev, [cfg, cfg, cfg], idle=(1,)).launch([piece, None, piece], [x[at:at + n + lead], None, x[at:at + n]], [3, 3, 5])
        stream.launch([piece], [x[fa:at + n + lead]], [3])
        at, fa = at + n, at + n + lead
    ref = stream.ref[0]
    assert int(ref[echo.I_T]) == sum(counts) and int(ref[echo.I_BLOCKS]) == sum(counts) // N and int(ref[echo.I_MISSING]) == 0
    assert int(ref[echo.I_ADAPTED]) > 8 and int(ref[echo.I_F]) - int(ref[echo.I_T]) == lead      # (a delay beyond the path's freezes many)
    whole = echo.scan(d[:at], x[:at + lead], cfg)                           # and the launches together are the one call
    assert torch.equal(torch.cat(stream.e[0]), whole[0]) and torch.equal(stream.ref[0], whole[1])
    assert not torch.equal(whole[0], torch.from_numpy(d[:at]))


def test_the_longest_filter_and_block_once(dev):
    cfg = EchoConfig(taps=2048, block_samples=256, delay_samples=11)
    d, x = clip_for(3, 1200, "white")
    bank = Bank(dev, [cfg, cfg])
    bank.launch([d[:700], d[:1200]], [x[:900], x[:1200]], [1, 2])           # slot 0 stops mid-block with far samples queued
    assert int(bank.ref[0][echo.I_FILL]) == 700 - 512 and int(bank.ref[0][echo.I_F]) == 900
    bank.launch([d[700:1200], None], [x[900:1200], None], [6, 0])
    assert torch.equal(bank.ref[0], bank.ref[1]) and torch.equal(bank.state[0], bank.state[1])
    assert torch.equal(torch.cat(bank.e[0]), bank.e[1][0]) and int(bank.ref[0][echo.I_BLOCKS]) == 4 and int(bank.ref[0][echo.I_ADAPTED]) >= 2


def test_state_over_three_launches_with_an_open_block_and_two_configs_in_one_launch(dev):
    a, b = EchoConfig(taps=64, block_samples=16, delay_samples=37), EchoConfig(taps=192, block_samples=24, mu=0.5, double_talk=0.0)
    d, x = clip_for(9, 400)
    bank = Bank(dev, [a, b])
    cuts = [0, 16 * 5 + 7, 16 * 5 + 12, 400]                                # the second launch neither begins nor ends on a block of `a`
    for lo, hi in zip(cuts, cuts[1:]):
        bank.launch([d[lo:hi], d[lo:hi]], [x[lo:hi], x[lo:hi]], [lo % 5, 2])
    for s, cfg in enumerate((a, b)):
        whole = echo.scan(d, x, cfg)
        assert torch.equal(torch.cat(bank.e[s]), whole[0]) and torch.equal(bank.ref[s], whole[1])
        assert torch.equal(torch.cat([p for p, _ in bank.out[s]]), whole[2]) and torch.equal(torch.cat([r for _, r in bank.out[s]]), whole[3])
    assert echo.report(bank.state[0], 16) == echo.report(bank.ref[0], 16)
    assert echo.report(bank.state[0, :16], 16).blocks == 25


def test_a_far_end_alone_ahead_by_the_whole_room_and_behind(dev):
    cfg = EchoConfig(taps=128, block_samples=32, delay_samples=37, far_floor=1e-4)
    n = echo.MAX_AHEAD + 600
    d, x = clip_for(21, n, "white")
    bank = Bank(dev, [cfg, cfg, cfg], idle=(1,))
    # slot 0: the far end alone, all the ring takes; slot 2: samples with no far end at all (every one behind the delay misses)
    bank.launch([None, None, d[:100]], [x[:echo.MAX_AHEAD], None, None], [0, 0, 1])
    assert echo.report(bank.state[0]).far_ahead == echo.MAX_AHEAD and echo.report(bank.state[0]).total_samples == 0
    assert echo.report(bank.state[2]).far_missing == 100 - 37 and echo.report(bank.state[2]).frozen_blocks == 3
    with pytest.raises(ValueError, match="ahead"):
        echo.scan(np.zeros(0, f32), x[:1], cfg, bank.ref[0])                # the host rule refuses one more
    # slot 0 catches up in two launches and the far end goes on; slot 2 gets its far end late: x[0 .. 63) had their turn and are
    # dropped, and the samples 500 .. 600 run 63 past the end of the far end again
    bank.launch([d[:3000], None, d[100:500]], [None, None, x[:500]], [3, 0, 2])
    bank.launch([d[3000:3100], None, d[500:600]], [x[echo.MAX_AHEAD:], None, None], [1, 0, 0])
    assert echo.report(bank.state[0]).far_ahead == n - 3100 and echo.report(bank.state[0]).far_missing == 0
    assert echo.report(bank.state[2]).far_missing == 126
    assert echo.report(bank.state[2]) == echo.report(bank.ref[2]) and echo.report(bank.state[2]).adapted_blocks > 5
    # the same samples with every far sample in time: the bits of one call
    assert torch.equal(torch.cat(bank.e[0]), echo.scan(d[:3100], x[:echo.MAX_AHEAD], cfg)[0])


def test_a_frozen_block_of_each_kind(dev):
    cfg = EchoConfig(taps=64, block_samples=16, far_floor=1e-3, double_talk=0.5)
    rng = np.random.default_rng(11)
    x = (rng.standard_normal(64) * 0.1).astype(f32)
    d = np.concatenate([np.zeros(1, f32), 0.4 * x[:-1]]).astype(f32)
    loud = d[:48].copy()
    loud[20] = f32(0.6) * np.abs(x[:32]).max()                               # the near end talks in block 1
    bank = Bank(dev, [cfg, cfg, cfg])
    bank.launch([d[:16] * f32(1e-3), loud, d[:48]], [x[:16] * f32(1e-3), x[:48], x[:48]], [0, 1, 2])
    got = [(r.adapted_blocks, r.frozen_blocks) for r in (echo.report(bank.state[s], 16) for s in range(3))]
    assert got == [(0, 1), (2, 1), (3, 0)]                                   # below the far floor; the Geigel test; neither
    assert not bank.state[0, echo.O_W:echo.O_E].any() and bank.state[1, echo.O_W:echo.O_E].any()


def test_the_refusals_return_an_error_and_write_nothing(dev):
    cfg = EchoConfig(taps=64, block_samples=16)
    rows = torch.full((2, 200), 0.25, dtype=torch.float32, device=dev)
    state = torch.zeros(2, echo.ROW_WORDS, dtype=torch.int32, device=dev)
    out = [torch.full((2, p), SENTINEL_OUT, dtype=torch.float32, device=dev) for p in (4, 4, 12)]
    far = torch.full((50,), 0.5, dtype=torch.float32, device=dev)

    def untouched():
        torch.cuda.synchronize()
        return bool((rows == 0.25).all()) and not state.any() and all(bool((o == SENTINEL_OUT).all()) for o in out)
    with pytest.raises(RuntimeError, match="item 1.*output pitch"):         # 100 samples can complete 7 blocks of 16
        echo.echo_items(rows, [0, 0], [10, 100], [far, far], [cfg, cfg], state, out[0], out[1])
    assert untouched()
    for kw, match in ((dict(first=[0, 150]), "no part of a row"), (dict(n_new=[10, -1]), "no part of a row"), (dict(configs=[cfg, None]), "no config"),
                      (dict(far=[far, far[::2]]), "contiguous"), (dict(far=[far, far.cpu()]), "contiguous"), (dict(far=[far.double(), None]), "fp32"),
                      (dict(state=state[:, :-1]), "state"), (dict(state=state[:1]), "state"), (dict(out_res=out[2]), "one pitch"),
                      (dict(table=torch.empty(31, dtype=torch.int32, device=dev)), "table"), (dict(first=[0]), "2 slots")):
        a = dict(dict(samples=rows, first=[0, 0], n_new=[10, 60], far=[far, None], configs=[cfg, cfg], state=state, out_in=out[0], out_res=out[1]), **kw)
        with pytest.raises(ValueError, match=match):
            echo.echo_items(**a)
        assert untouched(), kw
    # and the same launch, accepted, writes
    echo.echo_items(rows, [0, 0], [10, 60], [far, None], [cfg, cfg], state, out[0], out[1])
    assert not untouched() and int(state[1, echo.I_T]) == 60 and int(state[0, echo.I_F]) == 50
