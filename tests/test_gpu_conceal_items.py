"""dmel_conceal_items on the GPU against the host rule (dmel_codec_amd/utils/conceal.py: scan), bit for bit: the samples re-written in
place, the state rows compared as int32, and both output rows.  Row offsets on and off the 16-byte grid; a range at column 0 and
one that ends with the launch; a run a second launch continues; a launch cut inside a recovery; two runs closer than the recovery;
a run that fades out and mutes; an onset on a young session and one behind a wrap of the ring; sixteen ranges and two configs in
one launch; a launch of one sample; an idle item between two live ones.  Idle rows, the columns around an item's range and the
words behind a row's onsets carry sentinels."""
import pytest
import torch

from dmel_codec_amd.utils import conceal
from dmel_codec_amd.utils.conceal import ConcealConfig
from test_conceal_cpu import D, F, H, PMAX, RATE, W, voiced

pytestmark = pytest.mark.gpu

SENTINEL_WORD, SENTINEL_PERIOD, SENTINEL_SCORE, SENTINEL_SAMPLE, GUARD = 0x7FC00123, -77, -7.5, 3.0e38, 9
CFG = ConcealConfig()
OTHER = ConcealConfig(window_ms=10.0, min_period_ms=1.0, max_period_ms=8.0, hold_ms=2.0, fade_ms=6.0, recover_ms=1.0, floor=1e-6)


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
        self.state = torch.zeros(self.S, conceal.ROW_WORDS, dtype=torch.int32, device=dev)
        for s in idle:
            self.state[s] = SENTINEL_WORD
        self.idle = set(idle)
        self.ref = [conceal.fresh_state() for _ in range(self.S)]
        self.table = torch.empty(conceal.TABLE_WORDS * self.S, dtype=torch.int32, device=dev)
        self.out = [[] for _ in range(self.S)]

    def launch(self, pieces, ranges, first):
        """pieces[s]: the new samples of slot s (None or empty: idle), placed at column first[s] of its row between sentinels;
        ranges[s]: its lost ranges, whose content the device finds spoilt"""
        S = self.S
        n_new = [0 if p is None else int(p.shape[0]) for p in pieces]
        ranges = [list(r) if n else [] for r, n in zip(ranges, n_new)]
        width = max(f + n for f, n in zip(first, n_new)) + GUARD
        pitch = max(len(r) for r in ranges) + 2
        rows = torch.full((S, width), SENTINEL_SAMPLE, dtype=torch.float32)
        for s in range(S):
            if n_new[s]:
                spoilt = pieces[s].copy()
                for lo, hi in ranges[s]:
                    spoilt[lo:hi] = -5.0                                     # the content of a lost range is ignored
                rows[s, first[s]:first[s] + n_new[s]] = torch.from_numpy(spoilt)
        drows = rows.to(self.dev)
        per = torch.full((S, pitch), SENTINEL_PERIOD, dtype=torch.int32, device=self.dev)
        sc = torch.full((S, pitch), SENTINEL_SCORE, dtype=torch.float32, device=self.dev)
        conceal.conceal_items(drows, first, n_new, ranges, [c if n else None for c, n in zip(self.cfgs, n_new)], self.state, per, sc,
                              sample_rate=self.rate, table=self.table)
        got, state, per, sc = drows.cpu(), self.state.cpu(), per.cpu(), sc.cpu()
        for s in range(S):
            f, n = first[s], n_new[s]
            if n:
                y, self.ref[s], p, q = conceal.scan(pieces[s], ranges[s], self.cfgs[s], self.ref[s], self.rate)
                bad = (bits(got[s, f:f + n]) != bits(y)).nonzero().flatten().tolist()
                assert not bad, (s, n, f, bad[:8], got[s, f:f + n][bad[:8]].tolist(), y[bad[:8]].tolist())
                rows[s, f:f + n] = y
            else:
                p, q = torch.zeros(0, dtype=torch.int32), torch.zeros(0)
            assert torch.equal(bits(got[s]), bits(rows[s])), (s, n, f)          # the guard columns, and a whole idle row, unchanged
            B = p.shape[0]
            assert torch.equal(per[s, :B], p) and torch.equal(bits(sc[s, :B]), bits(q)), (s, n, per[s, :B].tolist(), p.tolist(), sc[s, :B], q)
            assert (per[s, B:] == SENTINEL_PERIOD).all() and (sc[s, B:] == SENTINEL_SCORE).all(), (s, n)
            if s in self.idle:
                assert (state[s] == SENTINEL_WORD).all(), s
            else:
                diff = (state[s] != self.ref[s]).nonzero().flatten().tolist()
                assert not diff, (s, n, diff[:8], state[s][diff[:8]].tolist(), self.ref[s][diff[:8]].tolist())
            self.out[s].append((p, q))


@pytest.mark.parametrize("first", [0, 1, 3, 4])
def test_ranges_at_both_ends_at_every_alignment(dev, first):
    """S = 3 with an idle middle item; a range at column 0 (a young session: zeros), one in the middle and one ending at n_new"""
    x, z = voiced(117.0, 3000, seed=first), voiced(211.7, 2500, seed=9)
    bank = Bank(dev, [CFG, CFG, CFG], idle=(1,))
    bank.launch([x, None, z], [[(0, 37), (1500, 1980), (2900, 3000)], [], [(2020, 2500)]], [first, first, first + 2])
    assert [p.tolist() for p, _ in bank.out[0]][0][0] == 0 and bank.out[0][0][0][1] > 0 and bank.out[2][0][0][0] > 0
    assert conceal.report(bank.state[0]).open and conceal.report(bank.state[0]).runs == 3


def test_a_second_launch_continues_a_run_and_a_cut_inside_a_recovery(dev):
    x = voiced(163.0, 5000)
    ranges = [(1500, 2300)]
    bank = Bank(dev, [CFG, CFG, CFG])
    # slot 0: one launch; slot 1: cut inside the run, then inside the recovery; slot 2: cut at the run's end
    bank.launch([x, x[:1800], x[:2300]], [ranges, [(1500, 1800)], [(1500, 2300)]], [2, 5, 0])
    assert int(bank.ref[1][conceal.I_PHASE]) == 1 and int(bank.ref[2][conceal.I_PHASE]) == 1
    bank.launch([None, x[1800:2350], x[2300:2301]], [[], [(0, 500)], []], [0, 3, 1])
    assert len(bank.out[1][1][0]) == 0                                      # the continued run is no onset
    assert int(bank.ref[1][conceal.I_PHASE]) == 2 and int(bank.ref[1][conceal.I_REC]) == F - 50
    assert int(bank.ref[2][conceal.I_REC]) == F - 1                         # n_new = 1: the first sample of a recovery
    bank.launch([None, x[2350:], x[2301:]], [[], [], []], [0, 1, 4])
    assert torch.equal(bank.ref[0], bank.ref[1]) and torch.equal(bank.ref[0], bank.ref[2])
    assert torch.equal(bank.state[0], bank.state[1]) and torch.equal(bank.state[0], bank.state[2])


def test_close_runs_a_long_run_a_young_onset_and_a_wrap(dev):
    x = voiced(87.3, 9000)
    close = [(3000, 3200), (3200 + F // 2, 3400), (3401, 3402)]              # the second and third begin inside a recovery
    long = [(2500, 4500)]                                                    # 2000 samples: hold, fade, mute
    young = [(W + PMAX - 1, W + PMAX + 200), (6000, 6100)]                   # no search one sample early; then one behind a wrap
    bank = Bank(dev, [CFG, CFG, CFG])
    bank.launch([x, x, x], [close, long, young], [1, 2, 3])
    assert conceal.report(bank.state[1]).muted_samples == 2000 - H - D and conceal.report(bank.state[1]).longest_run == 2000
    assert bank.out[2][0][0].tolist()[0] == 0 and bank.out[2][0][0].tolist()[1] > 0
    assert all(p > 0 for p in bank.out[0][0][0].tolist())
    # more than a ring's length in one launch, then an onset in the next: the ring holds the newest 4096 samples
    bank.launch([x[:5000], x[:4097], x[:1]], [[], [], []], [0, 1, 2])
    bank.launch([x[5000:6000], x[4097:5000], x[1:1000]], [[(100, 700)], [(0, 300)], [(998, 999)]], [3, 0, 1])


def test_sixteen_ranges_and_two_configs_in_one_launch(dev):
    x = voiced(297.0, 6000)
    sixteen = [(1000 + 250 * i, 1000 + 250 * i + 30 + 11 * i) for i in range(16)]
    assert OTHER.samples(RATE) == (240, 24, 192, 48, 144, 24)
    bank = Bank(dev, [CFG, OTHER, OTHER])
    bank.launch([x, x, x[:3000]], [sixteen, sixteen, [(500, 1500)]], [4, 1, 0])
    assert len(bank.out[0][0][0]) == 16 and len(bank.out[1][0][0]) == 16
    assert bank.out[0][0][0].tolist() != bank.out[1][0][0].tolist()          # another lag range finds other periods
    assert conceal.report(bank.state[2]).muted_samples == 1000 - 48 - 144
    bank.launch([x[:1], x[:1], x[:1]], [[(0, 1)], [], [(0, 1)]], [0, 3, 5])  # n_new = 1, lost
