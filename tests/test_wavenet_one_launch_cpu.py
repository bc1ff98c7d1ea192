"""What tests/test_gpu_wavenet_one_launch_matrix.py rests on, checked without a GPU: the covering properties of its case tables (a later
edit cannot thin them silently), the recorded reference ratio R its per-row tolerance is a multiple of, and the condition that lets
every output row take part in that bound."""
import collections
import itertools

import torch

import test_gpu_wavenet_one_launch_matrix as M

CS = (33, 47, 48, 49, 63, 64, 65, 70, 79, 80)
CINS = (None, 1, 8, 9, 10, 16)
LS = (1, 2, 3, 4, 5, 20)
CYCLES = (0, 1, 2, 3, 4)
TS = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96)


def test_whole_sequence_table_covers_what_it_promises():
    cases = M.CASES
    assert 45 <= len(cases) <= 55 and len(set(cases)) == len(cases)
    for idx, values in enumerate((CS, CINS, LS, CYCLES, TS)):
        seen = collections.Counter(c[idx] for c in cases)
        assert set(seen) == set(values), (idx, sorted(seen, key=str))
        assert min(seen.values()) >= 2, (idx, seen)                 # every value of every factor at least twice
    # every (chunk count, T block class) pair; every width in every T block class; depth 1 and 2 with every cycle
    assert {(M.chunks(c), M.t_class(t)) for c, _, _, _, t in cases} == set(itertools.product((3, 4, 5), (0, 1, 2)))
    assert {(c, M.t_class(t)) for c, _, _, _, t in cases} == set(itertools.product(CS, (0, 1, 2)))
    assert {(l, cyc) for _, _, l, cyc, _ in cases if l <= 2} == set(itertools.product((1, 2), CYCLES))
    assert [M.t_class(t) for t in (32, 33, 64, 65, 96)] == [0, 1, 1, 2, 2]
    assert {c % 4 for c in CS} == {0, 1, 2, 3} and {M.chunks(c) for c in CS} == {3, 4, 5}
    # all of them inside the predicate
    assert all(M.eligible(c, cin, None, False, cyc) and t <= M.MAX_T for c, cin, _, cyc, t in cases)


def test_lengths_of_the_table_reach_every_kind():
    kinds = collections.Counter()
    for i, (_, _, _, _, T) in enumerate(M.CASES):
        assert M.case_lengths(i, "none") == (None, None)
        il, ol = M.case_lengths(i, "equal")
        assert il == ol and len(il) * M.GROUP == M.N_ITEMS
        il, ol = M.case_lengths(i, "differ")
        assert il != ol, (i, il, ol)
        for mode in ("equal", "differ"):
            ik, ok = M.case_length_kinds(i, mode)
            kinds.update(ik)
            kinds.update(ok)
            assert all(v in (0, 1, T // 2, T - 1, T, T + 5) for v in sum(M.case_lengths(i, mode), []))
    assert set(kinds) == set(M.LEN_KINDS)
    assert kinds["0"] >= 6 and kinds["T+5"] >= 6, kinds
    assert M.length_of("T+5", 96) == 101 and M.length_of("0", 96) == 0


def test_dispatch_edges_lie_one_step_outside_the_predicate():
    assert set(M.EDGES) == {"C32", "C81", "T97", "Cin17", "cycle5", "condition8", "output20"}
    assert all(M.edge_is_outside(name) for name in M.EDGES)
    # ... and one step only: the neighbour on the inside is eligible
    assert M.eligible(33, 10, None, False, 4) and M.eligible(80, 16, None, False, 4) and M.eligible(70, None, None, False, 0)
    assert not M.eligible(70, 10, 8, False, 4) and not M.eligible(70, 10, None, True, 4)
    kw, T = M.EDGES["T97"]
    assert M.eligible(kw["C_res"], kw["Cin"], None, False, kw["cycle"]) and T == M.MAX_T + 1


def test_streaming_table_covers_what_it_promises():
    stacks = M.STREAM_STACKS
    assert {s[0] for s in stacks} == {33, 47, 49, 65, 79, 80}
    assert {(s[2], s[3]) for s in stacks} == {(1, 0), (2, 1), (3, 2), (5, 3), (20, 4), (32, 4)}
    cin = collections.Counter(s[1] for s in stacks)
    assert set(cin) == {None, 1, 9, 16} and min(cin.values()) >= 2, cin
    assert all(M.eligible(c, i, None, False, cyc) and l <= M.MAX_STREAM_L for c, i, l, cyc in stacks)
    assert (M.N_ITEMS, M.GROUP, M.STREAM_CAP, M.STREAM_T, M.STREAM_LENS) == (4, 2, 256, 230, [230, 181])
    assert M.PUSHES == (1, 96, 97, 7, 8) and M.SUBSTEP == 96
    for variant in (0, 1):
        ops = M.plain_ops(variant)
        assert ops.index("rebase") == 4 and ops[-1] == (M.STREAM_T, True) and ops[-2][0] == M.STREAM_T
    # the per-item schedule: rows of three different block counts in one launch, an idle row in every second step, one re-based row
    queues = [M.utterance_ops(r) for r in range(3)]
    assert all(op is None for op in queues[2][0::2]) and all(op is not None for op in queues[2][1::2])
    assert "rebase" in queues[0] and all("rebase" not in q for q in queues[1:])
    assert queues[1][-2:] == [(M.STREAM_T, False), (M.STREAM_T, True)]


def reference_figures():
    """-> (largest per-row ratio of the float32 oracle against the float64 one, smallest row maximum / global maximum) over CASES x MODES"""
    worst, floor = 0.0, 1.0
    for i in range(len(M.CASES)):
        for mode in M.MODES:
            _, ol = M.case_lengths(i, mode)
            y64 = M.case_reference(i, mode)
            y32 = M.case_reference(i, mode, torch.float32)
            r, f = M.row_ratio(y32, y64, ol)
            worst, floor = max(worst, r), min(floor, f)
    return worst, floor


def test_reference_ratio_does_not_exceed_the_recorded_one():
    """oracle.ref_cpu.wavenet_forward in float32 against float64, per (item, channel) row, over every run of the whole-sequence table: not
    above the recorded R the kernel's tolerance is a multiple of (nor below half of it: a stale constant), and no row's max |y64| below
    ROW_FLOOR of its run's global maximum, so that no row is left out.  Measured: R 1.171e-6, smallest row / global maximum 0.372.  (CPU.)"""
    worst, floor = reference_figures()
    print(f"R measured {worst:.3e}, recorded {M.R:.2e}, tolerance {M.ROW_TOL:.2e}; smallest row maximum / global maximum {floor:.3f}")
    assert 0.5 * M.R <= worst <= M.R, (worst, M.R)
    assert M.ROW_TOL == min(M.FACTOR * M.R, M.TOL) and M.FACTOR == 8
    assert floor >= M.ROW_FLOOR, floor
