"""The backward-run schedule (cbfssm_bwd_schedule, host only): the chunk table of the backward-run adjoint covers exactly
the live steps of both runs, once each, in whole resample-to-resample segments, longest chunk first.

Liveness is derived here from the reference's two conditions (cbfssm/model/cbfssm.py:123-128), not from the library: run r
(0 or 1) walks t = T-1 .. 0, resamples its hidden state where (t + 1 + r R) mod 2R == 0 and writes y2 at t where
t mod 2R < R (run 0) or >= R (run 1).  A step is live if its segment (the steps from one resample down to the next)
still has a written step at or below it: everything a step computes flows downwards in t and ends at the next resample."""
import ctypes as C
import heapq

import pytest

from cbfssm.hip import lib

CAP = 32
UNITS = 256          # one adjoint workgroup per CU of the MI355X


def _problem(T, R, B, S, group0=0, ngroups=0):
    p = lib.make_problem(B, S, T, 4, 1, 2, 20, R, 1.0, True)
    p.group0, p.ngroups = group0, ngroups
    return p


def _table(p):
    arr = [(C.c_int * CAP)() for _ in range(3)]
    n = lib.load().cbfssm_bwd_schedule(C.byref(p), CAP, *arr)
    assert 0 <= n <= CAP, lib.load().cbfssm_last_error()
    assert lib.load().cbfssm_bwd_schedule(C.byref(p), 0, None, None, None) == n
    return [(arr[0][i], arr[1][i], arr[2][i]) for i in range(n)]


def _live_and_starts(T, R):
    """per run: the set of live steps and the set of segment starts (lowest step of a segment), from cbfssm.py:123-128"""
    P = 2 * R
    live, starts = [set(), set()], [set(), set()]
    for run in (0, 1):
        written = lambda t: (t % P < R) if run == 0 else (t % P >= R)
        resample = lambda t: (t + 1 + run * R) % P == 0
        for t in range(T):
            if t == 0 or resample(t - 1):
                starts[run].add(t)
            # the segment of t reaches down to its start: the first s <= t with s == 0 or a resample at s - 1
            s = t
            while not (s == 0 or resample(s - 1)):
                s -= 1
            if any(written(q) for q in range(s, t + 1)):
                live[run].add(t)
    return live, starts


def _check_table(T, R, B, S):
    p = _problem(T, R, B, S)
    tab = _table(p)
    live, starts = _live_and_starts(T, R)
    seen = [set(), set()]
    for run, tb, ns in tab:
        assert run in (0, 1) and ns >= 1 and 0 <= tb and tb + ns <= T, (T, R, tab)
        steps = set(range(tb, tb + ns))
        assert not (steps & seen[run]), ('step listed twice', T, R, tab)
        seen[run] |= steps
        assert tb in starts[run], ('chunk does not begin on a segment start', T, R, tab)
        assert tb + ns == T or (tb + ns) in starts[run], ('chunk does not end on a segment end', T, R, tab)
    assert seen == live, (T, R, tab)
    ns = [e[2] for e in tab]
    assert ns == sorted(ns, reverse=True), (T, R, tab)
    # the tail is single segments: the last entry of each run holds no segment start but its own
    for run in (0, 1):
        mine = [e for e in tab if e[0] == run]
        if mine:
            _, tb, n = mine[-1]
            assert not (starts[run] & set(range(tb + 1, tb + n))), (T, R, tab)
        assert len(mine) <= 16
    groups = (B * S + 15) // 16
    assert lib.load().cbfssm_rev_workgroups(C.byref(p), 1) == groups * len(tab)
    assert lib.load().cbfssm_rev_workgroups(C.byref(p), 0) == groups
    return tab


@pytest.mark.parametrize('R', [1, 2, 3, 4, 5])
def test_table_covers_the_live_steps_once(R):
    for T in range(1, 71):
        tab = _check_table(T, R, 3, 7)
        if T <= R:
            assert all(run == 0 for run, _, _ in tab)             # run 1 has no live step
        else:
            assert min(tb for run, tb, _ in tab if run == 1) == R   # run 1 starts at t = R


def test_table_does_not_depend_on_the_chain_group_range():
    for T, R, B, S in ((23, 2, 3, 7), (41, 4, 5, 11), (250, 16, 256, 20)):
        groups = (B * S + 15) // 16
        ref = _table(_problem(T, R, B, S))
        for g0, ng in ((0, 1), (1, groups - 1), (0, groups), (groups // 2, groups - groups // 2)):
            assert _table(_problem(T, R, B, S, g0, ng)) == ref


def test_c3_table_is_within_two_percent_of_the_ideal_packing():
    """C3 (T=250, R=16, 5120 chains = 320 chain groups): a greedy list schedule of the table on 256 workgroup slots, one step
    a unit of time, against live steps x 320 / 256 (the two-equal-chunks-per-run split this table replaced: 4.6 % over)."""
    T, R, B, S = 250, 16, 256, 20
    tab = _check_table(T, R, B, S)
    groups = (B * S + 15) // 16
    assert groups == 320
    free = [0] * UNITS
    for _, _, ns in tab:
        for _ in range(groups):
            heapq.heappush(free, heapq.heappop(free) + ns)
    makespan = max(free)
    live = sum(ns for _, _, ns in tab)
    assert live == 250 + 234
    ideal = live * groups / UNITS
    print('C3 table', tab, 'makespan', makespan, 'ideal', ideal)
    assert makespan <= 1.02 * ideal, (makespan, ideal, tab)
