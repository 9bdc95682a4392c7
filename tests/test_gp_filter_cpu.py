"""Host-side checks of the GP filter loop (no GPU): the reference of tests/gp_filter_cases.py is fit to measure the kernels
by (two CPU codings agree 100 times tighter than the rules, no gradient tensor is so small that its rule is vacuous, kl is
well away from 0 wherever a step conditions), and the new entry points are declared, exported and bound."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gp_filter_cases as fc
from gp_filter_cases import CASES, PARAMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = ('cbfssm_gp_filter_partials', 'cbfssm_gp_filter_bwd_workgroups', 'cbfssm_gp_filter_bwd_work_elems')
CALLS = ('cbfssm_gp_filter_f64', 'cbfssm_gp_filter_bwd_f64')


def test_cases_cover_what_the_kernels_dispatch_on():
    def nblk(M):
        return min(n for n in (1, 2, 4, 7, 10, 13, 16, 20) if 16 * n >= M)
    assert {nblk(c[0]) for c in CASES} == {1, 2, 4, 7, 10, 13, 16, 20}
    assert {(c[1] + 7) // 8 * 2 for c in CASES} == {2, 4, 6}                         # DK
    assert (112, 24, 16) in {c[:3] for c in CASES} and 113 in {c[0] for c in CASES}
    assert any(c[3] < 16 for c in CASES) and any(c[3] > 16 and c[3] % 16 for c in CASES)
    assert any(c[1] == c[2] for c in CASES) and any(c[4] == 1 for c in CASES)
    assert any(c[4] == 40 and c[0] <= 32 for c in CASES)
    assert {c[5] for c in CASES} == {True, False} and any(not c[6] for c in CASES)
    assert sum(c[7] != 1.0 for c in CASES) >= 3
    assert {c[8] for c in CASES} == {'ones', 'zeros', 'prefix', 'random'}
    for c in CASES:
        p, h0, a, ytilde, cond, eps, var_x, var_y, W = fc.make_inputs(*c)
        if c[8] == 'random':
            frac = 1.0 - cond.mean()
            assert 0.2 < frac < 0.45 and np.all(np.isnan(ytilde[cond == 0.0])) and np.all(np.isfinite(ytilde[cond == 1.0]))
        else:
            assert np.all(np.isfinite(ytilde))


@pytest.mark.parametrize('case', CASES, ids=str)
def test_two_cpu_codings_agree_100_times_tighter_than_the_rules(case):
    r1, r2 = fc.reference(case), fc.evaluate(case, 'second')
    assert np.all(np.isfinite(r1['traj']))
    fc.traj_rule('traj', r2['traj'], r1['traj'], tol=1e-10)
    fc.kl_rule(r2['kl'], r1['kl'], tol=1e-11)
    names, zeros = fc.grad_names(case)
    for k in names:
        if r1['g_' + k].size:
            fc.within_rule(k, r2['g_' + k], r1['g_' + k], rtol=1e-8)
    for k in zeros:
        assert not np.any(r1['g_' + k]) and not np.any(r2['g_' + k]), k
    # missing data: no gradient flows into a masked-out pseudo-observation, and none is NaN
    p, h0, a, ytilde, cond, eps, var_x, var_y, W = fc.make_inputs(*case)
    if cond is not None:
        assert not np.any(r1['g_ytilde'][cond == 0.0])
    assert all(np.all(np.isfinite(r1['g_' + k])) for k in fc.GRADS + PARAMS if 'g_' + k in r1)


def test_no_gradient_rule_is_vacuous_and_kl_is_well_away_from_zero():
    smallest, kl_min = np.inf, np.inf
    for case in CASES:
        ref = fc.reference(case)
        names, _ = fc.grad_names(case)
        for k in names:
            if ref['g_' + k].size:
                smallest = min(smallest, np.abs(ref['g_' + k]).max())
        if case[8] == 'zeros':
            assert ref['kl'] == 0.0
        else:
            kl_min = min(kl_min, ref['kl'])
    print('smallest largest-entry of a gradient tensor: %.3e; smallest kl: %.3e' % (smallest, kl_min))
    # the rule is 1e-6 of the largest entry: at 1e-3 it still resolves 1e-9 absolute, seven orders above double rounding
    assert smallest > 1e-3
    # every term of kl is >= 0 (no cancellation) and a conditioned entry adds O(0.1) or more: the 1e-9 relative rule is a
    # rule on at least nine digits of a number of order 1 or larger
    assert kl_min > 1.0


def test_new_symbols_are_declared_exported_and_bound():
    from cbfssm.hip import lib
    text = open(os.path.join(ROOT, 'include', 'cbfssm_hip.h')).read()
    declared = set(re.findall(r'\b(cbfssm_[a-z0-9_]+)\s*\(', text))
    so = C.CDLL(lib.LIB_PATH)
    for name in COUNTS + CALLS:
        assert name in declared and name in lib.SYMBOLS and hasattr(so, name), name
    l = lib.load()
    vp, i64, ip, dbl = C.c_void_p, C.c_int64, C.c_int, C.c_double
    lay = C.POINTER(lib.PackLayout)
    for name in CALLS:
        assert getattr(l, name).restype is C.c_int, name
    for name in COUNTS:
        assert getattr(l, name).restype is i64, name
    assert l.cbfssm_gp_filter_partials.argtypes == [lay, i64] and l.cbfssm_gp_filter_bwd_workgroups.argtypes == [lay, i64]
    assert l.cbfssm_gp_filter_bwd_work_elems.argtypes == [lay, i64, i64]
    # layout, pack, h0, a, ytilde, cond, eps, var_x, var_y | k_factor | N, T, reverse | traj, msave, vsave, kl_part, stream
    assert l.cbfssm_gp_filter_f64.argtypes == [lay] + [vp] * 8 + [dbl, i64, i64, ip] + [vp] * 5
    # layout, pack, h0, a, ytilde, cond, eps, var_y | k_factor | traj, msave, vsave, gtraj, g_kl | N, T, reverse |
    # gh0, ga, gytilde, gpart, work, gB_image, stream
    assert l.cbfssm_gp_filter_bwd_f64.argtypes == [lay] + [vp] * 7 + [dbl] + [vp] * 5 + [i64, i64, ip] + [vp] * 7
    # each declaration cites the reference lines it replaces
    for name in COUNTS + CALLS:
        at = text.index(name + '(const cbfssm_pack_layout')
        assert 'cbfssm.py:185-237' in text[at:text.index('\n', text.index(';', at))], name


def test_counts_and_refusals_without_a_device():
    from cbfssm.hip import lib
    l = lib.load()
    for (M, D, Do) in ((12, 4, 3), (100, 21, 14), (113, 9, 1), (300, 6, 4)):
        lay = lib.pack_layout(M, D, Do)
        for N in (0, 1, 16, 17, 5120):
            groups = (N + 15) // 16
            assert l.cbfssm_gp_filter_partials(C.byref(lay), N) == groups
            assert l.cbfssm_gp_filter_bwd_workgroups(C.byref(lay), N) == groups
            for T in (0, 1, 64):
                assert l.cbfssm_gp_filter_bwd_work_elems(C.byref(lay), N, T) == l.cbfssm_gp_rollout_bwd_work_elems(C.byref(lay), N, T)
    lay = lib.pack_layout(300, 6, 4)
    assert l.cbfssm_gp_filter_bwd_work_elems(C.byref(lay), 2 ** 20, 2 ** 10) > 2 ** 32
    good = lib.pack_layout(100, 21, 14)
    one = C.c_void_p(8)                              # a non-null address that is never dereferenced: every call below fails first

    def fwd(lay, N, T, ptr=None, msave=None):
        return l.cbfssm_gp_filter_f64(lay, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, 1.0, N, T, 0, ptr, msave, ptr, ptr, None)

    def bwd(lay, N, T, ptr=None):
        return l.cbfssm_gp_filter_bwd_f64(lay, ptr, ptr, ptr, ptr, ptr, ptr, ptr, 1.0, ptr, ptr, ptr, ptr, ptr, N, T, 0,
                                          ptr, ptr, ptr, ptr, ptr, ptr, None)

    for field, value in (('M', 321), ('D', 25), ('Do', 17), ('M', 0), ('NBLK', 3), ('gp_form', 7)):
        bad = lib.pack_layout(100, 21, 14)
        setattr(bad, field, value)
        assert l.cbfssm_gp_filter_partials(C.byref(bad), 37) == -1 and l.cbfssm_gp_filter_bwd_workgroups(C.byref(bad), 37) == -1
        assert l.cbfssm_gp_filter_bwd_work_elems(C.byref(bad), 37, 8) == -1
        assert fwd(C.byref(bad), 37, 8, one, one) == -3 and bwd(C.byref(bad), 37, 8, one) == -3
    assert fwd(C.byref(good), -1, 8, one, one) == -1 and fwd(C.byref(good), 37, 0, one, one) == -1
    assert bwd(C.byref(good), -1, 8, one) == -1 and bwd(C.byref(good), 37, 0, one) == -1
    assert fwd(C.byref(good), 2 ** 30 + 1, 8, one, one) == -3 and bwd(C.byref(good), 37, 2 ** 24 + 1, one) == -3
    assert fwd(C.byref(good), 37, 8) == -1 and b'null' in l.cbfssm_last_error()
    assert bwd(C.byref(good), 37, 8) == -1 and b'null' in l.cbfssm_last_error()
    assert fwd(C.byref(good), 37, 8, one, None) == -1 and b'together' in l.cbfssm_last_error()      # msave without vsave
    assert fwd(None, 37, 8, one, one) == -1 and bwd(None, 37, 8, one) == -1


def test_python_surface():
    from cbfssm.hip import autograd
    from cbfssm.model import gp_tf
    assert callable(autograd.gp_filter) and callable(autograd.gp_filter_eval)
    assert hasattr(gp_tf.GPModel, 'filter') and 'cbfssm.py:185-237' in gp_tf.GPModel.filter.__doc__
