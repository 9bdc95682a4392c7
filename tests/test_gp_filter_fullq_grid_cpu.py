"""The coverage proof of the GP-filter and full-covariance q(z) tile grid (tests/gp_filter_fullq_grid.py), without a GPU:
the rows of gp_tile_grid.ROWS reach every compiled leaf of gp_filter_kernel, gp_filter_bwd_kernel, gp_fullq_bwd_kernel and
gp_fullq_fwd_kernel, the long and slice cases meet the conditions of the host-side schedules they are there for, the random
mask exercises both branches of the conditioned epilogue in both chain groups -- and on every case the two CPU codings of
the references agree 100 times closer than the rules of tests/test_gp_filter_tile_grid_gpu.py and
tests/test_gp_fullq_tile_grid_gpu.py, so that those rules measure the kernels."""
import numpy as np
import pytest

import gp_filter_cases as fc
import gp_fullq_cases as fq
import gp_filter_fullq_grid as fg
import gp_tile_grid as gg

HEIGHTS = fg.dispatch_heights()
FAMILIES = ('filter', 'filter_bwd', 'fullq_bwd', 'fullq_fwd')


def test_launcher_families_list_the_same_leaves():
    """four families, one tree: the heights of CBF_FOR_EACH_GPBWD_NBLK times DK 2, 4, 6; trims in the forward filter only"""
    fam = fg.compiled_families()
    assert set(fam) == set(FAMILIES)
    assert len(HEIGHTS) >= 8 and len(set(HEIGHTS)) == len(HEIGHTS)
    for key, (heights, dks) in fam.items():
        assert heights == sorted(HEIGHTS), key
        assert dks == [2, 4, 6], key
        assert len(fg.compiled_leaves(key)) == 3 * len(HEIGHTS)
    trim_height, kts = fg.compiled_filter_trims()
    assert trim_height == 7 and kts == [-1, 0, 1, 2, 3]
    assert len(fg.compiled_filter_leaves()) == 3 * (len(HEIGHTS) - 1) + 3 * 5
    # the same tree as the kernels these are copies of
    assert fg.compiled_filter_leaves() == gg.compiled_rollout_leaves()
    assert all(fg.compiled_leaves(k) == gg.compiled_leaves() for k in FAMILIES)


def test_only_the_forward_filter_has_a_trim_level():
    for func in ('launch_gp_filt_bwd_n', 'launch_gp_fq_n', 'launch_gp_fq_fwd_n'):
        args = fg.launcher_template_arguments(func)
        assert sorted(args) == [('NBLK', '2'), ('NBLK', '4'), ('NBLK', '6')], (func, args)
    for name in ('cbfssm_gp_fullq.hpp', 'cbfssm_gp_fullq.hip'):
        text = fg.tg._read(name)
        assert 'trim_tiles' not in text and 'KT' not in text and '_fq_t' not in text and '_fq_fwd_t' not in text, name


def test_every_compiled_leaf_is_reached():
    assert fg.missing_leaves() == {}
    # and no row reaches something the source text does not list (the parser and the host agree)
    assert set(fg.reached()) <= fg.compiled_filter_leaves()
    trim_height, kts = fg.compiled_filter_trims()
    got = {(dk, kt) for nb, dk, kt in fg.reached() if nb == trim_height}
    assert len(got) == 15 and got == {(dk, kt) for dk in (2, 4, 6) for kt in kts}


def test_a_removed_row_is_noticed():
    """the proof has teeth: rows that are the only one at their leaf cannot leave unnoticed"""
    alone = [names[0] for names in fg.reached().values() if len(names) == 1]
    assert len(alone) >= 15                                    # every (DK, KT) of the trimmed height, at the least
    for name in alone:
        rest = [r for r in fg.ROWS if r[0] != name]
        assert fg.missing_leaves(rest), name
    two_d = {}
    for (nb, dk, _), names in fg.reached().items():
        two_d.setdefault((nb, dk), []).extend(names)
    for (nb, dk), names in two_d.items():
        rest = [r for r in fg.ROWS if r[0] not in names]
        miss = fg.missing_leaves(rest)
        assert all((nb, dk) in miss.get(k, ()) for k in ('filter_bwd', 'fullq_bwd', 'fullq_fwd', 'filter')), (nb, dk)


def test_derived_cases():
    for row in fg.ROWS:
        name, M, D, Do = row
        case = fg.filter_case(row)
        assert case == (M, D, Do, 21, 5, M % 2 == 1, Do % 2 == 1, (1.0, 1.3, 2.0)[M % 3], 'random'), name
        assert fg.fullq_case(row) == (M, D, Do, 37), name
    cases = [fg.filter_case(r) for r in fg.ROWS]
    assert {c[5] for c in cases} == {True, False} and {c[6] for c in cases} == {True, False}
    assert {c[7] for c in cases} == {1.0, 1.3, 2.0}
    assert fg.FULLQ_BWD_LONG == [(130, 6, 4, 4149), (300, 6, 4, 4101), (12, 4, 3, 16405), (24, 8, 8, 16407), (50, 9, 2, 8227),
                                 (100, 21, 14, 8249), (180, 6, 2, 4139), (250, 12, 6, 4173)]
    assert fg.FULLQ_FWD_LONG == [(12, 4, 3, 65573), (130, 6, 4, 16421), (50, 9, 2, 32805), (24, 8, 8, 65559),
                                 (99, 7, 5, 32825), (180, 6, 2, 16403), (250, 12, 6, 16445), (320, 12, 4, 16449)]
    assert fg.FULLQ_SLICE_ROWS == [(50, 9, 2, 277), (24, 8, 8, 643)]


@pytest.mark.parametrize('name', fg.ROW_IDS)
def test_random_mask_runs_both_branches_in_both_chain_groups(name):
    case = fg.filter_case(fg.ROW_BY_NAME[name])
    p, h0, a, ytilde, cond, eps, var_x, var_y, W = fc.make_inputs(*case)
    assert cond.shape == (5, 21) and set(np.unique(cond)) == {0.0, 1.0}
    frac = 1.0 - cond.mean()
    print('zero fraction of the mask %.3f' % frac)
    assert 0.2 <= frac <= 0.45
    for group in (cond[:, :16], cond[:, 16:]):
        assert np.any(group == 0.0) and np.any(group == 1.0)
    assert np.array_equal(np.isnan(ytilde), np.broadcast_to((cond == 0.0)[:, :, None], ytilde.shape))
    assert (var_x is not None) == case[6]


def test_restated_schedules_are_the_source_texts():
    s = fg.source_schedules()
    (b1, c1), (b2, c2), c3 = s['maxwg']
    for nb in HEIGHTS:
        assert gg.max_workgroups(nb) == (c1 if nb <= b1 else (c2 if nb <= b2 else c3)), nb
        assert fg.fullq_bwd_cap(nb) == s['bwd_cap'] * gg.max_workgroups(nb)
        assert fg.fullq_fwd_cap(nb) == s['fwd_cap'] * gg.max_workgroups(nb)
    assert s['bwd_cap'] == 1 and s['fwd_cap'] == 4
    assert s['slices'] == (16, 1, 8) and s['per'] == '(nblocks + ns - 1) / ns'
    step, lo, hi = s['slices']
    for n in list(range(1, 200)) + [601, 1027, 4099]:
        ns, per = fg.fq_slices(n)
        assert ns == min(max(-(-n // step), lo), hi) and per == -(-n // ns)
        sizes = fg.slice_sizes(n)
        assert len(sizes) == ns and sum(sizes) == n and min(sizes) >= 1, n      # no slice is empty, none runs past the end


def test_long_rows_go_round_the_persistent_loops_twice():
    for rows, cap_of in ((fg.FULLQ_BWD_LONG, fg.fullq_bwd_cap), (fg.FULLQ_FWD_LONG, fg.fullq_fwd_cap)):
        caps = set()
        for M, D, Do, npts in rows:
            nb, _, _ = fg.leaf_key(M, D, Do)
            blocks, cap = (npts + 15) // 16, cap_of(nb)
            assert cap < blocks <= 2 * cap, (M, npts, blocks, cap)
            assert npts % 16 != 0
            caps.add((gg.max_workgroups(nb), nb > 7))
        assert sum(stash for _, stash in caps) >= 1, 'a stash height among each long set'
        assert {c for c, _ in caps} >= {1024, 256}
        # one long case at every tile height; the rows after the first three by the rule npts = 16 (cap + k) + r
        assert gg.long_heights(rows) == sorted(HEIGHTS)
        for M, D, Do, npts in rows[3:]:
            k, r = gg.long_k_r(npts, cap_of(fg.leaf_key(M, D, Do)[0]))
            assert 1 <= k <= 4 and 1 <= r <= 15, (M, npts, k, r)
            assert M < 113 or D >= 6, (M, D)
            cond = gg.kmm_condition(M, D, Do)
            print('%s cond_2(K_mm + jitter I) %.3e' % ((M, D, Do, npts), cond))
            assert cond <= 1e5, (M, D, Do, cond)               # (the bound the rows of gp_tile_grid.ROWS keep)
        # the three rows each table had before: 2.5e3, 59 and, at (300, 6, 4) of FULLQ_BWD_LONG alone, 1.6e5 (below 1e6)
        assert all(gg.kmm_condition(*r[:3]) < 1e6 for r in rows[:3])
    assert {fg.fullq_fwd_cap(fg.leaf_key(*r[:3])[0]) for r in fg.FULLQ_FWD_LONG} == {4096, 1024, 2048}
    assert {fg.fullq_bwd_cap(fg.leaf_key(*r[:3])[0]) for r in fg.FULLQ_BWD_LONG} == {1024, 512, 256}
    # no other full-q case of the suite exceeds the forward cap, and the only one above the backward cap is at NBLK 7
    for M, D, Do, npts in fq.CASES:
        nb = fg.leaf_key(M, D, Do)[0]
        assert (npts + 15) // 16 <= fg.fullq_fwd_cap(nb)
        assert (npts + 15) // 16 <= fg.fullq_bwd_cap(nb) or nb == 7


def test_slice_rows_sum_in_two_and_in_three_slices():
    seen = {}
    for M, D, Do, npts in fg.FULLQ_SLICE_ROWS:
        blocks = (npts + 15) // 16
        ns, per = fg.fq_slices(blocks)
        sizes = fg.slice_sizes(blocks)
        assert ns in (2, 3) and (len(set(sizes)) > 1 or npts % 16 != 0), (npts, sizes)
        seen[ns] = (blocks, per, sizes)
    assert seen == {2: (18, 9, [9, 9]), 3: (41, 14, [14, 14, 13])}
    # what the other cases have: one slice or eight
    for M, D, Do, npts in list(fq.CASES) + [fg.fullq_case(r) for r in fg.ROWS]:
        assert fg.fq_slices((npts + 15) // 16)[0] in (1, 8)


def test_chain_group_rows_have_auxiliary_inputs():
    for n in fg.CHAIN_GROUP_ROWS:
        _, M, D, Do = fg.ROW_BY_NAME[n]
        assert D > Do and fg.N_CHAINS > 16


# ---- the references alone
def _agree(name, x, r, tol):
    scale = np.abs(r).max()
    err = np.abs(x - r).max() / scale
    print('%-34s max|ref| %.3e  codings differ by %.2e of it' % (name, scale, err))
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(r)) and scale > 0.0 and err < tol, (name, err)
    return scale


def _check_fullq(case):
    """fq.reference against fq.reference2, 100 times inside the GPU rules; every gradient tensor carries signal, except the
    two that are exactly zero at M = 1"""
    M = case[0]
    ref, sec = fq.reference(*case), fq.reference2(*case)
    _agree('fmean', sec['fmean'], ref['fmean'], 1e-10)
    _agree('fvar', sec['fvar'], ref['fvar'], 1e-10)
    assert ref['fvar'].min() > 0.0, ref['fvar'].min()
    print('min fvar %.3e  kl %.6e' % (ref['fvar'].min(), ref['kl']))
    assert abs(sec['kl'] - ref['kl']) < 1e-11 * abs(ref['kl'])
    assert _agree('loss: X', sec['g_X'], ref['g_X'], 1e-8) > 1e-3
    zeros = fg.kl_zero_names(M)
    for k in fq.PARAMS:
        assert _agree('loss: ' + k, sec['g_' + k], ref['g_' + k], 1e-8) > 1e-3, k
        if k in zeros:
            assert not np.any(ref['k_' + k]) and not np.any(sec['k_' + k]), k
        else:
            assert _agree('prior_kl alone: ' + k, sec['k_' + k], ref['k_' + k], 1e-8) > 1e-3, k
    # nothing flows into the entries above the diagonal of q
    upper = np.triu(np.ones((M, M), dtype=bool), 1)
    assert not np.any(ref['g_zeta_sqrt'][:, upper]) and not np.any(ref['k_zeta_sqrt'][:, upper])


@pytest.mark.parametrize('name', fg.ROW_IDS)
def test_reference_alone_stays_inside_the_tolerances(name):
    """Reference and second coding agree 100 times inside the rules: trajectory, fmean and fvar to 1e-10 of the largest
    entry, kl to 1e-11 relative, every gradient tensor to 1e-8 of its largest entry.  No gradient tensor's largest entry is
    below 1e-3 (the 1e-6 rule then still resolves 1e-9 absolute), kl > 1 on the filter, min fvar > 0."""
    row = fg.ROW_BY_NAME[name]
    case = fg.filter_case(row)
    ref, sec = fc.reference(case), fc.evaluate(case, 'second')
    fc.traj_rule('traj', sec['traj'], ref['traj'], tol=1e-10)
    fc.kl_rule(sec['kl'], ref['kl'], tol=1e-11)
    assert ref['kl'] > 1.0
    names, zeros = fc.grad_names(case)
    assert not zeros and set(names) >= {'h0', 'a', 'ytilde', 'var_y'} | set(fc.PARAMS) and ('var_x' in names) == case[6]
    for k in names:
        if ref['g_' + k].size:
            assert _agree('filter: ' + k, sec['g_' + k], ref['g_' + k], 1e-8) > 1e-3, k
    p, h0, a, ytilde, cond, eps, var_x, var_y, W = fc.make_inputs(*case)
    assert not np.any(ref['g_ytilde'][cond == 0.0]) and np.all(np.isfinite(ref['g_ytilde']))
    _check_fullq(fg.fullq_case(row))


@pytest.mark.parametrize('case', fg.FULLQ_BWD_LONG + fg.FULLQ_FWD_LONG + fg.FULLQ_SLICE_ROWS, ids=str)
def test_long_and_slice_references_alone_stay_inside_the_tolerances(case):
    _check_fullq(case)
