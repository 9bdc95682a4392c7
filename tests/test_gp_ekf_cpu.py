"""GPModel.ekf without a GPU: the two CPU references of tests/gp_ekf_cases.py -- (a) the oracle's predict, Jacobians by
autodiff, the joint Kalman update and slogdet; (b) the closed form through an explicit inverse and the sequential scalar
updates -- agree to 1e-9 of the largest entry on means, covs and loglik for EVERY case the GPU tests use, ten times inside the
1e-8 rule of tests/test_gp_ekf_gpu.py; and every row of gp_tile_grid.ROWS reaches a leaf the EKF launcher instantiates.

Measured here, (a) against (b), worst of means / covs / loglik: at most 1.7e-11 over the 36 grid rows (at (257, 6, 3), where
max |P| is 78), 1.1e-11 at (30, 7, 5), T = 40 under the random mask and 5.6e-14 under the all-zero mask (max |P| 780), at most
4.3e-13 on the other mask and edge cases; the smallest eigenvalue of any reference covariance is 1.7e-2.  The whole file
takes about six seconds."""
import re

import numpy as np
import pytest

import gp_ekf_cases as ec
import gp_tile_grid as gg
import tile_grid as tg

FLOOR = 1e-9


@pytest.mark.parametrize('c', ec.ALL_GPU_CASES, ids=str)
def test_the_two_references_agree(c):
    ag = ec.agreement(c)
    lo, scale = ec.min_eig(c)
    print('%s (a) against (b): %s  min eig %.2e  max |P| %.2e' % (c, {k: '%.1e' % v for k, v in ag.items()}, lo, scale))
    assert all(np.isfinite(v) and v <= FLOOR for v in ag.values()), (c, ag)
    assert lo > 0.0, (c, lo)                               # the reference covariances are positive definite
    ref = ec.reference_joint(c)
    assert np.all(np.isfinite(ref['means'])) and np.all(np.isfinite(ref['covs'])) and np.all(np.isfinite(ref['loglik']))
    if c[6] == 'zeros':
        assert np.all(ref['loglik'] == 0.0)
    else:
        assert np.abs(ref['loglik']).max() > 0.0


def test_the_cases_cover_what_the_gpu_tests_name():
    cases = ec.MASK_CASES + ec.EDGE_CASES
    assert {c[6] for c in ec.MASK_CASES} == {'ones', 'zeros', 'prefix', 'random'}
    assert any(not c[7] for c in cases) and any(not c[8] for c in cases)            # var_x None, P0 None
    assert any(c[1] == c[2] for c in cases) and any(c[5] == c[2] > 1 for c in cases)   # a None, Dy == Do
    assert any(c[2] == 1 for c in cases)
    assert {c[3] for c in cases} >= {1, 16, 17, 21} and {c[4] for c in cases} >= {1, 40}
    assert any(c[:3] == (20, 19, 6) for c in cases)
    for c in ec.GRID_CASES:
        assert c[3:] == (21, 5, max(1, c[2] // 2), 'random', True, True)
    # a random mask conditions and skips in every grid case, and y is NaN exactly where it skips
    for c in ec.GRID_CASES:
        i = ec.make_inputs(c)
        assert 0 < i['cond'].sum() < i['cond'].size
        assert np.array_equal(np.isnan(i['y']).all(axis=2), i['cond'] == 0) and not np.isnan(i['y'][i['cond'] != 0]).any()
    nbs = sorted(gg.leaf_key(*s)[0] for s in ec.CHAIN_GROUP_SHAPES)
    assert len(nbs) == 2 and nbs[0] <= 7 < nbs[1]


def test_the_ill_conditioned_candidates():
    """(130, 3, 2) of gp_linearize_cases.ILL_CASES stays only if (a) and (b) agree ten times inside the 1e-6 rule, i.e. to
    1e-7; measured 8.1e-8 (means), 1.1e-7 (covs), 3.0e-8 (loglik) with max |P| 1.6e6, so the GPU file runs no
    ill-conditioned case.  The figure is printed, not asserted against 1e-7 (it sits 10 % from it); what is asserted is that
    the references are still inside the 1e-6 rule itself, i.e. that the verdict is about their precision and not a bug.
    (64, 2, 3) has D < Do: no transition exists for it."""
    ag = ec.agreement(ec.ILL_CANDIDATE)
    print('%s (a) against (b): %s; keep criterion %.0e' % (ec.ILL_CANDIDATE, ag, ec.ILL_KEEP))
    assert all(np.isfinite(v) and v < 1e-6 for v in ag.values()), ag
    M, D, Do = ec.ILL_REFUSED
    assert D < Do


# ---- the compiled tree of the EKF launcher, from the source text
def _compiled():
    text = tg._read('cbfssm_gp_ekf.hpp')
    return gg._instantiated('CBF_GPEKF_INSTANTIATE'), gg._case_values(text, 'launch_gp_ekf_n')


def test_every_row_of_the_grid_reaches_a_compiled_leaf_of_the_ekf():
    heights, dks = _compiled()
    assert heights == sorted(gg.dispatch_heights()) and dks == [2, 4, 6]
    host = tg._read('cbfssm_gp_ekf.hip')
    assert re.search(r'#define X\(NB\) case NB: return launch_gp_ekf_nb##NB\([^\n]*\n\s*CBF_FOR_EACH_GPBWD_NBLK\(X\)', host)
    body = gg._body(tg._read('cbfssm_gp_ekf.hpp'), 'launch_gp_ekf_n')
    assert len(re.findall(r'launch_gp_ekf_k<NBLK, \d+>', body)) == len(dks)
    leaves = {(nb, dk) for nb in heights for dk in dks}
    got = {gg.leaf_key(M, D, Do)[:2] for _, M, D, Do in gg.ROWS}
    assert got == leaves, (sorted(leaves - got), sorted(got - leaves))
    assert len(leaves) == 24


def test_the_lds_budget_is_asserted():
    text = tg._read('cbfssm_gp_ekf.hpp')
    geom = text[text.index('struct GpEkfGeom'):]
    geom = geom[:geom.index('};')]
    assert re.search(r'static_assert\(LDS_DOUBLES <= 163840 / 8', geom)
    # the layout restated: 16 528 doubles at 20 row blocks / DK 6, the largest instantiation
    def lds(nblk, dk):
        w = nblk if nblk <= 7 else (nblk + 1) // 2
        jb, pd, mp = (4 * dk + 1 + 15) // 16, 17, 16 * nblk
        pw, ct = 16 * jb * pd + 16, 16 * 16 * pd
        return 4 * dk * pd + max(mp * pd, ct) + max(mp * pd, w * pw) + w * 16 + 4 * dk + ct + 2 * 16 * pd
    heights, dks = _compiled()
    sizes = {(nb, dk): lds(nb, dk) for nb in heights for dk in dks}
    assert max(sizes.values()) == sizes[(20, 6)] == 16528 and 8 * 16528 <= 163840
