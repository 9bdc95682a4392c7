"""The references of the GPModel.linearize tests against each other (no GPU): reverse-mode autodiff of the oracle's
GPModel.predict per output dimension (a) and the closed form through an explicit inverse (b), tests/gp_linearize_cases.py.

Bounds: 1e-12 of the largest entry on the well-conditioned cases (measured: 9e-15) and 1e-7 on the two ill-conditioned ones
(measured: 4.9e-10 and 6.3e-9), so the reference of the GPU tests is at least two orders inside their 1e-6 rule."""
import numpy as np
import pytest
import torch

import gp_autograd_cases as gc
import gp_linearize_cases as lc


@pytest.mark.parametrize('case', lc.WELL_CASES, ids=str)
def test_autodiff_and_closed_form_agree_well_conditioned(case):
    a, b = lc.reference_autodiff(*case), lc.reference_closed_form(*case)
    em, ev = lc.rel_err(b['dmean'], a['dmean']), lc.rel_err(b['dvar'], a['dvar'])
    print('%s cond %.1e  dmean %.1e  dvar %.1e' % (case, b['cond'], em, ev))
    assert b['cond'] < 1e3
    assert em < 1e-12 and ev < 1e-12


@pytest.mark.parametrize('case', lc.ILL_CASES, ids=str)
def test_autodiff_and_closed_form_agree_ill_conditioned(case):
    a, b = lc.reference_autodiff(*case), lc.reference_closed_form(*case)
    em, ev = lc.rel_err(b['dmean'], a['dmean']), lc.rel_err(b['dvar'], a['dvar'])
    print('%s cond %.1e  dmean %.1e  dvar %.1e' % (case, b['cond'], em, ev))
    assert b['cond'] > 1e7
    assert em < 1e-7 and ev < 1e-7


@pytest.mark.parametrize('case', lc.LONG_CASES, ids=str)
def test_autodiff_and_closed_form_agree_on_the_long_cases(case):
    """cond_2(K_mm + jitter I) <= 1e5, the bound of gp_tile_grid.ROWS (measured: at most 1.9e3), and the 1e-12 of the
    well-conditioned cases (measured: 2.9e-14); fmean and fvar agree entry by entry 100 times inside the rtol 1e-8 / atol
    1e-12 the GPU test holds them to (measured: 0.9 % of it)"""
    a, b = lc.reference_autodiff(*case), lc.reference_closed_form(*case)
    em, ev = lc.rel_err(b['dmean'], a['dmean']), lc.rel_err(b['dvar'], a['dvar'])
    print('%s cond %.1e  dmean %.1e  dvar %.1e' % (case, b['cond'], em, ev))
    assert b['cond'] <= 1e5
    assert em < 1e-12 and ev < 1e-12
    for k in ('fmean', 'fvar'):
        np.testing.assert_allclose(b[k], a[k], rtol=1e-10, atol=1e-14)


def test_long_cases_go_round_the_column_block_loop_twice_at_every_tile_height():
    import gp_tile_grid as grid
    import tile_grid as tg
    assert lc.LONG_CASES[0] == lc.LONG_CASE
    assert grid.long_heights(lc.LONG_CASES) == sorted(grid.dispatch_heights())
    host = tg._read('cbfssm_gp_lin.hip')
    assert 'const int64_t cap = gp_lin_maxwg(L->NBLK);' in host and 'case NB: return GpBwdCfg<NB>::MAXWG;' in host
    for M, D, Do, npts in lc.LONG_CASES:
        k, r = grid.long_k_r(npts, grid.max_workgroups(grid.leaf_key(M, D, Do)[0]))
        assert 1 <= k <= 4 and 1 <= r <= 15, (M, npts, k, r)
        assert M < 113 or D >= 6, (M, D)


def test_autodiff_against_central_differences():
    """(a) at (12, 4, 3, 5): h = 1e-5 on inputs of size 1 leaves a truncation error of h^2 |f'''| / 6 ~ 1e-10 and a rounding
    error of eps |f| / h ~ 1e-11; the bound is 1e-7 of the largest entry"""
    M, D, Do, npts = 12, 4, 3, 5
    ref = lc.reference_autodiff(M, D, Do, npts)
    p, X, _, _ = gc.make_inputs(M, D, Do, npts)
    _, gp = gc.oracle_model(p)
    h = 1e-5
    dmean, dvar = np.empty((npts, Do, D)), np.empty((npts, Do, D))
    with torch.no_grad():
        for i in range(D):
            Xp, Xm = X.copy(), X.copy()
            Xp[:, i] += h
            Xm[:, i] -= h
            mp, vp = gp.predict(torch.tensor(Xp))
            mm, vm = gp.predict(torch.tensor(Xm))
            dmean[:, :, i] = ((mp - mm) / (2 * h)).numpy()
            dvar[:, :, i] = ((vp - vm) / (2 * h)).numpy()
    assert lc.rel_err(dmean, ref['dmean']) < 1e-7
    assert lc.rel_err(dvar, ref['dvar']) < 1e-7


def test_transition_jacobians_restated():
    """A = I + d fmean / d h, B = d fmean / d a: the Jacobians of m = h + fmean(concat(h, a)) by autodiff of that expression"""
    M, D, Do, npts = lc.VOLIRO_CASE
    A, B = lc.transition_reference(M, D, Do, npts)
    assert A.shape == (npts, Do, Do) and B.shape == (npts, Do, D - Do)
    p, X, _, _ = gc.make_inputs(M, D, Do, npts)
    _, gp = gc.oracle_model(p)
    hh = torch.tensor(X[:, :Do], requires_grad=True)
    aa = torch.tensor(X[:, Do:], requires_grad=True)
    m = hh + gp.predict(torch.cat([hh, aa], dim=1))[0]
    for d in range(Do):
        gh, ga = torch.autograd.grad(m[:, d].sum(), (hh, aa), retain_graph=True)
        assert np.abs(gh.numpy() - A[:, d, :]).max() < 1e-13 * max(1.0, np.abs(A).max())
        assert np.abs(ga.numpy() - B[:, d, :]).max() < 1e-13 * max(1.0, np.abs(B).max())
    # the state alone (a = None): B is empty
    A0, B0 = lc.transition_reference(30, 5, 5, 7)
    assert A0.shape == (7, 5, 5) and B0.shape == (7, 5, 0)
