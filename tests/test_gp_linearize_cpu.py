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
