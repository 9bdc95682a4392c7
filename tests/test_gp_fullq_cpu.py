"""Host-side checks of the full-covariance q(z) reference (no GPU): the restatement of tests/gp_fullq_cases.py is fit to
measure the kernels by -- a second, independent coding agrees to 1e-10 of the largest entry on every case, the forward is
the numpy oracle's conditional(), nothing above the diagonal of q is read, and with L_d = diag(std_d) it is the diagonal
GPModel of oracle/cbfssm_torch_ref."""
import numpy as np
import pytest
import torch

import gp_autograd_cases as gc
import gp_fullq_cases as fq
from gp_fullq_cases import CASES, PARAMS

TOL = 1e-10


def _close(name, a, b, tol=TOL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = np.abs(b).max()
    err = np.abs(a - b).max() / scale
    print('%-28s max|ref| %.3e  err/max %.2e' % (name, scale, err))
    assert err < tol, (name, err)


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'M%d-D%d-Do%d-n%d' % c)
def test_two_codings_agree(case):
    r, s = fq.reference(*case), fq.reference2(*case)
    for k in ('fmean', 'fvar', 'g_X'):
        _close(k, s[k], r[k])
    assert abs(s['kl'] - r['kl']) <= TOL * abs(r['kl'])
    for k in PARAMS:
        _close('g_' + k, s['g_' + k], r['g_' + k])
        _close('k_' + k, s['k_' + k], r['k_' + k])


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'M%d-D%d-Do%d-n%d' % c)
def test_gradient_above_the_diagonal_is_exactly_zero(case):
    M = case[0]
    upper = np.triu(np.ones((M, M), dtype=bool), 1)
    for ref in (fq.reference(*case), fq.reference2(*case)):
        for k in ('g_zeta_sqrt', 'k_zeta_sqrt'):
            assert np.all(ref[k][:, upper] == 0.0), k
            assert np.abs(ref[k][:, ~upper]).max() > 0.0, k


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'M%d-D%d-Do%d-n%d' % c)
def test_forward_equals_the_oracle_conditional(case):
    from oracle import cbfssm_oracle as orc
    p, X, _, _ = fq.make_inputs(*case)
    kern = orc.RBF(p['variance_unc'], p['lengthscales_unc'])
    fmean, fvar = orc.conditional(X, p['zeta_pos'], kern, p['zeta_mean'], np.tril(p['zeta_sqrt']))
    r = fq.reference(*case)
    np.testing.assert_allclose(r['fmean'], fmean, rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(r['fvar'], fvar, rtol=1e-8, atol=1e-11)


@pytest.mark.parametrize('case', [(12, 4, 3, 41), (100, 21, 14, 41), (113, 9, 1, 17)], ids=lambda c: 'M%d-D%d-Do%d-n%d' % c)
def test_diagonal_factors_give_the_diagonal_model(case):
    M, D, Do, npts = case
    p, X, Wm, Wv = gc.make_inputs(*case)
    t, gp = gc.oracle_model(p)
    Xd = torch.tensor(X, requires_grad=True)
    fm, fv = gp.predict(Xd)
    kl = gp.prior_kl()
    ((torch.tensor(Wm) * fm).sum() + (torch.tensor(Wv) * fv).sum() + gc.KL_WEIGHT * kl).backward()

    std = torch.sqrt(torch.nn.functional.softplus(torch.tensor(p['zeta_var_unc'])) + 1e-10)      # (M, Do)
    pf = {k: p[k] for k in PARAMS if k != 'zeta_sqrt'}
    pf['zeta_sqrt'] = torch.diag_embed(std.T).numpy()
    tf = fq.tensors(pf)
    Xf = torch.tensor(X, requires_grad=True)
    fm2, fv2, kl2 = fq.restatement(tf, Xf)
    ((torch.tensor(Wm) * fm2).sum() + (torch.tensor(Wv) * fv2).sum() + gc.KL_WEIGHT * kl2).backward()

    np.testing.assert_allclose(fm2.detach().numpy(), fm.detach().numpy(), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(fv2.detach().numpy(), fv.detach().numpy(), rtol=1e-9, atol=1e-12)
    assert abs(float(kl2.detach()) - float(kl.detach())) <= 1e-10 * abs(float(kl.detach()))
    _close('g_X', Xf.grad.numpy(), Xd.grad.numpy())
    for k in ('zeta_pos', 'zeta_mean', 'variance_unc', 'lengthscales_unc'):
        _close('g_' + k, tf[k].grad.numpy(), t[k].grad.numpy())
    # d/d zeta_var_unc = d/d L_ii * d std / d zeta_var_unc = gL_ii * sigmoid(unc) / (2 std)
    gdiag = torch.diagonal(tf['zeta_sqrt'].grad, dim1=1, dim2=2).T
    chain = gdiag * torch.sigmoid(torch.tensor(p['zeta_var_unc'])) / (2.0 * std)
    _close('g_zeta_var_unc', chain.numpy(), t['zeta_var_unc'].grad.numpy())
