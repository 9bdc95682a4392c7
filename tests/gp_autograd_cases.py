"""Shared by the differentiable-GPModel tests: the cases, their inputs, and the reference -- reverse-mode autodiff of
oracle/cbfssm_torch_ref.GPModel on the CPU with the five parameter tensors and X requiring grad.

The loss of every case is  sum(Wm o fmean) + sum(Wv o fvar) + 0.3 prior_kl  with fixed standard-normal Wm, Wv.
On this input family cond_2(K_mm + 1e-8 I) is between 9 and 5e2 and two independent CPU codings of the function agree on
every gradient tensor to 4e-14 of its largest entry, so the reference sits eight orders inside the 1e-6 rule and no entry
is masked."""
import functools

import numpy as np
import torch

PARAMS = ('zeta_pos', 'zeta_mean', 'zeta_var_unc', 'variance_unc', 'lengthscales_unc')
KL_WEIGHT = 0.3

# (M, D, Do, npts): the shapes of the feature's own tests; tests/gp_tile_grid.py holds the table that reaches every compiled
# (tile height, input width) leaf of the adjoint kernels
CASES = [
    (12, 4, 3, 41),             # one row block, ragged columns
    (30, 7, 5, 16),
    (64, 16, 8, 1),
    (100, 21, 14, 41),          # the Sarcos tile
    (112, 24, 16, 50),          # every limit at once, full tile
    (113, 9, 1, 17),            # first stash height, Do = 1
    (130, 6, 4, 41),
    (200, 13, 7, 41),
    (250, 6, 2, 33),
    (300, 6, 4, 41),
    (100, 21, 14, 16 * 600 + 5),   # many column blocks per persistent workgroup
]


def softplus_inverse(y):
    y = np.asarray(y, dtype=np.float64) - 1e-10
    return y + np.log(-np.expm1(-y))


def make_inputs(M, D, Do, npts, seed=None):
    """numpy inputs of one case, drawn in the documented order"""
    rng = np.random.default_rng(1000 * M + 10 * D + Do if seed is None else seed)
    zeta_pos = rng.uniform(-2, 2, (M, D))
    zeta_mean = 0.5 * rng.standard_normal((M, Do))
    zeta_var = 0.05 * np.exp(rng.uniform(-1, 1, (M, Do)))
    gl = max(1.0, 0.75 * np.sqrt(D))
    ls = rng.uniform(0.8, 1.25, D) * gl
    X = 1.4 * rng.standard_normal((npts, D))
    Wm = rng.standard_normal((npts, Do))
    Wv = rng.standard_normal((npts, Do))
    p = {'zeta_pos': zeta_pos, 'zeta_mean': zeta_mean, 'zeta_var_unc': softplus_inverse(zeta_var),
         'variance_unc': softplus_inverse(np.array([0.4])), 'lengthscales_unc': softplus_inverse(ls)}
    return p, X, Wm, Wv


def oracle_model(p):
    from oracle import cbfssm_torch_ref as tref
    t = {k: torch.tensor(p[k], dtype=torch.float64, requires_grad=True) for k in PARAMS}
    return t, tref.GPModel(*[t[k] for k in PARAMS])


@functools.lru_cache(maxsize=None)
def reference(M, D, Do, npts):
    """dict: fmean, fvar, kl, the gradients of the case's loss ('g_' + name, 'g_X') and of prior_kl alone ('k_' + name);
    computed once per case and shared (treat as read-only)"""
    p, X, Wm, Wv = make_inputs(M, D, Do, npts)
    t, gp = oracle_model(p)
    Xt = torch.tensor(X, requires_grad=True)
    fmean, fvar = gp.predict(Xt)
    kl = gp.prior_kl()
    loss = (torch.tensor(Wm) * fmean).sum() + (torch.tensor(Wv) * fvar).sum() + KL_WEIGHT * kl
    loss.backward()
    out = {'fmean': fmean.detach().numpy(), 'fvar': fvar.detach().numpy(), 'kl': float(kl.detach()), 'g_X': Xt.grad.numpy().copy()}
    for k in PARAMS:
        out['g_' + k] = t[k].grad.numpy().copy()
    t2, gp2 = oracle_model(p)
    gp2.prior_kl().backward()
    for k in PARAMS:
        out['k_' + k] = t2[k].grad.numpy().copy()
    return out


def within_rule(name, g, r, rtol=1e-6):
    """the rule of tests/test_hip_grad.py: every entry within rtol of the largest entry of its tensor; prints the ratio"""
    g, r = np.asarray(g, dtype=np.float64), np.asarray(r, dtype=np.float64)
    assert g.shape == r.shape, (name, g.shape, r.shape)
    scale = np.abs(r).max()
    assert scale > 0.0, (name, 'the reference is all zero')
    err = np.abs(g - r).max() / scale
    print('%-34s max|ref| %.3e  err/max %.2e' % (name, scale, err))
    assert np.all(np.isfinite(g)) and err < rtol, (name, err)
    return err
