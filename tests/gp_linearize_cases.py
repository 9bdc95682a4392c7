"""Shared by the GPModel.linearize tests: the cases, their inputs (gp_autograd_cases.make_inputs) and two CPU references of

    dmean[n, d, i] = d fmean[n, d] / d X[n, i],   dvar[n, d, i] = d fvar[n, d] / d X[n, i]

  (a) reference_autodiff: reverse-mode autodiff of oracle/cbfssm_torch_ref.GPModel.predict (triangular solves), one output
      dimension at a time -- the points do not interact, so the gradient of sum_n fmean[n, d] with respect to X is row by row
      the Jacobian of dimension d;
  (b) reference_closed_form: the closed form in numpy through an explicit inverse of K = K_mm + jitter I,

          k = K(Z, x_n), A2 = K^-1 k, alpha = K^-1 mu, z~ = Z / l, x~ = x / l
          dmean[n, d, :] = ( z~^T Em_d - x~_n sum_m Em_d ) / l,   Em_d = alpha[:, d] o k
          dvar[n, d, :]  = ( z~^T Ev_d - x~_n sum_m Ev_d ) / l,   Ev_d = 2 (K^-1 (A2 o s2_d) - A2) o k

Measured here: (a) and (b) agree to 8e-15 (dmean) and 9e-15 (dvar) of the largest entry on the well-conditioned cases
(cond_2(K) between 1 and 5e2), to 2.3e-10 / 4.9e-10 at (130, 3, 2, 33) (cond_2 7.9e7) and 3.9e-9 / 6.3e-9 at (64, 2, 3, 33)
(cond_2 7.5e8); on LONG_CASES cond_2 is at most 1.9e3 (at (320, 12, 4)) and they agree to 2.3e-14 / 2.9e-14 at worst, and on
every entry of fmean and fvar to 0.9 % of the elementwise rtol 1e-8 / atol 1e-12 the GPU test holds them to.  ((257, 6, 3),
cond_2 9.8e4, was not taken for the tallest tile: there the two codings differ on an entry of fmean by 0.99 of that
elementwise tolerance, so the test would measure the reference.)  Results are cached per case: treat them as read-only."""
import functools

import numpy as np
import torch

import gp_autograd_cases as gc

JITTER = 1e-8

# (M, D, Do, npts)
WELL_CASES = [(12, 4, 3, 41), (1, 1, 1, 1), (16, 4, 16, 17), (17, 5, 2, 16), (100, 21, 14, 41), (112, 24, 16, 50),
              (113, 9, 1, 17), (200, 13, 7, 33), (320, 24, 16, 18)]
ILL_CASES = [(130, 3, 2, 33), (64, 2, 3, 33)]
# the edges tests/gp_tile_grid.ROWS does not force: the smallest problem; D = 15 / 16 at one tile height (the ones row of
# the ZT image moves from the first to the second input row block); every limit of the input side with Do = 16; Do = 1;
# one point, one full column block, one more, three ragged
EDGE_CASES = [(1, 1, 1, 1), (40, 15, 3, 17), (40, 16, 3, 17), (112, 24, 16, 17), (113, 9, 1, 17),
              (30, 7, 5, 1), (30, 7, 5, 16), (30, 7, 5, 17), (30, 7, 5, 41)]
# more column blocks than the launch has workgroups at the cheapest tile (GpBwdCfg<1>::MAXWG = 1024)
LONG_CASE = (12, 4, 3, 16 * 1026 + 5)
# and at every tile height, because W = ceil(NBLK / RB) waves and what a second trip finds in LDS differ per height:
# npts = 16 (cap + k) + r, cap = GpBwdCfg<NBLK>::MAXWG (gp_tile_grid.max_workgroups), 1 <= k <= 4, 1 <= r <= 15, so that a few
# workgroups take a second column block and the last block is ragged.  Small Do; D >= 9 at M >= 113 (conditioning: see the
# module docstring).  The references are per batch and cheap: every point is distinct.
LONG_CASES = [LONG_CASE, (24, 8, 8, 16 * (1024 + 2) + 11), (50, 9, 2, 16 * (512 + 1) + 13), (99, 7, 5, 16 * (512 + 4) + 3),
              (160, 9, 3, 16 * (256 + 3) + 7), (180, 12, 3, 16 * (256 + 1) + 15), (250, 12, 6, 16 * (256 + 2) + 1),
              (320, 12, 4, 16 * (256 + 4) + 9)]
# Voliro's recognition shape: state 6, inputs (u, y) 13
VOLIRO_CASE = (20, 19, 6, 37)


def softplus(x):
    return np.logaddexp(0.0, x) + 1e-10


@functools.lru_cache(maxsize=None)
def reference_autodiff(M, D, Do, npts):
    """(a): dict fmean, fvar (npts, Do), dmean, dvar (npts, Do, D)"""
    p, X, _, _ = gc.make_inputs(M, D, Do, npts)
    _, gp = gc.oracle_model(p)
    Xt = torch.tensor(X, requires_grad=True)
    fmean, fvar = gp.predict(Xt)
    dmean, dvar = np.empty((npts, Do, D)), np.empty((npts, Do, D))
    for d in range(Do):
        dmean[:, d, :] = torch.autograd.grad(fmean[:, d].sum(), Xt, retain_graph=True)[0].numpy()
        dvar[:, d, :] = torch.autograd.grad(fvar[:, d].sum(), Xt, retain_graph=True)[0].numpy()
    return {'fmean': fmean.detach().numpy(), 'fvar': fvar.detach().numpy(), 'dmean': dmean, 'dvar': dvar}


@functools.lru_cache(maxsize=None)
def reference_closed_form(M, D, Do, npts):
    """(b): dict fmean, fvar (npts, Do), dmean, dvar (npts, Do, D), cond (cond_2 of K_mm + jitter I)"""
    p, X, _, _ = gc.make_inputs(M, D, Do, npts)
    ls, var = softplus(p['lengthscales_unc']), float(softplus(p['variance_unc'])[0])
    s2, mu = softplus(p['zeta_var_unc']), p['zeta_mean']
    Zs, Xs = p['zeta_pos'] / ls, X / ls

    def rbf(A, B):
        d2 = (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * A @ B.T
        return var * np.exp(-0.5 * np.maximum(d2, 0.0))

    K = rbf(Zs, Zs) + JITTER * np.eye(M)
    Kinv = np.linalg.inv(K)
    k = rbf(Zs, Xs)                                         # (M, npts)
    A2 = Kinv @ k
    alpha = Kinv @ mu                                       # (M, Do)
    dmean, dvar = np.empty((npts, Do, D)), np.empty((npts, Do, D))
    for d in range(Do):
        Em = alpha[:, d:d + 1] * k
        Ev = 2.0 * (Kinv @ (A2 * s2[:, d:d + 1]) - A2) * k
        for E, out in ((Em, dmean), (Ev, dvar)):
            out[:, d, :] = (E.T @ Zs - Xs * E.sum(0)[:, None]) / ls
    fvar = (var - (k * A2).sum(0))[:, None] + (A2 * A2).T @ s2
    return {'fmean': k.T @ alpha, 'fvar': fvar, 'dmean': dmean, 'dvar': dvar, 'cond': float(np.linalg.cond(K))}


def transition_reference(M, D, Do, npts):
    """(A, B) of GPModel.transition_jacobians restated from (a): the recurrence m = h + fmean(concat(h, a))"""
    dmean = reference_autodiff(M, D, Do, npts)['dmean']
    return dmean[:, :, :Do] + np.eye(Do)[None], dmean[:, :, Do:]


def rel_err(g, r):
    """largest deviation over the largest entry of the reference (the measure of gp_autograd_cases.within_rule)"""
    return float(np.abs(np.asarray(g) - np.asarray(r)).max() / np.abs(np.asarray(r)).max())
