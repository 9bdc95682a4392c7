"""Shared by the GPModel.moment_match tests: the cases, their inputs (the GP of gp_autograd_cases.make_inputs, its X as the
means of the beliefs, covariances drawn here) and two CPU references of the moments of the GP output under x ~ N(m, S),

    fmean[n, d] = E[f_d],   fcov[n, d, e] = Cov(f_d, f_e),   xcov[n, d, i] = Cov(f_d, x_i)

  (a) reference_closed_form: the closed form for the RBF kernel in numpy through explicit inverses (of K = K_mm + jitter I, of
      I + S~ and of I / 2 + S~) and sums over all pairs of inducing points -- any positive semi-definite S;
  (b) reference_quadrature: Gauss-Hermite quadrature, 48 nodes per axis, through oracle/cbfssm_torch_ref.GPModel.predict for
      S = V V^T with V (D, r), r <= 2 -- a quadrature over r dimensions whatever D is:
      E[f], E[f f^T] - E[f] E[f]^T + diag E[fvar], E[(f - E f)(x - m)^T].

The covariance of point n is one of three kinds, in turn (KINDS[n % 3]):

    rank2   S = V V^T,  V = 0.5 l[:, None] N(0, 1) / sqrt(D)  of shape (D, min(2, D))      -- what (b) can pin
    full    S = A A^T,  A the same draw of shape (D, D)
    block   S = blockdiag(P, 0), P = A A^T of shape (Do, Do) on the same scale, where D > Do (else: full)
                                                                     -- the belief of transition_moments: a known input

Measured here over every rank2 belief of the GPU tests (tests/test_gp_moment_match_cpu.py, per case tensor): (a) and (b) agree
to 7.2e-13 (fmean), 5.6e-11 (fcov) and 3.5e-13 (xcov) of the largest entry, and to 1.5e-10 on the strictly lower triangle of fcov
relative to its own largest entry, which is never below 7.6e-3 on the rows of gp_tile_grid.ROWS; cond_2(K) is at most 9.8e4.
LONG_CASES (the shapes of gp_linearize_cases.LONG_CASES) stay inside these figures: cond_2 at most 1.9e3, and at worst
2.2e-14 / 9.5e-13 / 1.7e-14 / 5.8e-12, all at (320, 12, 4).
Results are cached per case: treat them as read-only."""
import functools

import numpy as np
import torch

import gp_autograd_cases as gc

JITTER = 1e-8
KINDS = ('rank2', 'full', 'block')
N_POINTS = 37
QUAD_NODES = 48

# (M, D, Do, npts).  The edges tests/gp_tile_grid.ROWS does not force: the smallest problem; D = 15 / 16 at one tile height (the
# ones row of the ZT image moves from the first to the second input row block); Do = 16 with D = 24; one point, one full
# point group, one more
EDGE_CASES = [(1, 1, 1, 1), (40, 15, 3, 17), (40, 16, 3, 17), (112, 24, 16, 17), (30, 7, 5, 1), (30, 7, 5, 16), (30, 7, 5, 17)]
# more point groups than the launch has workgroups at the cheapest tile (GpBwdCfg<1>::MAXWG = 1024).  Its beliefs are those of
# npts = 37 repeated with period 37 (coprime to the 16 points of a group): a wrong point index still shows, and (b) has 13
# quadratures to do instead of 5474
LONG_CASE = (12, 4, 3, 16 * 1026 + 5)
# and at every tile height (the slot and region aliasing of cbfssm_gp_mm.hpp differs per height): npts = 16 (cap + k) + r,
# cap = GpBwdCfg<NBLK>::MAXWG, 1 <= k <= 4, 1 <= r <= 15; the same period-37 beliefs (distinct_points)
LONG_CASES = [LONG_CASE, (24, 8, 8, 16 * (1024 + 2) + 11), (50, 9, 2, 16 * (512 + 1) + 13), (99, 7, 5, 16 * (512 + 4) + 3),
              (160, 9, 3, 16 * (256 + 3) + 7), (180, 12, 3, 16 * (256 + 1) + 15), (250, 12, 6, 16 * (256 + 2) + 1),
              (320, 12, 4, 16 * (256 + 4) + 9)]
# Voliro's recognition shape: state 6, inputs (u, y) 13
VOLIRO_CASE = (20, 19, 6, 37)
# transition_moments: a stash height, Voliro, and a GP that takes the state alone (D = Do, a = None)
TRANSITION_CASES = [(130, 21, 14, 19), VOLIRO_CASE, (30, 5, 5, 7)]
WIDE_CASE = (30, 7, 5, 19)
RANK1_CASE = (100, 21, 14, 19)


def softplus(x):
    return np.logaddexp(0.0, x) + 1e-10


def distinct_points(npts):
    return min(npts, N_POINTS) if npts > 1000 else npts


def make_beliefs(M, D, Do, npts, kind='mixed'):
    """(p, mean (npts, D), cov (npts, D, D), kinds): kind 'mixed' takes KINDS in turn; 'rank2', 'full', 'block', 'rank1', 'zero'
    and 'wide' (full rank, eigenvalues of S~ around 1e4) give every point that kind; 'transition' is 'block' everywhere (D > Do)
    or 'full' (D = Do)."""
    nd = distinct_points(npts)
    p, X, _, _ = gc.make_inputs(M, D, Do, nd)
    ls = softplus(p['lengthscales_unc'])
    rng = np.random.default_rng(7000 * M + 70 * D + Do)
    cov, kinds = np.zeros((nd, D, D)), []
    for n in range(nd):
        A = 0.5 * ls[:, None] * rng.standard_normal((D, D)) / np.sqrt(D)          # (drawn for every point: one stream per case)
        k = KINDS[n % 3] if kind == 'mixed' else kind
        if k == 'transition':
            k = 'block'
        if k == 'block' and D == Do:
            k = 'full'
        if k == 'rank2':
            V = A[:, :min(2, D)]
            cov[n] = V @ V.T
        elif k == 'rank1':
            cov[n] = np.outer(A[:, 0], A[:, 0])
        elif k == 'full':
            cov[n] = A @ A.T
        elif k == 'block':
            cov[n, :Do, :Do] = A[:Do, :Do] @ A[:Do, :Do].T
        elif k == 'wide':
            cov[n] = 1e4 * ls[:, None] * ls[None, :] * (np.eye(D) + 0.3 * (A / ls[:, None]) @ (A / ls[:, None]).T)
        else:
            assert k == 'zero', k
        kinds.append(k)
    if nd < npts:
        idx = np.arange(npts) % nd
        X, cov, kinds = X[idx], cov[idx], [kinds[i] for i in idx]
    return p, X, cov, kinds


def rank2_factor(M, D, Do, n):
    """V (D, min(2, D)) of point n of the 'mixed' beliefs when it is of kind rank2 (the same stream as make_beliefs)"""
    p, _, _, _ = gc.make_inputs(M, D, Do, 1)
    ls = softplus(p['lengthscales_unc'])
    rng = np.random.default_rng(7000 * M + 70 * D + Do)
    for _ in range(n + 1):
        A = 0.5 * ls[:, None] * rng.standard_normal((D, D)) / np.sqrt(D)
    return A[:, :min(2, D)]


def closed_form(p, mean, cov):
    """(a) for the beliefs (mean (n, D), cov (n, D, D)): dict fmean (n, Do), fcov (n, Do, Do), xcov (n, Do, D), cond"""
    ls, var = softplus(p['lengthscales_unc']), float(softplus(p['variance_unc'])[0])
    s2, mu = softplus(p['zeta_var_unc']), p['zeta_mean']
    M, D = p['zeta_pos'].shape
    Do = mu.shape[1]
    Zs = p['zeta_pos'] / ls
    d2 = ((Zs[:, None, :] - Zs[None, :, :]) ** 2).sum(-1)
    K = var * np.exp(-0.5 * d2) + JITTER * np.eye(M)
    Kinv = np.linalg.inv(K)
    alpha = Kinv @ mu
    W = np.stack([Kinv - (Kinv * s2[:, d][None, :]) @ Kinv for d in range(Do)])            # (Do, M, M)
    n = mean.shape[0]
    fmean, fcov, xcov = np.empty((n, Do)), np.empty((n, Do, Do)), np.empty((n, Do, D))
    eye = np.eye(D)
    for i in range(n):
        St = cov[i] / ls[:, None] / ls[None, :]
        r = Zs - mean[i] / ls                                                       # (M, D)
        B1, B2 = np.linalg.inv(eye + St), np.linalg.inv(0.5 * eye + St)
        q = var / np.sqrt(np.linalg.det(eye + St)) * np.exp(-0.5 * np.einsum('id,de,ie->i', r, B1, r))
        fm = alpha.T @ q
        rr = r[:, None, :] + r[None, :, :]                                          # (M, M, D): every pair
        quad = np.einsum('ijd,ijd->ij', rr @ B2, rr)
        Q = var * var / np.sqrt(np.linalg.det(eye + 2.0 * St)) * np.exp(-0.25 * d2 - 0.125 * quad)
        fmean[i] = fm
        fcov[i] = alpha.T @ Q @ alpha - np.outer(fm, fm) + np.diag(var - (W * Q[None]).sum((1, 2)))
        xcov[i] = ((St @ B1 @ (r.T @ (alpha * q[:, None]))) * ls[:, None]).T
    return {'fmean': fmean, 'fcov': fcov, 'xcov': xcov, 'cond': float(np.linalg.cond(K))}


@functools.lru_cache(maxsize=None)
def reference_closed_form(M, D, Do, npts, kind='mixed'):
    """(a) of a case, computed once per distinct belief and shared (treat as read-only)"""
    nd = distinct_points(npts)
    p, mean, cov, _ = make_beliefs(M, D, Do, nd, kind)
    out = closed_form(p, mean, cov)
    if nd < npts:
        idx = np.arange(npts) % nd
        out = {k: (v[idx] if k != 'cond' else v) for k, v in out.items()}
    return out


def quadrature(gp, m, V, nodes=QUAD_NODES):
    """(b) at one belief N(m, V V^T), V (D, r) with r <= 2, through the oracle model `gp`: (fmean, fcov, xcov (Do, D))"""
    x, w = np.polynomial.hermite_e.hermegauss(nodes)
    w = w / np.sqrt(2.0 * np.pi)
    r = V.shape[1]
    G = np.stack(np.meshgrid(*([x] * r), indexing='ij'), -1).reshape(-1, r)
    ww = np.prod(np.stack(np.meshgrid(*([w] * r), indexing='ij'), -1).reshape(-1, r), 1)
    X = m + G @ V.T
    with torch.no_grad():
        f, fv = gp.predict(torch.tensor(X))
    f, fv = f.numpy(), fv.numpy()
    fm = ww @ f
    fc = (f * ww[:, None]).T @ f - np.outer(fm, fm) + np.diag(ww @ fv)
    xc = (f - fm).T @ ((X - m) * ww[:, None])
    return fm, fc, xc


@functools.lru_cache(maxsize=None)
def reference_quadrature(M, D, Do, npts):
    """(b) at every rank2 point of the 'mixed' beliefs of a case: {n: (fmean, fcov, xcov)} over the distinct beliefs"""
    nd = distinct_points(npts)
    p, mean, cov, kinds = make_beliefs(M, D, Do, nd)
    _, gp = gc.oracle_model(p)
    out = {}
    for n in range(nd):
        if kinds[n] == 'rank2':
            V = rank2_factor(M, D, Do, n)
            assert np.array_equal(V @ V.T, cov[n])
            out[n] = quadrature(gp, mean[n], V)
    return out


def transition_reference(M, D, Do, npts):
    """(m+, P+, cross) of GPModel.transition_moments restated from (a) on the 'transition' beliefs: h+ = h + f(concat(h, a)),
    h ~ N(h, P), a known"""
    p, mean, cov, _ = make_beliefs(M, D, Do, npts, 'transition')
    ref = reference_closed_form(M, D, Do, npts, 'transition')
    P = cov[:, :Do, :Do]
    Cm = np.transpose(ref['xcov'][:, :, :Do], (0, 2, 1))                             # Cov(h, f)
    return mean[:, :Do] + ref['fmean'], P + Cm + np.transpose(Cm, (0, 2, 1)) + ref['fcov'], P + Cm


def rel_err(g, r):
    """largest deviation over the largest entry of the reference (the measure of gp_autograd_cases.within_rule)"""
    return float(np.abs(np.asarray(g) - np.asarray(r)).max() / np.abs(np.asarray(r)).max())


def lower(fcov):
    """the strictly lower triangles of (n, Do, Do) as (n, Do (Do - 1) / 2)"""
    i, j = np.tril_indices(fcov.shape[-1], -1)
    return fcov[..., i, j]


def diagonal(fcov):
    return np.diagonal(fcov, axis1=-2, axis2=-1)
