"""Shared by the tests of the leaf gradients of GPModel.moment_match (`differentiable=True`): the loss of
tests/gp_mm_grad_cases.py (non-symmetric Wc, the variants all / fmean / fcov / xcov / nocross) with its gradients for the FIVE
UNCONSTRAINED LEAVES of the model as well as for `mean` and `cov`, three times over:

  (a) gram: gp_mm_grad_cases.gram_moments over model constants rebuilt differentiably from the leaves -- softplus + 1e-10,
      K = K_mm + jitter I, its Cholesky factor, alpha and K^-1 by Cholesky solves, W_d = K^-1 - K^-1 diag(s2_d) K^-1 --
      torch float64 autograd; what the GPU tests compare the kernels with;
  (b) inverse: gp_mm_grad_cases.inverse_moments over the same constants through torch.linalg.inv(K), point by point;
  (c) numpy_adjoint: the adjoint coded by hand in numpy, in the steps of the kernels: per point the terms of
      alpha-bar, W-bar_d, E-hat, r-bar and the scalars, once per call the products with K^-1, then the chain of the tail
      (K^-1 -> K_mm -> Z~, lengthscales, variance, softplus) restated.

Cases: the parameters are those of gp_autograd_cases.make_inputs and the beliefs those of gp_moment_match_cases.make_beliefs,
unchanged at every shape: measured on the CPU (tests/test_gp_mm_param_grad_cpu.py) the two references agree inside the
1e-7 rule on every row of gp_tile_grid.ROWS and every edge, (257, 6, 3) with cond_2(K) = 9.8e4 included, so no case needed a
better-conditioned draw.

Beliefs beyond 1000 points repeat with period 37 (gp_moment_match_cases.distinct_points).  The leaf gradients sum over ALL
points, so the reference of such a case is computed on the 37 distinct beliefs with every weight multiplied by the number of
times its belief occurs; the per-point gradients are divided by that count again.  Results are cached: read-only."""
import functools

import numpy as np
import torch

import gp_autograd_cases as gc
import gp_mm_grad_cases as gg
import gp_moment_match_cases as mc

PARAMS = gc.PARAMS
VARIANTS = gg.VARIANTS
CPU_RULE = gg.CPU_RULE
GPU_RULE = gg.GPU_RULE
# the M edges: one row, around one row block, the slab / stash switch of the tail (112 / 113), the largest first-of-height
M_EDGES = [(1, 3, 2), (15, 5, 3), (16, 5, 3), (17, 5, 3), (112, 7, 3), (113, 7, 3), (257, 6, 3)]
# ragged D, Do = 1
SHAPE_EDGES = [(30, 7, 5), (40, 15, 1), (40, 17, 3), (20, 19, 6)]


def softplus_t(x):
    return torch.nn.functional.softplus(x) + 1e-10


def leaf_tensors(p):
    return [torch.tensor(np.asarray(p[k], dtype=np.float64), requires_grad=True) for k in PARAMS]


def model_constants_t(leaves, coding='gram'):
    """the dict gp_mm_grad_cases.gram_moments / inverse_moments read, as differentiable functions of the five leaves"""
    zp, zm, zv, var_u, ls_u = leaves
    ls, var, s2 = softplus_t(ls_u.reshape(-1)), softplus_t(var_u.reshape(-1))[0], softplus_t(zv)
    Zs = zp / ls
    M = Zs.shape[0]
    d2 = ((Zs[:, None, :] - Zs[None, :, :]) ** 2).sum(-1)
    K = var * torch.exp(-0.5 * d2) + mc.JITTER * torch.eye(M, dtype=torch.float64)
    if coding == 'gram':
        L = torch.linalg.cholesky(K)
        alpha = torch.cholesky_solve(zm, L)
        Kinv = torch.cholesky_solve(torch.eye(M, dtype=torch.float64), L)
    else:
        Kinv = torch.linalg.inv(K)
        alpha = Kinv @ zm
    W = torch.stack([Kinv - (Kinv * s2[:, d][None, :]) @ Kinv for d in range(zm.shape[1])])
    return {'ls': ls, 'var': var, 'Zs': Zs, 'd2': d2, 'alpha': alpha, 'W': W}


def moments_t(leaves, mean, cov, coding='gram'):
    c = model_constants_t(leaves, coding)
    return (gg.gram_moments if coding == 'gram' else gg.inverse_moments)(c, mean, cov)


def evaluate(p, mean, cov, weights, variant='all', coding='gram'):
    """dict fmean, fcov, xcov, g_mean, g_cov (None without cov), g_<leaf> as numpy, of coding 'gram' or 'inverse'"""
    leaves = leaf_tensors(p)
    mt = torch.tensor(np.asarray(mean), requires_grad=True)
    ct = torch.tensor(np.asarray(cov), requires_grad=True) if cov is not None else None
    out = moments_t(leaves, mt, ct, coding)
    gg.loss_of(out, weights, variant).backward()
    res = {k: v.detach().numpy() for k, v in zip(('fmean', 'fcov', 'xcov'), out)}
    res['g_mean'] = mt.grad.numpy().copy()
    res['g_cov'] = ct.grad.numpy().copy() if ct is not None and ct.grad is not None else None
    for k, t in zip(PARAMS, leaves):
        res['g_' + k] = t.grad.numpy().copy() if t.grad is not None else np.zeros(tuple(t.shape))   # (unconnected: zero)
    return res


def counts(npts):
    """how often each distinct belief occurs among npts points"""
    nd = mc.distinct_points(npts)
    return np.bincount(np.arange(npts) % nd, minlength=nd).astype(np.float64)


def case_inputs(M, D, Do, npts, kind='mixed'):
    """(p, mean, cov, weights) of all npts points"""
    p, mean, cov, _ = mc.make_beliefs(M, D, Do, npts, kind)
    return p, mean, cov, gg.make_weights(M, D, Do, npts)


@functools.lru_cache(maxsize=None)
def reference(M, D, Do, npts, kind='mixed', variant='all', coding='gram'):
    """the reference of a case, computed once on the distinct beliefs and shared (treat as read-only)"""
    nd = mc.distinct_points(npts)
    p, mean, cov, _ = mc.make_beliefs(M, D, Do, nd, kind)
    cnt = counts(npts)
    Wf, Wc, Wx = gg.make_weights(M, D, Do, nd)
    weights = (Wf * cnt[:, None], Wc * cnt[:, None, None], Wx * cnt[:, None, None])
    if coding == 'numpy':
        res = numpy_adjoint(p, mean, cov, *cotangents(weights, variant))
    else:
        res = evaluate(p, mean, cov, weights, variant, coding)
    if nd < npts:
        idx = np.arange(npts) % nd
        for k in ('fmean', 'fcov', 'xcov'):
            if k in res:
                res[k] = res[k][idx]
        res['g_mean'] = (res['g_mean'] / cnt[:, None])[idx]
        res['g_cov'] = (res['g_cov'] / cnt[:, None, None])[idx]
    return res


def cotangents(weights, variant='all'):
    """(gf, gC, gX) of the loss: a result the variant leaves out has a zero cotangent"""
    Wf, Wc, Wx = weights
    use = {'all': (1, 1, 1), 'nocross': (1, 1, 0), 'fmean': (1, 0, 0), 'fcov': (0, 1, 0), 'xcov': (0, 0, 1)}[variant]
    return tuple(np.asarray(w) * u for w, u in zip((Wf, Wc, Wx), use))


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def numpy_adjoint(p, mean, cov, gf, gC, gX):
    """(c): dict g_mean, g_cov, g_<leaf> by hand.  Notation of DESIGN 3.2k / 3.2m / 3.2o."""
    ls, var = mc.softplus(p['lengthscales_unc']), float(mc.softplus(p['variance_unc'])[0])
    s2, mu, Z = mc.softplus(p['zeta_var_unc']), p['zeta_mean'], p['zeta_pos']
    M, D = Z.shape
    Do = mu.shape[1]
    Zs = Z / ls
    d2 = ((Zs[:, None, :] - Zs[None, :, :]) ** 2).sum(-1)
    Kmm = var * np.exp(-0.5 * d2)
    Kinv = np.linalg.inv(Kmm + mc.JITTER * np.eye(M))
    alpha = Kinv @ mu
    W = np.stack([Kinv - (Kinv * s2[:, d][None, :]) @ Kinv for d in range(Do)])
    n = mean.shape[0]
    eye = np.eye(D)
    abar, Wbar, Ehat, Rbar = np.zeros((M, Do)), np.zeros((Do, M, M)), np.zeros((M, M)), np.zeros((M, D))
    gsig = glogsig = 0.0
    glx = np.zeros(D)
    g_mean, g_cov = np.zeros((n, D)), np.zeros((n, D, D))
    for i in range(n):
        S = np.tril(cov[i]) + np.tril(cov[i], -1).T if cov is not None else np.zeros((D, D))
        St, mt = S / ls[:, None] / ls[None, :], mean[i] / ls
        r = Zs - mt
        A, B = eye + St, 0.5 * eye + St
        L1, L2 = np.linalg.cholesky(A), np.linalg.cholesky(B)
        L1i, L2i = np.linalg.inv(L1), np.linalg.inv(L2)
        w, u = r @ L1i.T, r @ L2i.T                                                  # rows w_i = L1^-1 r_i, u_i = L2^-1 r_i
        q = var / np.prod(np.diag(L1)) * np.exp(-0.5 * (w * w).sum(1))
        g = (u * u).sum(1)
        Q = var * var / (2.0 ** (0.5 * D) * np.prod(np.diag(L2))) * np.exp(-0.25 * d2 - 0.125 * (g[:, None] + g[None, :] + 2.0 * u @ u.T))
        fmean = alpha.T @ q
        Gs = 0.5 * (gC[i] + gC[i].T)
        fbar = gf[i] - 2.0 * Gs @ fmean
        Qbar = alpha @ Gs @ alpha.T - np.einsum('d,dij->ij', np.diag(gC[i]), W)
        E = Qbar * Q
        e = E.sum(1)
        Yh = ls[:, None] * gX[i].T                                                   # (D, Do)
        H = r.T @ (q[:, None] * alpha)
        Ainv = L1i.T @ L1i
        AH, Hbar = Ainv @ H, Ainv @ St @ Yh
        qbar = alpha @ fbar + np.einsum('ik,kd,id->i', r, Hbar, alpha)
        ebar = qbar * q
        # the model's side
        abar += q[:, None] * (fbar[None, :] + r @ Hbar) + 2.0 * Q @ alpha @ Gs
        Wbar -= np.diag(gC[i])[:, None, None] * Q[None]
        Ehat += E
        t, a1 = u @ L2i, w @ L1i                                                     # rows B^-1 r_i, A^-1 r_i
        rbar = q[:, None] * (alpha @ Hbar.T) - ebar[:, None] * a1 - 0.5 * (e[:, None] * t + E @ t)
        Rbar += rbar
        glogsig += ebar.sum() + 2.0 * E.sum()
        gsig += np.trace(gC[i])
        # the belief's side (3.2m), which also carries the lengthscales' part through m~, S~ and the scaling of xcov
        Stbar = (Yh - Hbar) @ AH.T + 0.5 * L1i.T @ (w.T @ (ebar[:, None] * w) - ebar.sum() * eye) @ L1i \
            + L2i.T @ (0.25 * (u.T @ (e[:, None] * u) + u.T @ E @ u) - 0.5 * e.sum() * eye) @ L2i
        mtbar = -rbar.sum(0)
        xcov = (ls[:, None] * (St @ AH)).T                                           # (Do, D)
        glx += mtbar * mt + ((Stbar + Stbar.T) * St).sum(1) - (gX[i] * xcov).sum(0)
        g_mean[i] = mtbar / ls
        Sbar = Stbar / ls[:, None] / ls[None, :]
        g_cov[i] = np.tril(Sbar + Sbar.T) - np.diag(np.diag(Sbar))
    # once per call: through alpha = K^-1 mu and W_d
    mubar = Kinv @ abar
    X = np.stack([Kinv @ Wbar[d] for d in range(Do)])
    s2bar = np.stack([-np.einsum('ik,ki->i', X[d], Kinv) for d in range(Do)], 1)
    Kib = 0.5 * (abar @ mu.T + mu @ abar.T)
    for d in range(Do):
        Kib += Wbar[d] - X[d].T * s2[:, d][None, :] - X[d] * s2[:, d][:, None]
    Ztbar = Rbar - Ehat.sum(1)[:, None] * Zs + Ehat @ Zs
    # the tail: K^-1 -> K_mm -> Z~, lengthscales, variance; then the positivity transforms
    G2 = -(Kinv @ Kib @ Kinv) * Kmm
    Ws = -0.5 * (G2 + G2.T)
    np.fill_diagonal(Ws, 0.0)
    Ztbar = Ztbar + 2.0 * (Ws.sum(1)[:, None] * Zs - Ws @ Zs)
    g_var = (G2.sum() / var + gsig + glogsig / var) * sigmoid(p['variance_unc'])
    g_ls = -((Ztbar * Zs).sum(0) + glx) / ls * sigmoid(p['lengthscales_unc'])
    return {'g_mean': g_mean, 'g_cov': g_cov if cov is not None else None, 'g_zeta_pos': Ztbar / ls, 'g_zeta_mean': mubar,
            'g_zeta_var_unc': s2bar * sigmoid(p['zeta_var_unc']), 'g_variance_unc': np.reshape(g_var, np.shape(p['variance_unc'])),
            'g_lengthscales_unc': g_ls}


def rel_err(g, r):
    return mc.rel_err(g, r)
