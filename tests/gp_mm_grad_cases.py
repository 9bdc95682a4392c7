"""Shared by the tests of the input gradients of GPModel.moment_match (`input_grads=True`): the loss, its weights and two
CPU references in torch float64 of

    loss = sum Wf o fmean + sum Wc o fcov + sum Wx o xcov         (Wc is not symmetric)

with its gradients for `mean` and `cov`; the model is a constant.  Both read cov as tril(cov) + tril(cov, -1)^T, so the
gradient for cov is that of the function of the lower triangle: zero above the diagonal, both symmetric contributions on a
strictly lower entry.

  (a) gram_moments: Cholesky factors of A = I + S~ and B = I / 2 + S~, w_i = L1^-1 r_i, u_i = L2^-1 r_i,
      quad_ij = g_i + g_j + 2 u_i . u_j, and only (npts, M, M) intermediates -- fast enough for every row of gp_tile_grid.ROWS;
  (b) inverse_moments: the explicit-inverse coding of gp_moment_match_cases.closed_form restated in torch, with its
      (M, M, D) pair differences, point by point.

The beliefs are those of gp_moment_match_cases.make_beliefs; the weights are drawn per distinct belief, so they have period
37 where the beliefs do.  The partial variants use one result each ('fmean', 'fcov', 'xcov'); 'nocross' is the loss without
xcov.  Results are cached per case: treat them as read-only."""
import functools

import numpy as np
import torch

import gp_moment_match_cases as mc

VARIANTS = ('all', 'fmean', 'fcov', 'xcov', 'nocross')
CPU_RULE = 1e-7          # gp_ekf_grad_cases.CPU_RULE: (a) against (b), of the largest entry
GPU_RULE = 1e-6          # the project's rule for gradients (gp_autograd_cases.within_rule)


def make_weights(M, D, Do, npts):
    """(Wf (npts, Do), Wc (npts, Do, Do), Wx (npts, Do, D)), period 37 where the beliefs have it"""
    nd = mc.distinct_points(npts)
    rng = np.random.default_rng(9000 * M + 90 * D + Do + 1)
    Wf, Wc, Wx = rng.standard_normal((nd, Do)), rng.standard_normal((nd, Do, Do)), rng.standard_normal((nd, Do, D))
    if nd < npts:
        idx = np.arange(npts) % nd
        Wf, Wc, Wx = Wf[idx], Wc[idx], Wx[idx]
    return Wf, Wc, Wx


def model_constants(p):
    """the constants of the call in torch: ls, var, Zs, d2, Kinv, alpha, W (Do, M, M)"""
    ls = torch.tensor(mc.softplus(p['lengthscales_unc']))
    var = float(mc.softplus(p['variance_unc'])[0])
    s2, mu = torch.tensor(mc.softplus(p['zeta_var_unc'])), torch.tensor(p['zeta_mean'])
    Zs = torch.tensor(p['zeta_pos']) / ls
    M = Zs.shape[0]
    d2 = ((Zs[:, None, :] - Zs[None, :, :]) ** 2).sum(-1)
    K = var * torch.exp(-0.5 * d2) + mc.JITTER * torch.eye(M, dtype=torch.float64)
    Kinv = torch.linalg.inv(K)
    alpha = Kinv @ mu
    W = torch.stack([Kinv - (Kinv * s2[:, d][None, :]) @ Kinv for d in range(mu.shape[1])])
    return {'ls': ls, 'var': var, 'Zs': Zs, 'd2': d2, 'alpha': alpha, 'W': W}


def sym_lower(cov):
    """the function of the lower triangle"""
    return torch.tril(cov) + torch.tril(cov, -1).transpose(-1, -2)


def gram_moments(c, mean, cov):
    """(a): (fmean, fcov, xcov) of torch tensors mean (n, D), cov (n, D, D) or None, all points at once"""
    ls, var, Zs, d2, alpha, W = c['ls'], c['var'], c['Zs'], c['d2'], c['alpha'], c['W']
    n, D = mean.shape
    eye = torch.eye(D, dtype=torch.float64)
    St = (sym_lower(cov) if cov is not None else torch.zeros(n, D, D, dtype=torch.float64)) / ls[:, None] / ls[None, :]
    r = Zs[None] - (mean / ls)[:, None, :]                                          # (n, M, D)
    L1, L2 = torch.linalg.cholesky(eye + St), torch.linalg.cholesky(0.5 * eye + St)
    w = torch.linalg.solve_triangular(L1, r.transpose(1, 2), upper=False)           # (n, D, M)
    u = torch.linalg.solve_triangular(L2, r.transpose(1, 2), upper=False)
    c1 = var / torch.diagonal(L1, dim1=1, dim2=2).prod(1)
    c2 = var * var / (2.0 ** (0.5 * D) * torch.diagonal(L2, dim1=1, dim2=2).prod(1))
    q = c1[:, None] * torch.exp(-0.5 * (w * w).sum(1))                              # (n, M)
    g = (u * u).sum(1)
    quad = g[:, :, None] + g[:, None, :] + 2.0 * u.transpose(1, 2) @ u              # (n, M, M)
    Q = c2[:, None, None] * torch.exp(-0.25 * d2[None] - 0.125 * quad)
    fmean = q @ alpha
    tr = torch.einsum('dij,nij->nd', W, Q)
    fcov = alpha.T[None] @ Q @ alpha[None] - fmean[:, :, None] * fmean[:, None, :] + torch.diag_embed(var - tr)
    Hm = torch.einsum('nmk,nm,md->nkd', r, q, alpha)                                # (n, D, Do)
    AH = torch.cholesky_solve(Hm, L1)
    xcov = ((St @ AH) * ls[None, :, None]).transpose(1, 2)
    return fmean, fcov, xcov


def inverse_moments(c, mean, cov):
    """(b): the explicit-inverse coding of gp_moment_match_cases.closed_form, point by point"""
    ls, var, Zs, d2, alpha, W = c['ls'], c['var'], c['Zs'], c['d2'], c['alpha'], c['W']
    n, D = mean.shape
    eye = torch.eye(D, dtype=torch.float64)
    fm, fc, xc = [], [], []
    for i in range(n):
        S = sym_lower(cov[i]) if cov is not None else torch.zeros(D, D, dtype=torch.float64)
        St = S / ls[:, None] / ls[None, :]
        r = Zs - mean[i] / ls
        B1, B2 = torch.linalg.inv(eye + St), torch.linalg.inv(0.5 * eye + St)
        q = var / torch.sqrt(torch.linalg.det(eye + St)) * torch.exp(-0.5 * torch.einsum('id,de,ie->i', r, B1, r))
        f = alpha.T @ q
        rr = r[:, None, :] + r[None, :, :]
        quad = torch.einsum('ijd,ijd->ij', rr @ B2, rr)
        Q = var * var / torch.sqrt(torch.linalg.det(eye + 2.0 * St)) * torch.exp(-0.25 * d2 - 0.125 * quad)
        fm.append(f)
        fc.append(alpha.T @ Q @ alpha - torch.outer(f, f) + torch.diag(var - (W * Q[None]).sum((1, 2))))
        xc.append(((St @ B1 @ (r.T @ (alpha * q[:, None]))) * ls[:, None]).T)
    return torch.stack(fm), torch.stack(fc), torch.stack(xc)


def loss_of(out, weights, variant='all'):
    fmean, fcov, xcov = out
    Wf, Wc, Wx = (torch.as_tensor(w, dtype=torch.float64, device=fmean.device) for w in weights)
    terms = {'fmean': lambda: (Wf * fmean).sum(), 'fcov': lambda: (Wc * fcov).sum(), 'xcov': lambda: (Wx * xcov).sum()}
    use = {'all': ('fmean', 'fcov', 'xcov'), 'nocross': ('fmean', 'fcov')}.get(variant, (variant,))
    return sum(terms[k]() for k in use)


def evaluate(p, mean, cov, weights, variant='all', coding='gram'):
    """dict fmean, fcov, xcov, g_mean, g_cov (None without cov) as numpy, of one coding"""
    c = model_constants(p)
    mt = torch.tensor(np.asarray(mean), requires_grad=True)
    ct = torch.tensor(np.asarray(cov), requires_grad=True) if cov is not None else None
    out = (gram_moments if coding == 'gram' else inverse_moments)(c, mt, ct)
    loss_of(out, weights, variant).backward()
    res = {k: v.detach().numpy() for k, v in zip(('fmean', 'fcov', 'xcov'), out)}
    res['g_mean'] = mt.grad.numpy().copy()
    res['g_cov'] = ct.grad.numpy().copy() if ct is not None and ct.grad is not None else None
    return res


@functools.lru_cache(maxsize=None)
def reference(M, D, Do, npts, kind='mixed', variant='all', coding='gram'):
    """the reference of a case, computed once per distinct belief and shared (treat as read-only)"""
    nd = mc.distinct_points(npts)
    p, mean, cov, _ = mc.make_beliefs(M, D, Do, nd, kind)
    res = evaluate(p, mean, cov, make_weights(M, D, Do, nd), variant, coding)
    if nd < npts:
        idx = np.arange(npts) % nd
        res = {k: (v[idx] if v is not None else None) for k, v in res.items()}
    return res


def rel_err(g, r):
    return mc.rel_err(g, r)
