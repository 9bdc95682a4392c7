"""Shared by the full-covariance q(z) tests: the cases, their inputs, and the reference -- CPU float64 reverse-mode
autodiff of a restatement of the conditional with q_sqrt of shape (Do, M, M) in the reference's order (gp_tf.py:76-98:
Cholesky, two triangular solves, LTA = L_d^T A) with the KL in closed form.  `second_coding` is an independent coding of
the same function (explicit K^-1, S_d = L_d L_d^T, torch.distributions.kl_divergence of two MultivariateNormals) that
tests/test_gp_fullq_cpu.py holds the reference against.

Everything but q comes from gp_autograd_cases.make_inputs.  q (Do, M, M), with rng = default_rng(7 + M): strictly lower
part 0.03 N(0, 1); diagonal 0.2 exp(U(-0.5, 0.5)) times a random sign (negative diagonal entries are legal: only L L^T and
log L_ii^2 enter); standard-normal garbage above the diagonal, which nothing may read.

The loss of every case is  sum(Wm o fmean) + sum(Wv o fvar) + 0.3 prior_kl, as in gp_autograd_cases.
On a subset of these cases the two codings agree to 1.1e-12 of the largest entry of every gradient tensor (worst: X at
(300, 6, 4, 41), cond(K) 1.6e5; a few 1e-14 elsewhere), so the reference sits six orders inside the 1e-6 rule and no entry
is masked."""
import functools

import numpy as np
import torch

import gp_autograd_cases as gc

PARAMS = ('zeta_pos', 'zeta_mean', 'zeta_sqrt', 'variance_unc', 'lengthscales_unc')
KL_WEIGHT = gc.KL_WEIGHT
JITTER = 1e-8

# (M, D, Do, npts): the smallest shapes at which each mechanism can go wrong
CASES = [
    (12, 4, 3, 41),                # one row block, ragged columns
    (64, 16, 8, 1),                # one point
    (100, 21, 14, 41),             # the Sarcos tile, seven row blocks, K^-1 in registers
    (112, 24, 16, 50),             # every limit of the register path at once
    (113, 9, 1, 17),               # first stash height, Do = 1
    (200, 13, 7, 41),              # 13 row blocks, two per wave
    (300, 6, 4, 41),               # 20 row blocks
    (320, 6, 16, 33),              # the largest pack and q, 13 MB
    (100, 21, 14, 16 * 600 + 5),   # many column blocks per persistent workgroup, and the slice sum of W_d
]


def make_q(M, Do):
    rng = np.random.default_rng(7 + M)
    q = np.tril(0.03 * rng.standard_normal((Do, M, M)), -1)
    diag = 0.2 * np.exp(rng.uniform(-0.5, 0.5, (Do, M))) * rng.choice([-1.0, 1.0], (Do, M))
    q = q + diag[:, :, None] * np.eye(M)[None]
    garbage = np.triu(rng.standard_normal((Do, M, M)), 1)
    return q + garbage


def make_inputs(M, D, Do, npts):
    """(p, X, Wm, Wv): p as gp_autograd_cases.make_inputs with 'zeta_sqrt' (Do, M, M) in place of 'zeta_var_unc'"""
    p, X, Wm, Wv = gc.make_inputs(M, D, Do, npts)
    p = dict(p)
    del p['zeta_var_unc']
    p['zeta_sqrt'] = make_q(M, Do)
    return p, X, Wm, Wv


def _softplus(x):
    return torch.nn.functional.softplus(x) + 1e-10                   # tf_transform.py:19-21


def _rbf(X, X2, var, ls):
    """gp_tf.py:33-49: the reference's expansion on lengthscale-scaled inputs"""
    a, b = X / ls, X2 / ls
    d2 = -2.0 * a @ b.T + (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :]
    return var * torch.exp(-0.5 * d2)


def restatement(t, X):
    """(fmean (N, Do), fvar (N, Do), kl) in the reference's order of operations; t: dict of torch tensors by PARAMS"""
    Z, f, q = t['zeta_pos'], t['zeta_mean'], t['zeta_sqrt']
    var, ls = _softplus(t['variance_unc']).reshape(()), _softplus(t['lengthscales_unc'])
    M, Do = f.shape
    Lq = torch.tril(q)
    Lm = torch.linalg.cholesky(_rbf(Z, Z, var, ls) + JITTER * torch.eye(M, dtype=torch.float64))   # :72-73
    Kmn = _rbf(Z, X, var, ls)                                                                        # :71
    A = torch.linalg.solve_triangular(Lm, Kmn, upper=False)                                          # :76
    fvar = var - (A * A).sum(0)                                                                      # :79
    A = torch.linalg.solve_triangular(Lm.T, A, upper=True)                                           # :84
    fmean = A.T @ f                                                                                  # :87
    LTA = Lq.transpose(1, 2) @ A[None]                                                               # :93-94
    fvar = fvar[None, :] + (LTA * LTA).sum(1)                                                        # :98
    # KL(N(f_d, L_d L_d^T) || N(0, K)) in closed form
    B = torch.linalg.solve_triangular(Lm, Lq, upper=False)              # Lm^-1 L_d: tr(K^-1 S_d) = |B|_F^2
    a = torch.linalg.solve_triangular(Lm, f, upper=False)               # f_d^T K^-1 f_d = |Lm^-1 f_d|^2
    logdetK = 2.0 * torch.log(torch.diagonal(Lm)).sum()
    dq = torch.diagonal(Lq, dim1=1, dim2=2)
    kl = 0.5 * ((B * B).sum() + (a * a).sum() - Do * M + Do * logdetK - torch.log(dq * dq).sum())
    return fmean, fvar.T, kl


def second_coding(t, X):
    """the same function, coded independently: explicit inverse, S_d, torch.distributions"""
    Z, f, q = t['zeta_pos'], t['zeta_mean'], t['zeta_sqrt']
    var, ls = _softplus(t['variance_unc']).reshape(()), _softplus(t['lengthscales_unc'])
    M, Do = f.shape
    K = _rbf(Z, Z, var, ls) + JITTER * torch.eye(M, dtype=torch.float64)
    Kinv = torch.linalg.inv(K)
    k = _rbf(Z, X, var, ls)
    A2 = Kinv @ k
    S = torch.tril(q) @ torch.tril(q).transpose(1, 2)
    fmean = A2.T @ f
    fvar = var - (k * A2).sum(0)[:, None] + torch.einsum('mn,dmk,kn->nd', A2, S, A2)
    D = torch.distributions
    post = D.MultivariateNormal(f.T, covariance_matrix=S)
    prior = D.MultivariateNormal(torch.zeros(Do, M, dtype=torch.float64), covariance_matrix=K[None].repeat(Do, 1, 1))
    return fmean, fvar, D.kl_divergence(post, prior).sum()


def tensors(p, requires_grad=True):
    return {k: torch.tensor(p[k], dtype=torch.float64, requires_grad=requires_grad) for k in PARAMS}


def _differentiate(fn, M, D, Do, npts):
    p, X, Wm, Wv = make_inputs(M, D, Do, npts)
    t = tensors(p)
    Xt = torch.tensor(X, requires_grad=True)
    fmean, fvar, kl = fn(t, Xt)
    loss = (torch.tensor(Wm) * fmean).sum() + (torch.tensor(Wv) * fvar).sum() + KL_WEIGHT * kl
    loss.backward()
    out = {'fmean': fmean.detach().numpy(), 'fvar': fvar.detach().numpy(), 'kl': float(kl.detach()), 'g_X': Xt.grad.numpy().copy()}
    for k in PARAMS:
        out['g_' + k] = t[k].grad.numpy().copy()
    t2 = tensors(p)
    fn(t2, torch.tensor(X))[2].backward()
    for k in PARAMS:
        out['k_' + k] = t2[k].grad.numpy().copy()
    return out


@functools.lru_cache(maxsize=None)
def reference(M, D, Do, npts):
    """dict: fmean, fvar, kl, the gradients of the case's loss ('g_' + name, 'g_X') and of prior_kl alone ('k_' + name);
    computed once per case and shared (treat as read-only)"""
    return _differentiate(restatement, M, D, Do, npts)


@functools.lru_cache(maxsize=None)
def reference2(M, D, Do, npts):
    """the same quantities from the second coding"""
    return _differentiate(second_coding, M, D, Do, npts)


within_rule = gc.within_rule
