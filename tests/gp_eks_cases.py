"""Shared by the GPModel.eks tests: two independent CPU references of the smoothed posterior behind the extended Kalman
filter of tests/gp_ekf_cases.py.  Cases and inputs are gp_ekf_cases.ALL_GPU_CASES / make_inputs, unchanged.

forward(c) is a forward recursion of its own (the oracle's predict, Jacobians by autodiff, the joint Kalman update) that
also keeps A_t, m-_t, P-_t of every step; its filtered outputs equal gp_ekf_cases.reference_joint to 1e-12
(test_gp_eks_cpu.py).  With time -1 the initial belief (m0, P0):

  (a) reference_rts: the Rauch-Tung-Striebel recursion, for t = T-1 .. 0 from (ms, Ps)[T-1] = (m, P)[T-1]

          G = (A_t P_{t-1})^T (P-_t)^-1  (np.linalg.solve);  ms[t-1] = m[t-1] + G (ms[t] - m-_t)
          Ps[t-1] = P[t-1] + G (Ps[t] - P-_t) G^T;  lag1[t] = G Ps[t]

  (b) reference_dense: no backward recursion at all.  Per chain the linear-Gaussian model x_t = A_t x_{t-1} + c_t + w_t,
      c_t = m-_t - A_t m_{t-1}, w_t ~ N(0, diag(fv_t + var_x)), linearised at (a)'s filtered means; the joint mean and the
      (T+1)Do x (T+1)Do covariance of (x_{-1}, .., x_{T-1}); conditioned on every observed y at once with one dense solve;
      the marginal blocks and the first off-diagonal blocks read off.

Rules: CPU, (a) against (b): 1e-9 of the largest entry of each tensor.  GPU against (a): 1e-8 of the largest entry of the
reference tensor -- the trajectory rule of the rollout, filter and ekf tests.  Results are cached per case: treat them as
read-only.

FAIL_CASE: one chain whose P0 is -4 I, so that P-_0 of that chain is not positive definite and the factorisation fails."""
import functools

import numpy as np
import torch

import gp_autograd_cases as gc
import gp_ekf_cases as ec

ALL_GPU_CASES = ec.ALL_GPU_CASES
KEYS = ('smeans', 'scovs', 'init_mean', 'init_cov', 'pmeans', 'pcovs', 'lag_one')
FAIL_CASE, FAIL_CHAIN = ec.case(30, 7, 5, T=1, mask='zeros'), 3


def fail_P0():
    P0 = ec.make_inputs(FAIL_CASE)['P0'].copy()
    P0[FAIL_CHAIN] = -4.0 * np.eye(FAIL_CASE[2])
    return P0


def _forward(c, P0):
    M, D, Do, N, T, Dy, mask, with_vx, with_P0 = c
    i = ec.make_inputs(c)
    _, gp = gc.oracle_model(i['p'])
    m = i['m0'].copy()
    P = np.zeros((N, Do, Do)) if P0 is None else P0.copy()
    vx = i['var_x'] if with_vx else np.zeros(Do)
    vy, eye = i['var_y'], np.eye(Do)
    out = {k: np.empty((T, N, Do)) for k in ('means', 'pmeans', 'Q')}
    out.update({k: np.empty((T, N, Do, Do)) for k in ('covs', 'pcovs', 'A')})
    out.update(loglik=np.zeros(N), m0=m.copy(), P0=P.copy())
    for t in range(T):
        Xt = torch.tensor(np.concatenate([m, i['a'][t]], 1), requires_grad=True)
        fmean, fvar = gp.predict(Xt)
        A = np.empty((N, Do, Do))
        for d in range(Do):
            A[:, d, :] = torch.autograd.grad(fmean[:, d].sum(), Xt, retain_graph=True)[0].numpy()[:, :Do]
        A += eye[None]
        Q = fvar.detach().numpy() + vx
        m = m + fmean.detach().numpy()
        P = A @ P @ A.transpose(0, 2, 1)
        P[:, np.arange(Do), np.arange(Do)] += Q
        out['A'][t], out['Q'][t], out['pmeans'][t], out['pcovs'][t] = A, Q, m, P
        on = np.ones(N, bool) if i['cond'] is None else (i['cond'][t] != 0)
        for n in np.nonzero(on)[0]:
            S = P[n, :Dy, :Dy] + np.diag(vy)
            dl = i['y'][t, n] - m[n, :Dy]
            PHt = P[n][:, :Dy]
            m[n] = m[n] + PHt @ np.linalg.solve(S, dl)
            P[n] = P[n] - PHt @ np.linalg.solve(S, PHt.T)
            out['loglik'][n] -= 0.5 * (Dy * np.log(2.0 * np.pi) + np.linalg.slogdet(S)[1] + dl @ np.linalg.solve(S, dl))
        out['means'][t], out['covs'][t] = m, P
    return out


@functools.lru_cache(maxsize=None)
def forward(c):
    """means, covs, loglik as gp_ekf_cases.reference_joint, and pmeans, pcovs, A (T, N, Do, Do), Q (T, N, Do), m0, P0"""
    return _forward(c, ec.make_inputs(c)['P0'])


@functools.lru_cache(maxsize=None)
def forward_failing():
    """forward(FAIL_CASE) with P0[FAIL_CHAIN] = -4 I"""
    return _forward(FAIL_CASE, fail_P0())


@functools.lru_cache(maxsize=None)
def reference_rts(c):
    """(a): dict of smeans, scovs, init_mean, init_cov, pmeans, pcovs, lag_one"""
    f = forward(c)
    T = c[4]
    ms, Ps = f['means'][T - 1], f['covs'][T - 1]
    smeans, scovs, lag1 = np.empty_like(f['means']), np.empty_like(f['covs']), np.empty_like(f['covs'])
    smeans[T - 1], scovs[T - 1] = ms, Ps
    for t in range(T - 1, -1, -1):
        mf, Pf = (f['means'][t - 1], f['covs'][t - 1]) if t > 0 else (f['m0'], f['P0'])
        cross = f['A'][t] @ Pf                                                  # A_t P_{t-1}
        G = np.linalg.solve(f['pcovs'][t], cross).transpose(0, 2, 1)            # P- symmetric: (P-^-1 cross)^T
        lag1[t] = G @ Ps
        ms = mf + (G @ (ms - f['pmeans'][t])[:, :, None])[:, :, 0]
        Ps = Pf + G @ (Ps - f['pcovs'][t]) @ G.transpose(0, 2, 1)
        if t > 0:
            smeans[t - 1], scovs[t - 1] = ms, Ps
    return {'smeans': smeans, 'scovs': scovs, 'init_mean': ms, 'init_cov': Ps, 'pmeans': f['pmeans'], 'pcovs': f['pcovs'],
            'lag_one': lag1}


@functools.lru_cache(maxsize=None)
def reference_dense(c):
    """(b): the same dict (pmeans, pcovs: the prior marginals of the joint model are not these, so they are left out)"""
    M, D, Do, N, T, Dy = c[:6]
    f, i = forward(c), ec.make_inputs(c)
    K = (T + 1) * Do
    blk = lambda s: slice((s + 1) * Do, (s + 2) * Do)                           # time s = -1 .. T-1
    smeans, scovs, lag1 = np.empty((T, N, Do)), np.empty((T, N, Do, Do)), np.empty((T, N, Do, Do))
    im, iP = np.empty((N, Do)), np.empty((N, Do, Do))
    for n in range(N):
        mu, S = np.zeros(K), np.zeros((K, K))
        mu[blk(-1)], S[blk(-1), blk(-1)] = f['m0'][n], f['P0'][n]
        for t in range(T):
            A = f['A'][t, n]
            mprev = f['means'][t - 1, n] if t > 0 else f['m0'][n]
            mu[blk(t)] = A @ mu[blk(t - 1)] + (f['pmeans'][t, n] - A @ mprev)
            row = A @ S[blk(t - 1), :blk(t - 1).stop]                           # Cov(x_t, x_s), s < t
            S[blk(t), :blk(t - 1).stop] = row
            S[:blk(t - 1).stop, blk(t)] = row.T
            S[blk(t), blk(t)] = A @ S[blk(t - 1), blk(t - 1)] @ A.T + np.diag(f['Q'][t, n])
        obs = [t for t in range(T) if i['cond'] is None or i['cond'][t, n] != 0]
        if obs:
            idx = np.concatenate([np.arange(blk(t).start, blk(t).start + Dy) for t in obs])
            yy = np.concatenate([i['y'][t, n] for t in obs])
            Syy = S[np.ix_(idx, idx)] + np.diag(np.tile(i['var_y'], len(obs)))
            Sxy = S[:, idx]
            mu = mu + Sxy @ np.linalg.solve(Syy, yy - mu[idx])
            S = S - Sxy @ np.linalg.solve(Syy, Sxy.T)
        im[n], iP[n] = mu[blk(-1)], S[blk(-1), blk(-1)]
        for t in range(T):
            smeans[t, n], scovs[t, n], lag1[t, n] = mu[blk(t)], S[blk(t), blk(t)], S[blk(t - 1), blk(t)]
    return {'smeans': smeans, 'scovs': scovs, 'init_mean': im, 'init_cov': iP, 'lag_one': lag1}


def rel_err(g, r):
    """largest deviation over the largest entry of the reference; an all-zero reference must be met exactly"""
    g, r = np.asarray(g), np.asarray(r)
    scale = np.abs(r).max()
    return float(np.abs(g - r).max() / scale) if scale > 0 else float(np.abs(g).max())


def agreement(c):
    a, b = reference_rts(c), reference_dense(c)
    return {k: rel_err(a[k], b[k]) for k in b}
