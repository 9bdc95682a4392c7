"""Shared by the GPModel.adf / GPModel.ads tests: three independent CPU references of the assumed-density filter

    for t in 0..T-1:
        x = concat(m, a[t]);  S = blockdiag(P, 0)
        fmean, fcov, xcov = moments of the GP under N(x, S);  Cx = xcov[:, :Do]
        m- = m + fmean;  cross[t] = P + Cx;  P- = P + Cx + Cx^T + fcov + diag(var_x);  pmeans[t], pcovs[t] = m-, P-
        where cond[t, n]: condition on y[t, n] = h[:Dy] + N(0, diag(var_y)), loglik[n] += log N(y; m-[:Dy], S_y)
        means[t], covs[t] = m, P

Cases and inputs are those of tests/gp_ekf_cases.py (case, make_inputs, GRID_CASES, MASK_CASES, EDGE_CASES,
CHAIN_GROUP_SHAPES; N = 21, T = 5): nothing is redrawn.

  (a) reference_joint: the GP moments by a coding that shares no route with gp_moment_match_cases.closed_form -- Cholesky
      factors and triangular solves for K_mm + jitter I, I + S~ and I / 2 + S~ (no explicit inverse; the pair exponent as
      g_i + g_j + 2 u_i . u_j of u = L2^-1 r, the traces of W_d Q through two factor solves of Q) -- and the JOINT Kalman
      update: a solve against S_y = H P- H^T + R and slogdet;
  (b) reference_sequential: closed_form per step on concat(m, a[t]) and blockdiag(P, 0), and the Dy sequential scalar
      updates the kernel runs;
  (c) reference_quadrature, Do <= 2 only: Gauss-Hermite quadrature over the state belief (a factor of P, Do-dimensional)
      through oracle/cbfssm_torch_ref.GPModel.predict -- E[h + f], Cov(h + f) + diag E[fvar], Cov(h + f, h) -- and the joint
      update.  It shares no formula with the closed form.

rts(fwd) is the Rauch-Tung-Striebel sweep in numpy over a forward reference, for GPModel.ads.

Rules: CPU, (a) against (b): 1e-9 of the largest entry of each tensor (test_gp_adf_cpu.py, every case the GPU file uses);
(c) against (b): 1e-8.  GPU against (b): 1e-8 of the largest entry of the reference tensor.  gp_ekf_cases.ILL_CANDIDATE
stays out, as it does for ekf.  Measured here, (a) against (b), the worst over all cases of the GPU file: 3.1e-10 (means),
2.6e-10 (covs), 2.0e-10 (loglik), 3.8e-10 (pmeans), 2.5e-10 (pcovs), 1.8e-10 (cross), all at (257, 6, 3); the next worst row
is (180, 6, 2) at 3.6e-11: no grid row is dropped.
Results are cached per case: treat them as read-only."""
import functools

import numpy as np
import scipy.linalg as sla
import torch

import gp_autograd_cases as gc
import gp_ekf_cases as ec
import gp_moment_match_cases as mc
import gp_tile_grid as grid
from gp_ekf_cases import case, make_inputs, GRID_CASES, MASK_CASES, EDGE_CASES, CHAIN_GROUP_SHAPES   # noqa: F401

JITTER = 1e-8
KEYS = ('means', 'covs', 'loglik', 'pmeans', 'pcovs', 'cross')
# every row of gp_tile_grid.ROWS meets the 1e-9 rule between (a) and (b): none is dropped
GRID_ROWS = list(grid.ROWS)
ALL_GPU_CASES = list(dict.fromkeys(GRID_CASES + MASK_CASES + EDGE_CASES))
SARCOS_CASE = case(100, 21, 14)
# (c): the two rows the rule names and one stash height with Do <= 2
QUAD_CASES = [case(50, 9, 2), case(64, 4, 1), case(113, 6, 2)]
QUAD_NODES = (48, 64)
# GPModel.ads: the masks, one grid row per LDS regime, Voliro's shape
ADS_ROWS = ('nb1_mid_dk6', 'nb7_kt3_dk6', 'nb20_mid_dk6')
ADS_CASES = list(dict.fromkeys(MASK_CASES + [ec.grid_case(grid.ROW_BY_NAME[r]) for r in ADS_ROWS] + [case(20, 19, 6, N=37, T=8)]))
# info: one chain's P0 replaced by -I
FAIL_CASE, FAIL_CHAIN = case(30, 7, 5, N=17), 11


def fail_P0():
    P0 = make_inputs(FAIL_CASE)['P0'].copy()
    P0[FAIL_CHAIN] = -np.eye(FAIL_CASE[2])
    return P0


# ---- the GP moments, coding (a)
def cholesky_moments(p, mean, cov):
    """fmean (n, Do), fcov (n, Do, Do), xcov (n, Do, D) for the beliefs N(mean[i], cov[i]) through factors and solves"""
    ls, var = mc.softplus(p['lengthscales_unc']), float(mc.softplus(p['variance_unc'])[0])
    s2, mu = mc.softplus(p['zeta_var_unc']), p['zeta_mean']
    M, D = p['zeta_pos'].shape
    Do = mu.shape[1]
    Zs = p['zeta_pos'] / ls
    G = Zs @ Zs.T
    d2 = np.maximum(np.diag(G)[:, None] + np.diag(G)[None, :] - 2.0 * G, 0.0)
    Lk = (np.linalg.cholesky(var * np.exp(-0.5 * d2) + JITTER * np.eye(M)), True)
    alpha = sla.cho_solve(Lk, mu)
    n = mean.shape[0]
    fmean, fcov, xcov = np.empty((n, Do)), np.empty((n, Do, Do)), np.empty((n, Do, D))
    eye = np.eye(D)
    for i in range(n):
        St = cov[i] / ls[:, None] / ls[None, :]
        r = Zs - mean[i] / ls
        L1, L2 = np.linalg.cholesky(eye + St), np.linalg.cholesky(0.5 * eye + St)
        w = sla.solve_triangular(L1, r.T, lower=True)
        u = sla.solve_triangular(L2, r.T, lower=True)
        q = var / np.prod(np.diag(L1)) * np.exp(-0.5 * (w * w).sum(0))
        g = (u * u).sum(0)
        Q = var * var / (2.0 ** (0.5 * D) * np.prod(np.diag(L2))) * np.exp(-0.25 * d2 - 0.125 * (g[:, None] + g[None, :] + 2.0 * u.T @ u))
        fm = alpha.T @ q
        X = sla.cho_solve(Lk, Q)                                                    # K^-1 Q
        Y = sla.cho_solve(Lk, X.T)                                                  # K^-1 Q K^-1
        fmean[i] = fm
        fcov[i] = alpha.T @ Q @ alpha - np.outer(fm, fm) + np.diag(var - np.trace(X) + s2.T @ np.diag(Y))
        v = r.T @ (alpha * q[:, None])                                              # (D, Do)
        xcov[i] = ((St @ sla.cho_solve((L1, True), v)) * ls[:, None]).T
    return fmean, fcov, xcov


# ---- the recursion
def _update(c, i, t, m, P, ll, joint):
    N, Dy = c[3], c[5]
    vy = i['var_y']
    on = np.ones(N, bool) if i['cond'] is None else (i['cond'][t] != 0)
    for n in np.nonzero(on)[0]:
        y = i['y'][t, n]
        if joint:
            S = P[n, :Dy, :Dy] + np.diag(vy)
            dl = y - m[n, :Dy]
            PHt = P[n][:, :Dy]
            m[n] = m[n] + PHt @ np.linalg.solve(S, dl)
            P[n] = P[n] - PHt @ np.linalg.solve(S, PHt.T)
            ll[n] -= 0.5 * (Dy * np.log(2.0 * np.pi) + np.linalg.slogdet(S)[1] + dl @ np.linalg.solve(S, dl))
        else:
            for j in range(Dy):
                s = P[n, j, j] + vy[j]
                dl = y[j] - m[n, j]
                g = P[n, :, j] / s
                m[n] = m[n] + g * dl
                P[n] = P[n] - s * np.outer(g, g)
                ll[n] -= 0.5 * (np.log(2.0 * np.pi * s) + dl * dl / s)


def _run(c, step, joint, scale=1.0):
    """the recursion over step(m, P, a_t) -> (m-, P- without var_x, cross); scale multiplies P0 and var_x"""
    M, D, Do, N, T, Dy, mask, with_vx, with_P0 = c
    i = make_inputs(c)
    m = i['m0'].copy()
    P = scale * i['P0'] if with_P0 else np.zeros((N, Do, Do))
    vx = scale * i['var_x'] if with_vx else np.zeros(Do)
    out = {k: np.empty((T, N, Do)) for k in ('means', 'pmeans')}
    out.update({k: np.empty((T, N, Do, Do)) for k in ('covs', 'pcovs', 'cross')})
    out.update(loglik=np.zeros(N), m0=m.copy(), P0=P.copy())
    for t in range(T):
        m, P, out['cross'][t] = step(m, P, i['a'][t])
        m, P = m.copy(), P.copy()
        P[:, np.arange(Do), np.arange(Do)] += vx
        out['pmeans'][t], out['pcovs'][t] = m, P
        _update(c, i, t, m, P, out['loglik'], joint)
        out['means'][t], out['covs'][t] = m, P
    return out


def _closed_step(c, moments):
    D, Do = c[1], c[2]
    p = make_inputs(c)['p']

    def step(m, P, a):
        S = np.zeros((m.shape[0], D, D))
        S[:, :Do, :Do] = P
        fmean, fcov, xcov = moments(p, np.concatenate([m, a], 1), S)
        Cx = xcov[:, :, :Do]
        return m + fmean, P + Cx + Cx.transpose(0, 2, 1) + fcov, P + Cx
    return step


@functools.lru_cache(maxsize=None)
def reference_joint(c):
    """(a)"""
    return _run(c, _closed_step(c, cholesky_moments), True)


def _closed(p, mean, cov):
    r = mc.closed_form(p, mean, cov)
    return r['fmean'], r['fcov'], r['xcov']


@functools.lru_cache(maxsize=None)
def reference_sequential(c, scale=1.0):
    """(b)"""
    return _run(c, _closed_step(c, _closed), False, scale)


@functools.lru_cache(maxsize=None)
def reference_quadrature(c, nodes, scale=1.0):
    """(c)"""
    Do = c[2]
    assert Do <= 2
    _, gp = gc.oracle_model(make_inputs(c)['p'])
    x, w = np.polynomial.hermite_e.hermegauss(nodes)
    w = w / np.sqrt(2.0 * np.pi)
    Gn = np.stack(np.meshgrid(*([x] * Do), indexing='ij'), -1).reshape(-1, Do)
    ww = np.prod(np.stack(np.meshgrid(*([w] * Do), indexing='ij'), -1).reshape(-1, Do), 1)

    def step(m, P, a):
        N = m.shape[0]
        mp, Pp, cr = np.empty((N, Do)), np.empty((N, Do, Do)), np.empty((N, Do, Do))
        for n in range(N):
            ev, V = np.linalg.eigh(P[n])
            F = V * np.sqrt(np.maximum(ev, 0.0))                                    # P = F F^T
            h = m[n] + Gn @ F.T
            with torch.no_grad():
                f, fv = gp.predict(torch.tensor(np.concatenate([h, np.broadcast_to(a[n], (h.shape[0], a.shape[1]))], 1)))
            hn = h + f.numpy()
            E = ww @ hn
            mp[n] = E
            Pp[n] = (hn * ww[:, None]).T @ hn - np.outer(E, E) + np.diag(ww @ fv.numpy())
            cr[n] = (hn - E).T @ ((h - m[n]) * ww[:, None])                         # Cov(h+, h): row = new state
        return mp, Pp, cr
    return _run(c, step, True, scale)


def rts(f, lag_one=True):
    """the Rauch-Tung-Striebel sweep over a forward reference: smeans, scovs, init_mean, init_cov, lag_one"""
    T = f['means'].shape[0]
    ms, Ps = f['means'][T - 1], f['covs'][T - 1]
    smeans, scovs, lag1 = np.empty_like(f['means']), np.empty_like(f['covs']), np.empty_like(f['covs'])
    smeans[T - 1], scovs[T - 1] = ms, Ps
    for t in range(T - 1, -1, -1):
        mf, Pf = (f['means'][t - 1], f['covs'][t - 1]) if t > 0 else (f['m0'], f['P0'])
        G = np.linalg.solve(f['pcovs'][t], f['cross'][t]).transpose(0, 2, 1)        # cross[t]^T (P-_t)^-1, P- symmetric
        lag1[t] = G @ Ps
        ms = mf + (G @ (ms - f['pmeans'][t])[:, :, None])[:, :, 0]
        Ps = Pf + G @ (Ps - f['pcovs'][t]) @ G.transpose(0, 2, 1)
        if t > 0:
            smeans[t - 1], scovs[t - 1] = ms, Ps
    return {'smeans': smeans, 'scovs': scovs, 'init_mean': ms, 'init_cov': Ps, 'lag_one': lag1}


@functools.lru_cache(maxsize=None)
def reference_rts(c):
    return rts(reference_sequential(c))


def rel_err(g, r):
    """largest deviation over the largest entry of the reference; an all-zero reference must be met exactly"""
    g, r = np.asarray(g), np.asarray(r)
    scale = np.abs(r).max()
    return float(np.abs(g - r).max() / scale) if scale > 0 else float(np.abs(g).max())


def agreement(a, b):
    """{key: a against b} over KEYS"""
    return {k: rel_err(a[k], b[k]) for k in KEYS}


def min_eig(covs):
    """(smallest eigenvalue of any matrix of covs, the largest |entry|)"""
    return float(np.linalg.eigvalsh(0.5 * (covs + np.swapaxes(covs, -1, -2))).min()), float(np.abs(covs).max())


# ---- the compiled tree of the ADF launcher, from the source text
def compiled_leaves():
    """every (NBLK, DK) the gpadf_nb*.hip units and launch_gp_adf_n instantiate"""
    import tile_grid as tg
    heights = grid._instantiated('CBF_GPADF_INSTANTIATE')
    dks = grid._case_values(tg._read('cbfssm_gp_adf.hpp'), 'launch_gp_adf_n')
    return {(nb, dk) for nb in heights for dk in dks}
