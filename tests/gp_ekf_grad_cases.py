"""Shared by the tests of the differentiable GPModel.ekf: the cases of gp_ekf_cases (GRID_CASES, MASK_CASES, EDGE_CASES), their
inputs (gp_ekf_cases.make_inputs), the loss and two independent CPU references of its gradients in torch float64.

Loss: sum Wm o means + sum Wc o covs + sum Wl o loglik with fixed random weights from default_rng(11 + M + T), drawn in this
order; Wc is NOT symmetric.  `which` picks the cotangents: 'full' (all three), 'loglik' (only loglik is used) and 'last_mean'
(only means[-1] is used).

  (a) the oracle's GPModel.predict (triangular solves), J by torch.autograd.grad(..., create_graph=True) one output dimension
      at a time, the JOINT update with torch.linalg.solve and slogdet;
  (b) gp_rollout_cases.second_coding (explicit inverse of K_mm + jitter I), J the same way through that coding, and the Dy
      sequential scalar updates the kernel runs.

Both read P0 as tril(P0) + tril(P0, -1)^T, select the conditioned branch with torch.where and replace NaN in y before use.
Gradients: 'm0', 'P0', 'a', 'y', 'var_x', 'var_y' (those the case has) and the five parameter tensors.

Rules: CPU, (a) against (b): every gradient tensor within 1e-7 of its largest entry (ten times inside the GPU rule).  GPU
against (a): gp_autograd_cases.within_rule, 1e-6 of the largest entry of the reference tensor.  Results are cached per case:
treat them as read-only."""
import functools

import numpy as np
import torch

import gp_autograd_cases as gc
import gp_ekf_cases as ec
import gp_rollout_cases as rc

PARAMS = gc.PARAMS
CPU_RULE = 1e-7
ALL_CASES = ec.ALL_GPU_CASES
TRAIN_CASE = ec.case(30, 7, 5)
PARTIAL_CASE = ec.case(30, 7, 5)
PARTIALS = ('loglik', 'last_mean')


def weights(c):
    M, D, Do, N, T, Dy = c[:6]
    rng = np.random.default_rng(11 + M + T)
    return rng.standard_normal((T, N, Do)), rng.standard_normal((T, N, Do, Do)), rng.standard_normal(N)


def loss_of(c, which, means, covs, loglik):
    """the case's loss from three torch tensors on any device"""
    Wm, Wc, Wl = (torch.tensor(w, dtype=torch.float64, device=means.device) for w in weights(c))
    if which == 'loglik':
        return (Wl * loglik).sum()
    if which == 'last_mean':
        return (Wm[-1] * means[-1]).sum()
    return (Wm * means).sum() + (Wc * covs).sum() + (Wl * loglik).sum()


def grad_names(c):
    M, D, Do, N, T, Dy, mask, with_vx, with_P0 = c
    return (['m0'] + (['P0'] if with_P0 else []) + (['a'] if D > Do else []) + ['y'] + (['var_x'] if with_vx else [])
            + ['var_y'])


def ekf_torch(c, predict, lv, joint):
    """the recursion in torch over predict(X) -> (fmean, fvar); lv: the leaves m0, P0, a, y, var_x, var_y (those present)"""
    M, D, Do, N, T, Dy, mask, with_vx, with_P0 = c
    i = ec.make_inputs(c)
    m = lv['m0']
    if with_P0:
        P = torch.tril(lv['P0']) + torch.tril(lv['P0'], -1).transpose(1, 2)
    else:
        P = torch.zeros(N, Do, Do, dtype=torch.float64)
    vx = lv['var_x'] if with_vx else torch.zeros(Do, dtype=torch.float64)
    vy = lv['var_y']
    eye = torch.eye(Do, dtype=torch.float64)
    ll = torch.zeros(N, dtype=torch.float64)
    means, covs = [], []
    for t in range(T):
        X = torch.cat([m, lv['a'][t]], 1) if D > Do else m
        fmean, fvar = predict(X)
        J = torch.stack([torch.autograd.grad(fmean[:, d].sum(), X, create_graph=True)[0][:, :Do] for d in range(Do)], 1)
        A = eye[None] + J
        m = m + fmean
        P = A @ P @ A.transpose(1, 2) + torch.diag_embed(fvar + vx)
        on = torch.ones(N, dtype=torch.bool) if i['cond'] is None else torch.tensor(i['cond'][t] != 0)
        y = torch.where(on[:, None], lv['y'][t], torch.zeros(N, Dy, dtype=torch.float64))      # NaN replaced before use
        if joint:
            S = P[:, :Dy, :Dy] + torch.diag(vy)
            dl = y - m[:, :Dy]
            PHt = P[:, :, :Dy]
            sol = torch.linalg.solve(S, dl[:, :, None])
            mc = m + (PHt @ sol)[:, :, 0]
            Pc = P - PHt @ torch.linalg.solve(S, PHt.transpose(1, 2))
            llc = ll - 0.5 * (Dy * np.log(2.0 * np.pi) + torch.linalg.slogdet(S)[1] + (dl * sol[:, :, 0]).sum(1))
        else:
            mc, Pc, llc = m, P, ll
            for j in range(Dy):
                s = Pc[:, j, j] + vy[j]
                dj = y[:, j] - mc[:, j]
                g = Pc[:, :, j] / s[:, None]
                mc = mc + g * dj[:, None]
                Pc = Pc - s[:, None, None] * g[:, :, None] * g[:, None, :]
                llc = llc - 0.5 * (torch.log(2.0 * np.pi * s) + dj * dj / s)
        m = torch.where(on[:, None], mc, m)
        P = torch.where(on[:, None, None], Pc, P)
        ll = torch.where(on, llc, ll)
        means.append(m)
        covs.append(P)
    return torch.stack(means), torch.stack(covs), ll


def leaves(c, device='cpu'):
    """the differentiable inputs of a case as torch leaves (y keeps its NaN)"""
    i = ec.make_inputs(c)
    lv = {}
    for k in grad_names(c):
        lv[k] = torch.tensor(i[k], dtype=torch.float64, device=device, requires_grad=True)
    return lv


@functools.lru_cache(maxsize=None)
def reference(c, which='full', coding='a'):
    """dict: means, covs, loglik, loss and the gradients 'g_' + name; (a) or (b)"""
    t, gp = gc.oracle_model(ec.make_inputs(c)['p'])
    lv = leaves(c)
    predict = gp.predict if coding == 'a' else rc.second_coding(t)
    means, covs, ll = ekf_torch(c, predict, lv, coding == 'a')
    loss = loss_of(c, which, means, covs, ll)
    names = list(lv) + list(PARAMS)
    grads = torch.autograd.grad(loss, [lv[k] for k in lv] + [t[k] for k in PARAMS], allow_unused=True)
    out = {'means': means.detach().numpy(), 'covs': covs.detach().numpy(), 'loglik': ll.detach().numpy(),
           'loss': float(loss.detach())}
    for k, g in zip(names, grads):
        ref = lv[k] if k in lv else t[k]
        out['g_' + k] = (torch.zeros_like(ref) if g is None else g).detach().numpy().copy()
    return out


def rel_err(g, r):
    """largest deviation over the largest entry of the reference; an all-zero reference must be met exactly"""
    g, r = np.asarray(g), np.asarray(r)
    scale = np.abs(r).max() if r.size else 0.0
    if scale == 0.0:
        return float(np.abs(g).max()) if g.size else 0.0
    return float(np.abs(g - r).max() / scale)
