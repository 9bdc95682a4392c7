"""Shared by the tests of the input gradients of GPModel.adf (`input_grads=True`): the cases of gp_ekf_cases.ALL_GPU_CASES
(55 cases, N = 21, T = 5, every row of gp_tile_grid.ROWS, the masks and the edges: nothing is redrawn), the loss and
`grad_names` of gp_ekf_grad_cases, and three codings of the gradients for m0, P0, a, y, var_x and var_y of

    loss = sum Wm o means + sum Wc o covs + sum Wl o loglik      ('full'; 'loglik' and 'last_mean' use one result each)

over the ADF recursion of tests/gp_adf_cases.py with the model held fixed:

  (a) torch float64 autograd through gp_mm_grad_cases.gram_moments and the JOINT update (solve, slogdet);
  (b) torch float64 autograd through gp_mm_grad_cases.inverse_moments and the Dy sequential scalar updates;
  (c) reverse_numpy: the reverse-time recursion the kernel runs, written out by hand in numpy -- the adjoint of the scalar
      updates (gp_ekf_bwd_kernel's S1 / S2 formulas), the cotangents of the moments (f = mb-, F = Pb-, X[:, :Do] = 2 Pb-), the
      carry with unfold / fold -- around the input adjoint of moment_match, which is taken as the vector-Jacobian product of
      gram_moments at the step's (x, S): that adjoint has its own three codings in tests/gp_mm_grad_cases.py.

(a) and (b) read P0 through its lower triangle, select the conditioned branch with torch.where and replace NaN in y before
use.  Rules: CPU, (a) against (b): CPU_RULE = 1e-7 of the largest entry (gp_ekf_grad_cases.CPU_RULE); GPU against (a):
gp_autograd_cases.within_rule, 1e-6.  Results are cached per case: treat them as read-only."""
import functools

import numpy as np
import torch

import gp_ekf_cases as ec
import gp_ekf_grad_cases as eg
import gp_mm_grad_cases as gg

CPU_RULE = eg.CPU_RULE
ALL_CASES = ec.ALL_GPU_CASES
PARTIAL_CASE = eg.PARTIAL_CASE
PARTIALS = eg.PARTIALS
FD_CASE = ec.case(30, 7, 5)
loss_of, grad_names, weights, leaves, rel_err = eg.loss_of, eg.grad_names, eg.weights, eg.leaves, eg.rel_err


@functools.lru_cache(maxsize=None)
def constants(c):
    return gg.model_constants(ec.make_inputs(c)['p'])


def adf_torch(c, moments, lv, joint):
    """the recursion in torch over moments(consts, mean, cov) -> (fmean, fcov, xcov); lv: the leaves that the case has"""
    M, D, Do, N, T, Dy, mask, with_vx, with_P0 = c
    i = ec.make_inputs(c)
    k = constants(c)
    m = lv['m0']
    P = gg.sym_lower(lv['P0']) if with_P0 else torch.zeros(N, Do, Do, dtype=torch.float64)
    vx = lv['var_x'] if with_vx else torch.zeros(Do, dtype=torch.float64)
    vy = lv['var_y']
    a = lv['a'] if D > Do else None
    ll = torch.zeros(N, dtype=torch.float64)
    means, covs = [], []
    for t in range(T):
        X = torch.cat([m, a[t]], 1) if D > Do else m
        S = torch.nn.functional.pad(P, (0, D - Do, 0, D - Do))                                  # blockdiag(P, 0)
        fmean, fcov, xcov = moments(k, X, S)
        Cx = xcov[:, :, :Do]
        m = m + fmean
        P = P + Cx + Cx.transpose(1, 2) + fcov + torch.diag_embed(vx.expand(N, Do))
        on = torch.ones(N, dtype=torch.bool) if i['cond'] is None else torch.tensor(i['cond'][t] != 0)
        y = torch.where(on[:, None], lv['y'][t], torch.zeros(N, Dy, dtype=torch.float64))      # NaN replaced before use
        if joint:
            Sy = P[:, :Dy, :Dy] + torch.diag(vy)
            dl = y - m[:, :Dy]
            PHt = P[:, :, :Dy]
            sol = torch.linalg.solve(Sy, dl[:, :, None])
            mc = m + (PHt @ sol)[:, :, 0]
            Pc = P - PHt @ torch.linalg.solve(Sy, PHt.transpose(1, 2))
            llc = ll - 0.5 * (Dy * np.log(2.0 * np.pi) + torch.linalg.slogdet(Sy)[1] + (dl * sol[:, :, 0]).sum(1))
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


@functools.lru_cache(maxsize=None)
def reference(c, which='full', coding='a'):
    """dict: means, covs, loglik, loss and the gradients 'g_' + name; (a) or (b)"""
    lv = leaves(c)
    means, covs, ll = adf_torch(c, gg.gram_moments if coding == 'a' else gg.inverse_moments, lv, coding == 'a')
    loss = loss_of(c, which, means, covs, ll)
    grads = torch.autograd.grad(loss, [lv[k] for k in lv], allow_unused=True)
    out = {'means': means.detach().numpy(), 'covs': covs.detach().numpy(), 'loglik': ll.detach().numpy(),
           'loss': float(loss.detach())}
    for k, g in zip(lv, grads):
        out['g_' + k] = (torch.zeros_like(lv[k]) if g is None else g).detach().numpy().copy()
    return out


def loss_numpy(c, over):
    """the 'full' loss of (a) with some inputs replaced: over = {name: numpy array}"""
    i = ec.make_inputs(c)
    lv = {k: torch.tensor(over.get(k, i[k]), dtype=torch.float64) for k in grad_names(c)}
    with torch.no_grad():
        return float(loss_of(c, 'full', *adf_torch(c, gg.gram_moments, lv, True)))


# ---- (c): the reverse-time recursion by hand
def _mm_vjp(k, x, S, gf, gF, gX):
    """(gmean, gcov in the lower-triangle convention) of moment_match at (x, S) for the three cotangents"""
    xt, St = torch.tensor(x, requires_grad=True), torch.tensor(S, requires_grad=True)
    fmean, fcov, xcov = gg.gram_moments(k, xt, St)
    loss = (torch.tensor(gf) * fmean).sum() + (torch.tensor(gF) * fcov).sum() + (torch.tensor(gX) * xcov).sum()
    gm, gc = torch.autograd.grad(loss, [xt, St])
    return gm.numpy(), gc.numpy()


def _unfold(g):
    low = np.tril(g, -1)
    return 0.5 * (low + low.transpose(0, 2, 1)) + g * np.eye(g.shape[-1])


def _fold(Pb):
    return 2.0 * np.tril(Pb, -1) + Pb * np.eye(Pb.shape[-1])


def reverse_numpy(c, which='full'):
    """dict of the gradients 'g_' + name by the four points of the derivation, from the forward records of (a)"""
    M, D, Do, N, T, Dy, mask, with_vx, with_P0 = c
    i = ec.make_inputs(c)
    k = constants(c)
    fwd = reference(c, which, 'a')
    Wm, Wc, Wl = weights(c)
    gmeans, gcovs, gll = np.zeros((T, N, Do)), np.zeros((T, N, Do, Do)), np.zeros(N)
    if which in ('full', 'last_mean'):
        gmeans[-1] = Wm[-1]
    if which == 'full':
        gmeans, gcovs = Wm.copy(), Wc.copy()
    if which in ('full', 'loglik'):
        gll = Wl.copy()
    P0 = np.zeros((N, Do, Do))
    if with_P0:
        P0 = np.tril(i['P0']) + np.tril(i['P0'], -1).transpose(0, 2, 1)
    vx = i['var_x'] if with_vx else np.zeros(Do)
    vy = i['var_y']
    y = np.nan_to_num(i['y'])
    out = {'g_a': np.zeros((T, N, D - Do)), 'g_y': np.zeros((T, N, Dy)), 'g_var_x': np.zeros(Do), 'g_var_y': np.zeros(Dy)}
    mb, Pb = np.zeros((N, Do)), np.zeros((N, Do, Do))
    for t in range(T - 1, -1, -1):
        mp, Pp = (fwd['means'][t - 1], fwd['covs'][t - 1]) if t > 0 else (i['m0'], P0)
        mb = mb + gmeans[t]
        Pb = Pb + 0.5 * (gcovs[t] + gcovs[t].transpose(0, 2, 1))
        # the predictive moments again: one step of the forward from the belief behind it
        S = np.zeros((N, D, D))
        S[:, :Do, :Do] = Pp
        x = np.concatenate([mp, i['a'][t]], 1)
        with torch.no_grad():
            fmean, fcov, xcov = (v.numpy() for v in gg.gram_moments(k, torch.tensor(x), torch.tensor(S)))
        Cx = xcov[:, :, :Do]
        m = mp + fmean
        P = Pp + Cx + Cx.transpose(0, 2, 1) + fcov + np.diag(vx)[None]
        on = np.ones(N, bool) if i['cond'] is None else (i['cond'][t] != 0)
        # 1. the scalar updates forward (keeping g_j, s_j, delta_j), then their adjoint, last first
        G, sj, dj = np.zeros((Dy, N, Do)), np.ones((Dy, N)), np.zeros((Dy, N))
        for j in range(Dy):
            sj[j] = P[:, j, j] + vy[j]
            dj[j] = np.where(on, y[t, :, j] - m[:, j], 0.0)
            G[j] = P[:, :, j] / sj[j][:, None]
            m = np.where(on[:, None], m + G[j] * dj[j][:, None], m)
            P = np.where(on[:, None, None], P - sj[j][:, None, None] * G[j][:, :, None] * G[j][:, None, :], P)
        for j in range(Dy - 1, -1, -1):
            g, s, dl = G[j], sj[j], dj[j]
            u = np.einsum('nik,nk->ni', Pb, g)
            gb = dl[:, None] * mb - 2.0 * s[:, None] * u
            db = (g * mb).sum(1) - gll * dl / s
            sb = -(g * u).sum(1) - (gb * g).sum(1) / s - 0.5 * gll * (1.0 / s - dl * dl / (s * s))
            h = np.where(on[:, None], 0.5 * gb / s[:, None], 0.0)
            Pb[:, :, j] += h
            Pb[:, j, :] += h
            Pb[:, j, j] += np.where(on, sb, 0.0)
            mb[:, j] -= np.where(on, db, 0.0)
            out['g_y'][t, :, j] = np.where(on, db, 0.0)
            out['g_var_y'][j] += np.where(on, sb, 0.0).sum()
        # 2. the transition; 3. the input adjoint of moment_match; 4. the carry
        out['g_var_x'] += np.einsum('nii->i', Pb)
        gX = np.zeros((N, Do, D))
        gX[:, :, :Do] = 2.0 * Pb
        gm, gc = _mm_vjp(k, x, S, mb, Pb, gX)
        out['g_a'][t] = gm[:, Do:]
        mb = mb + gm[:, :Do]
        Pb = Pb + _unfold(gc[:, :Do, :Do])
    out['g_m0'], out['g_P0'] = mb, _fold(Pb)
    return {k2: v for k2, v in out.items() if k2[2:] in grad_names(c)}
