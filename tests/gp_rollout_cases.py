"""Shared by the GP-rollout tests: the cases, their inputs, and the reference -- the recurrence

    for t in 0..T-1 (reverse: T-1..0):  fmean, fvar = gp.predict(concat(h, a[t]));  v = fvar + var_add
                                        h = h + fmean + eps[t][:, None] sqrt(v);  traj[t] = h;  entropy += 0.5 sum log(2 pi e v)

written over oracle/cbfssm_torch_ref.GPModel on the CPU, differentiated by reverse-mode autodiff with h0, a, var_add and
the five parameter tensors requiring grad.  Parameters: gp_autograd_cases.make_inputs(M, D, Do, 1); then from
default_rng(7 + M + T), in this order: h0 = 0.5 N, a = 1.4 N, eps = N, var_add = 0.02 exp(U(-1, 1)), W = N (T, N, Do).
The loss of every case is  sum(W o traj) + 0.7 entropy.

Measured on the CPU (second_coding below: the K^-1 contraction with an explicit inverse instead of the two triangular
solves, the same loop): over all twelve cases the two codings agree on the trajectories to 6.1e-11 absolute (|traj| up to
10.7), on the entropy to 9e-14 relative, and on every gradient tensor to 3.3e-10 of its largest entry (the worst is
(300, 6, 4); every other case is within 1.7e-12).  No gradient tensor's largest entry is below 3.9e-2.  So the reference
sits three orders inside the rules below and no entry is masked.  A case costs at most a second.

Rules: gradients -- every entry within 1e-6 of the largest entry of its tensor (within_rule); trajectories -- within 1e-8
of max |traj|; entropy -- 1e-9 relative."""
import functools

import numpy as np
import torch

import gp_autograd_cases as gc
from gp_autograd_cases import PARAMS, within_rule   # noqa: F401  (re-exported)

ENT_WEIGHT = 0.7
LOG2PIE = float(np.log(2.0 * np.pi * np.e))

# (M, D, Do, N, T, reverse, var_add): the shapes of the feature's own tests; tests/gp_tile_grid.py holds the table that
# reaches every compiled (tile height, input width, trim) leaf of the rollout kernels
CASES = [
    (12, 4, 3, 21, 6, True, False),        # one row block, ragged columns
    (20, 19, 6, 37, 8, True, False),       # Voliro's recognition shape
    (30, 3, 3, 5, 7, False, True),         # Da = 0, N < 16
    (64, 16, 8, 16, 1, False, True),       # T = 1
    (100, 21, 14, 33, 6, False, True),     # the Sarcos tile
    (112, 24, 16, 17, 5, False, True),     # every limit at once
    (113, 9, 1, 17, 5, True, True),        # first stash height, Do = 1
    (130, 6, 4, 21, 6, True, True),
    (200, 13, 7, 21, 5, False, False),
    (250, 6, 2, 18, 4, True, True),
    (300, 6, 4, 18, 4, False, False),
    (30, 7, 5, 16, 40, False, True),       # forty steps of carry
]


def make_inputs(M, D, Do, N, T, reverse, with_var):
    """(parameter dict, h0, a, eps, var_add or None, W) as numpy arrays, drawn in the documented order"""
    p, _, _, _ = gc.make_inputs(M, D, Do, 1)
    rng = np.random.default_rng(7 + M + T)
    h0 = 0.5 * rng.standard_normal((N, Do))
    a = 1.4 * rng.standard_normal((T, N, D - Do))
    eps = rng.standard_normal((T, N))
    var_add = 0.02 * np.exp(rng.uniform(-1, 1, Do))
    W = rng.standard_normal((T, N, Do))
    return p, h0, a, eps, (var_add if with_var else None), W


def rollout(predict, h0, a, eps, var_add, reverse):
    """the recurrence over any predict(X) -> (fmean, fvar) of torch tensors; returns (traj (T, N, Do), entropy)"""
    T = eps.shape[0]
    h, ent = h0, 0.0
    rows = [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        fmean, fvar = predict(torch.cat([h, a[t]], 1))
        v = fvar if var_add is None else fvar + var_add
        h = h + fmean + eps[t][:, None] * torch.sqrt(v)
        rows[t] = h
        ent = ent + 0.5 * torch.sum(LOG2PIE + torch.log(v))
    return torch.stack(rows), ent


def second_coding(t):
    """predict(X) of the same GP through an explicit inverse of K_mm + jitter I (the form the kernels' dense path evaluates)"""
    from oracle import cbfssm_torch_ref as tref
    kern = tref.RBF(t['variance_unc'], t['lengthscales_unc'])
    Z, M = t['zeta_pos'], t['zeta_pos'].shape[0]
    Kinv = torch.linalg.inv(kern.K(Z) + tref.JITTER * torch.eye(M, dtype=torch.float64))
    zvar = tref.tf_forward(t['zeta_var_unc'])

    def predict(X):
        k = kern.K(Z, X)
        A2 = Kinv @ k
        fvar0 = torch.squeeze(kern.variance) - torch.sum(k * A2, 0)
        return A2.T @ t['zeta_mean'], fvar0[:, None] + (A2 * A2).T @ zvar
    return predict


def evaluate(case, coding='oracle'):
    """dict: traj, entropy, loss and the gradients 'g_' + name of the case's loss"""
    M, D, Do, N, T, reverse, with_var = case
    p, h0, a, eps, var_add, W = make_inputs(*case)
    t, gp = gc.oracle_model(p)
    lv = {'h0': torch.tensor(h0, requires_grad=True), 'a': torch.tensor(a, requires_grad=True)}
    if with_var:
        lv['var_add'] = torch.tensor(var_add, requires_grad=True)
    predict = gp.predict if coding == 'oracle' else second_coding(t)
    traj, ent = rollout(predict, lv['h0'], lv['a'], torch.tensor(eps), lv.get('var_add'), reverse)
    loss = (torch.tensor(W) * traj).sum() + ENT_WEIGHT * ent
    loss.backward()
    out = {'traj': traj.detach().numpy(), 'entropy': float(ent.detach()), 'loss': float(loss.detach())}
    for k, v in lv.items():
        out['g_' + k] = v.grad.numpy().copy()
    for k in PARAMS:
        out['g_' + k] = t[k].grad.numpy().copy()
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    """computed once per case and shared (treat as read-only)"""
    return evaluate(case)


def traj_rule(name, x, r, tol=1e-8):
    """every entry within tol of the largest |entry| of the reference trajectory; prints the ratio"""
    x, r = np.asarray(x, dtype=np.float64), np.asarray(r, dtype=np.float64)
    assert x.shape == r.shape, (name, x.shape, r.shape)
    scale = np.abs(r).max()
    err = np.abs(x - r).max() / scale
    print('%-34s max|ref| %.3e  err/max %.2e' % (name, scale, err))
    assert np.all(np.isfinite(x)) and err < tol, (name, err)
    return err


def entropy_rule(x, r, tol=1e-9):
    err = abs(float(x) - float(r)) / abs(float(r))
    print('%-34s ref %.6e  rel err %.2e' % ('entropy', float(r), err))
    assert np.isfinite(float(x)) and err < tol, ('entropy', err)
    return err
