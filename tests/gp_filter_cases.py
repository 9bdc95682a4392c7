"""Shared by the GP-filter tests: the cases, their inputs, and the reference -- the recurrence

    for t in 0..T-1 (reverse: T-1..0):
        fmean, fvar = gp.predict(concat(h, a[t]));  m = h + fmean;  v = fvar + var_x                      cbfssm.py:199-206
        where cond[t, n]:  r = var_y + (k_factor - 1) v;  s = r + v;  k = v / s;  delta = ytilde[t] - m    :212-217
                           mu = m + k delta;  sig = (1 - k)^2 v + k^2 r;  h = mu + eps[t][:, None] sqrt(sig)
                           kl += 0.5 (log v - log sig + (sig + (mu - m)^2) / v - 1)                        :232-234
        elsewhere:         h = m + eps[t][:, None] sqrt(v)                                                 :224
        traj[t] = h

written over oracle/cbfssm_torch_ref.GPModel on the CPU, differentiated by reverse-mode autodiff with h0, a, ytilde,
var_x, var_y and the five parameter tensors requiring grad.  Parameters: gp_autograd_cases.make_inputs(M, D, Do, 1); then
from default_rng(11 + M + T), in this order: h0 = 0.5 N, a = 1.4 N, eps = N, var_x = 0.02 exp(U(-1, 1)),
var_y = 0.05 exp(U(-1, 1)), ytilde = 0.7 N (T, N, Do), W = N (T, N, Do), U = U(0, 1) (T, N) for the random mask.
The loss of every case is  sum(W o traj) + 0.7 kl.

Masks: 'ones' (handed to the library as NULL / None), 'zeros', 'prefix' (the first K = ceil(T / 2) steps IN THE ORDER THE
LOOP RUNS condition: warm-up then forecast; under reverse these are the last K time indices) and 'random' (cond = U >= 1/3,
about a third zeros, per step and chain).  In the random-mask cases ytilde holds NaN at every masked-out entry; the
reference selects around them (torch.where on the inputs of the update, so that no NaN enters the tape).

Measured on the CPU (second_coding of gp_rollout_cases: the K^-1 contraction with an explicit inverse instead of the two
triangular solves, the same loop): over all twelve cases the two codings agree on the trajectories to 3.8e-12 of
max |traj|, on kl to 3.7e-13 relative, and on every gradient tensor to 9.1e-11 of its largest entry.  No gradient tensor's
largest entry is below 1.4e-1 (tensors that are exactly zero by construction -- d/d ytilde and d/d var_y under the
all-zero mask -- are checked as zeros, not by the rule).  The smallest kl of a case with a conditioned step is 7.6e1.  So
the reference sits three to four orders inside the rules below and no entry is masked.  A case costs at most a second.

Rules (those of gp_rollout_cases): gradients -- every entry within 1e-6 of the largest entry of its tensor (within_rule);
trajectories -- within 1e-8 of max |traj|; kl -- 1e-9 relative."""
import functools

import numpy as np
import torch

import gp_autograd_cases as gc
from gp_autograd_cases import PARAMS, within_rule   # noqa: F401  (re-exported)
from gp_rollout_cases import second_coding, traj_rule   # noqa: F401  (re-exported)

KL_WEIGHT = 0.7

# (M, D, Do, N, T, reverse, var_x, k_factor, mask): every tile height once (1, 2, 4, 7, 10, 13, 16, 20 row blocks), the three
# input widths (DK 2: D <= 8, DK 4: D <= 16, DK 6: D <= 24), and the four masks
CASES = [
    (12, 4, 3, 21, 6, True, False, 1.0, 'ones'),         # one row block, ragged columns, var_x = NULL
    (20, 19, 6, 37, 8, True, False, 1.5, 'random'),      # two row blocks, DK 6
    (30, 3, 3, 5, 7, False, True, 1.0, 'prefix'),        # Da = 0, N < 16
    (64, 16, 8, 16, 1, False, True, 1.0, 'ones'),        # T = 1, four row blocks, DK 4
    (100, 21, 14, 33, 6, False, True, 2.0, 'random'),    # the Sarcos tile (seven row blocks, trimmed)
    (112, 24, 16, 17, 5, False, True, 1.0, 'prefix'),    # every limit at once
    (113, 9, 1, 17, 5, True, True, 1.0, 'random'),       # first stash height (ten row blocks), Do = 1
    (200, 13, 7, 21, 5, False, False, 1.3, 'ones'),      # thirteen row blocks
    (250, 6, 2, 18, 4, True, True, 1.0, 'zeros'),        # sixteen row blocks, nothing conditioned
    (300, 6, 4, 18, 4, False, False, 1.2, 'prefix'),     # twenty row blocks
    (30, 7, 5, 16, 40, False, True, 1.0, 'random'),      # forty steps of carry
    (20, 6, 4, 19, 5, True, True, 1.0, 'prefix'),        # a prefix under reverse
]

GRADS = ('h0', 'a', 'ytilde', 'var_x', 'var_y')


def make_mask(kind, T, N, reverse, U):
    """(T, N) array of 0. / 1.; None for 'ones' (the library's NULL)"""
    if kind == 'ones':
        return None
    if kind == 'zeros':
        return np.zeros((T, N))
    if kind == 'prefix':
        K = (T + 1) // 2
        c = np.zeros((T, N))
        if reverse:
            c[T - K:] = 1.0
        else:
            c[:K] = 1.0
        return c
    assert kind == 'random'
    return (U >= 1.0 / 3.0).astype(np.float64)


def make_inputs(M, D, Do, N, T, reverse, with_vx, k_factor, mask):
    """(parameter dict, h0, a, ytilde, cond or None, eps, var_x or None, var_y, W) as numpy arrays, drawn in the documented
    order; ytilde holds NaN where a random mask is 0"""
    p, _, _, _ = gc.make_inputs(M, D, Do, 1)
    rng = np.random.default_rng(11 + M + T)
    h0 = 0.5 * rng.standard_normal((N, Do))
    a = 1.4 * rng.standard_normal((T, N, D - Do))
    eps = rng.standard_normal((T, N))
    var_x = 0.02 * np.exp(rng.uniform(-1, 1, Do))
    var_y = 0.05 * np.exp(rng.uniform(-1, 1, Do))
    ytilde = 0.7 * rng.standard_normal((T, N, Do))
    W = rng.standard_normal((T, N, Do))
    U = rng.uniform(0, 1, (T, N))
    cond = make_mask(mask, T, N, reverse, U)
    if mask == 'random':
        ytilde[cond == 0.0] = np.nan
    return p, h0, a, ytilde, cond, eps, (var_x if with_vx else None), var_y, W


def filter_loop(predict, h0, a, ytilde, cond, eps, var_x, var_y, k_factor, reverse):
    """the recurrence over any predict(X) -> (fmean, fvar) of torch tensors; cond: (T, N) tensor or None; returns
    (traj (T, N, Do), kl).  ytilde may hold NaN where cond is 0."""
    T = eps.shape[0]
    h, kl = h0, torch.zeros((), dtype=torch.float64, device=h0.device)
    rows = [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        fmean, fvar = predict(torch.cat([h, a[t]], 1))
        m = h + fmean
        v = fvar if var_x is None else fvar + var_x
        e = eps[t][:, None]
        free = m + e * torch.sqrt(v)
        if cond is not None and not bool((cond[t] != 0).any()):
            h = free
        else:
            on = torch.ones_like(m, dtype=torch.bool) if cond is None else (cond[t] != 0)[:, None].expand_as(m)
            yt = torch.where(on, ytilde[t], torch.zeros_like(m))
            r = var_y + (k_factor - 1.0) * v
            s = r + v
            k = v / s
            delta = yt - m
            mu = m + k * delta
            sig = (1.0 - k) ** 2 * v + k ** 2 * r
            h = torch.where(on, mu + e * torch.sqrt(sig), free)
            term = 0.5 * (torch.log(v) - torch.log(sig) + (sig + (mu - m) ** 2) / v - 1.0)
            kl = kl + torch.where(on, term, torch.zeros_like(term)).sum()
        rows[t] = h
    return torch.stack(rows), kl


def evaluate(case, coding='oracle'):
    """dict: traj, kl, loss and the gradients 'g_' + name of the case's loss"""
    M, D, Do, N, T, reverse, with_vx, k_factor, mask = case
    p, h0, a, ytilde, cond, eps, var_x, var_y, W = make_inputs(*case)
    t, gp = gc.oracle_model(p)
    lv = {'h0': torch.tensor(h0, requires_grad=True), 'a': torch.tensor(a, requires_grad=True),
          'ytilde': torch.tensor(ytilde, requires_grad=True), 'var_y': torch.tensor(var_y, requires_grad=True)}
    if with_vx:
        lv['var_x'] = torch.tensor(var_x, requires_grad=True)
    predict = gp.predict if coding == 'oracle' else second_coding(t)
    traj, kl = filter_loop(predict, lv['h0'], lv['a'], lv['ytilde'], None if cond is None else torch.tensor(cond),
                           torch.tensor(eps), lv.get('var_x'), lv['var_y'], k_factor, reverse)
    loss = (torch.tensor(W) * traj).sum() + KL_WEIGHT * kl
    loss.backward()
    out = {'traj': traj.detach().numpy(), 'kl': float(kl.detach()), 'loss': float(loss.detach())}
    for k, v in lv.items():
        out['g_' + k] = (v.grad if v.grad is not None else torch.zeros_like(v)).numpy().copy()
    for k in PARAMS:
        out['g_' + k] = t[k].grad.numpy().copy()
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    """computed once per case and shared (treat as read-only)"""
    return evaluate(case)


def grad_names(case):
    """(the tensors the gradient rule applies to, the tensors that are exactly zero by construction)"""
    with_vx, mask = case[6], case[8]
    names = ('h0', 'a') + (('var_x',) if with_vx else ()) + PARAMS
    if mask == 'zeros':
        return names, ('ytilde', 'var_y')
    return names + ('ytilde', 'var_y'), ()


def kl_rule(x, r, tol=1e-9):
    """1e-9 relative; a reference of exactly 0 (nothing conditioned) must be met exactly"""
    if float(r) == 0.0:
        print('%-34s ref 0  got %r' % ('kl', float(x)))
        assert float(x) == 0.0, ('kl', float(x))
        return 0.0
    err = abs(float(x) - float(r)) / abs(float(r))
    print('%-34s ref %.6e  rel err %.2e' % ('kl', float(r), err))
    assert np.isfinite(float(x)) and err < tol, ('kl', err)
    return err
