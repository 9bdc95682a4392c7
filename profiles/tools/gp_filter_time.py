"""The fused GP filter loop against what the surface offered before it: a Python loop of one `gp_predict` per step plus
tensor-library elementwise ops (the masked Gaussian update and the KL term), under torch autograd, on the same GPU; and
against the fused `gp_rollout` at the same shapes, whose kernels differ from the filter's in the step epilogue only.

    python profiles/tools/gp_filter_time.py [rounds] [reps]

Per shape (M, D, Do, N, T): forward under grad plus the full backward into h0, a, ytilde, var_x, var_y and the five
parameter tensors (the rollout: h0, a, var_add and the five), HIP events around `reps` calls (one call of the loop), the
three sides alternating over `rounds` after two warm-up calls each.  The mask is random per (step, chain) with about a
third zeros and ytilde is NaN where it is zero.  Prints one JSON line per shape."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'cbf-ssm_amd')]

import numpy as np
import torch

from cbfssm.hip import autograd
from cbfssm.model import gp_tf

SHAPES = [(100, 21, 14, 5120, 64), (20, 19, 6, 320, 64)]
DEV = 'cuda:0'
K_FACTOR = 1.5


def softplus_inverse(y):
    y = np.asarray(y, dtype=np.float64) - 1e-10
    return y + np.log(-np.expm1(-y))


def make(M, D, Do, N, T):
    rng = np.random.default_rng(M)
    ls = rng.uniform(0.8, 1.25, D) * max(1.0, 0.75 * np.sqrt(D))
    p = [rng.uniform(-2, 2, (M, D)), 0.1 * rng.standard_normal((M, Do)),
         softplus_inverse(0.05 * np.exp(rng.uniform(-1, 1, (M, Do)))), softplus_inverse(np.array([0.4])), softplus_inverse(ls)]
    cond = (rng.uniform(0, 1, (T, N)) >= 1.0 / 3.0).astype(np.float64)
    ytilde = 0.7 * rng.standard_normal((T, N, Do))
    ytilde[cond == 0.0] = np.nan
    return (p, 0.5 * rng.standard_normal((N, Do)), 1.4 * rng.standard_normal((T, N, D - Do)), ytilde, cond,
            rng.standard_normal((T, N)), 0.02 * np.exp(rng.uniform(-1, 1, Do)), 0.05 * np.exp(rng.uniform(-1, 1, Do)),
            rng.standard_normal((T, N, Do)))


def loop_filter(gp, h0, a, ytilde, cond, eps, var_x, var_y):
    """the per-step loop: T launches of the predict kernel, T prepares, T adjoint launches, elementwise ops in between"""
    h, kl, rows = h0, 0.0, []
    for t in range(eps.shape[0]):
        fmean, fvar = autograd.gp_predict(gp._pack, torch.cat([h, a[t]], 1), *gp.parameters())
        m, v, e = h + fmean, fvar + var_x, eps[t][:, None]
        on = (cond[t] != 0)[:, None].expand_as(m)
        r = var_y + (K_FACTOR - 1.0) * v
        k = v / (r + v)
        mu = m + k * (torch.where(on, ytilde[t], torch.zeros_like(m)) - m)
        sig = (1.0 - k) ** 2 * v + k ** 2 * r
        h = torch.where(on, mu + e * torch.sqrt(sig), m + e * torch.sqrt(v))
        term = 0.5 * (torch.log(v) - torch.log(sig) + (sig + (mu - m) ** 2) / v - 1.0)
        kl = kl + torch.where(on, term, torch.zeros_like(term)).sum()
        rows.append(h)
    return torch.stack(rows), kl


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    for M, D, Do, N, T in SHAPES:
        p, h0, a, ytilde, cond, eps, var_x, var_y, W = make(M, D, Do, N, T)
        t = lambda x: torch.tensor(x, dtype=torch.float64, device=DEV)
        gp = gp_tf.GPModel(D, Do, M, 0.4, 1.0, 0.1, 1.0, 0.01, seed=0, device=DEV)
        gp.zeta_pos, gp.zeta_mean, gp.zeta_var_unc, gp.kern.variance_unc, gp.kern.lengthscales_unc = [t(x) for x in p]
        leaves = gp.parameters()
        for q in leaves:
            q.requires_grad_()
        h0d, ad, ytd = t(h0).requires_grad_(), t(a).requires_grad_(), t(ytilde).requires_grad_()
        vxd, vyd = t(var_x).requires_grad_(), t(var_y).requires_grad_()
        cd, epsd, Wd = t(cond), t(eps), t(W)
        wrt = [h0d, ad, ytd, vxd, vyd] + leaves
        wrt_r = [h0d, ad, vxd] + leaves
        keep = {}

        def fused():
            traj, kl = gp.filter(h0d, ad, ytd, epsd, vxd, vyd, cond=cd, k_factor=K_FACTOR)
            keep['f'] = torch.autograd.grad((Wd * traj).sum() + 0.7 * kl, wrt)

        def loop():
            traj, kl = loop_filter(gp, h0d, ad, ytd, cd, epsd, vxd, vyd)
            keep['l'] = torch.autograd.grad((Wd * traj).sum() + 0.7 * kl, wrt)

        def rollout():
            traj, ent = gp.rollout(h0d, ad, epsd, vxd)
            keep['r'] = torch.autograd.grad((Wd * traj).sum() + 0.7 * ent, wrt_r)
        for _ in range(2):
            fused(); loop(); rollout()
        torch.cuda.synchronize()
        err = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(keep['f'], keep['l']))
        res = {'fused': [], 'loop': [], 'rollout': []}
        for _ in range(rounds):
            res['fused'].append(timed(fused, reps))
            res['loop'].append(timed(loop, 1))
            res['rollout'].append(timed(rollout, reps))
        med = {k: float(np.median(v)) for k, v in res.items()}
        out = {'shape': [M, D, Do, N, T], 'rounds': rounds, 'reps': reps, 'ms_median': med,
               'ms_min': {k: float(np.min(v)) for k, v in res.items()}, 'ms_max': {k: float(np.max(v)) for k, v in res.items()},
               'loop_over_fused': med['loop'] / med['fused'], 'fused_over_rollout': med['fused'] / med['rollout'],
               'workgroups': (N + 15) // 16, 'grad_max_rel_diff_fused_vs_loop': err}
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
