"""GPModel.ekf against the per-step Python loop a caller wrote before it, and the launch alone against the kernels it is
built from.

    python profiles/tools/gp_ekf_time.py [rounds]

Per shape (M, D, Do, N, T, Dy), float64: HIP events around one call, the measurements alternating over `rounds` (default 5)
after two warm-up calls each; the median is reported.

    ekf             GPModel.ekf(m0, P0, a, y, var_x, var_y, cond)                one prepare, one pre-kernel, one launch
    loop            per step: GPModel.predict + GPModel.transition_jacobians (one prepare each), batched torch A P A^T and
                    the same Dy sequential scalar updates behind torch.where on the mask
    launch          cbfssm.hip.autograd.gp_ekf_eval on the pack prepared beforehand
    filter_launch   cbfssm.hip.autograd.gp_filter_eval at the same shape (the sampled-state loop: the GP work without
                    Jacobians or a covariance)
    lin_launches    T launches of gp_linearize_eval(variance=False) on N points (the GP work of the T steps, with the
                    Jacobians stored to memory, without the covariance recursion)

The loop's results are compared with ekf's.  Prints one JSON line per shape."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'cbf-ssm_amd')]

import numpy as np
import torch

from cbfssm.hip import autograd as ag
from cbfssm.model import gp_tf

SHAPES = [(100, 21, 14, 5120, 64, 7), (20, 19, 6, 320, 64, 3)]
DEV = 'cuda:0'


def softplus_inverse(y):
    y = np.asarray(y, dtype=np.float64) - 1e-10
    return y + np.log(-np.expm1(-y))


def make(M, D, Do, N, T, Dy):
    rng = np.random.default_rng(M)
    ls = rng.uniform(0.8, 1.25, D) * max(1.0, 0.75 * np.sqrt(D))
    zv = 0.05 * np.exp(rng.uniform(-1, 1, (M, Do)))
    p = [rng.uniform(-2, 2, (M, D)), 0.5 * rng.standard_normal((M, Do)), softplus_inverse(zv), softplus_inverse(np.array([0.4])),
         softplus_inverse(ls)]
    G = 0.2 * rng.standard_normal((N, Do, Do))
    return p, {'m0': 0.5 * rng.standard_normal((N, Do)), 'P0': G @ G.transpose(0, 2, 1),
               'a': 1.4 * rng.standard_normal((T, N, D - Do)), 'y': 0.7 * rng.standard_normal((T, N, Dy)),
               'var_x': 0.02 * np.exp(rng.uniform(-1, 1, Do)), 'var_y': 0.05 * np.exp(rng.uniform(-1, 1, Dy)),
               'cond': (rng.uniform(0, 1, (T, N)) >= 1.0 / 3.0).astype(np.float64), 'eps': rng.standard_normal((T, N)),
               'ytilde': 0.7 * rng.standard_normal((T, N, Do)), 'var_y_full': 0.05 * np.exp(rng.uniform(-1, 1, Do))}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def python_loop(gp, i, Do, Dy, T):
    """what a caller of predict + transition_jacobians writes: one prepare per GPModel call, batched tensor algebra"""
    m, P = i['m0'], i['P0']
    ll = torch.zeros(m.shape[0], dtype=torch.float64, device=m.device)
    means, covs = [], []
    for t in range(T):
        fmean, fvar = gp.predict(torch.cat([m, i['a'][t]], 1))
        A, _ = gp.transition_jacobians(m, i['a'][t])
        m = m + fmean
        P = A @ P @ A.transpose(1, 2) + torch.diag_embed(fvar + i['var_x'])
        on = i['cond'][t] != 0
        for j in range(Dy):
            s = P[:, j, j] + i['var_y'][j]
            dl = i['y'][t, :, j] - m[:, j]
            g = P[:, :, j] / s[:, None]
            m = torch.where(on[:, None], m + g * dl[:, None], m)
            P = torch.where(on[:, None, None], P - s[:, None, None] * g[:, :, None] * g[:, None, :], P)
            ll = torch.where(on, ll - 0.5 * (torch.log(2.0 * np.pi * s) + dl * dl / s), ll)
        means.append(m)
        covs.append(P)
    return torch.stack(means), torch.stack(covs), ll


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    for M, D, Do, N, T, Dy in SHAPES:
        p, raw = make(M, D, Do, N, T, Dy)
        t = lambda x: torch.tensor(x, dtype=torch.float64, device=DEV)
        gp = gp_tf.GPModel(D, Do, M, 0.4, 1.0, 0.1, 1.0, 0.01, seed=0, device=DEV)
        gp.zeta_pos, gp.zeta_mean, gp.zeta_var_unc, gp.kern.variance_unc, gp.kern.lengthscales_unc = [t(x) for x in p]
        i = {k: t(v) for k, v in raw.items()}
        X = torch.cat([i['m0'], i['a'][0]], 1).contiguous()
        keep = {}
        pack = gp._prepared()
        args = (i['m0'], i['P0'], i['a'], i['y'], i['var_x'], i['var_y'])

        def ekf():
            keep['ekf'] = gp.ekf(*args, cond=i['cond'])

        def loop():
            keep['loop'] = python_loop(gp, i, Do, Dy, T)

        def lin_launches():
            for _ in range(T):
                ag.gp_linearize_eval(pack, X, variance=False)

        fns = {'ekf': ekf, 'loop': loop, 'launch': lambda: ag.gp_ekf_eval(pack, *args, cond=i['cond']),
               'filter_launch': lambda: ag.gp_filter_eval(pack, i['m0'], i['a'], i['ytilde'], i['eps'], i['var_x'],
                                                          i['var_y_full'], cond=i['cond']),
               'lin_launches': lin_launches}
        for _ in range(2):
            for f in fns.values():
                f()
        torch.cuda.synchronize()
        err = [float(((x - z).abs().max() / z.abs().max()).cpu()) for x, z in zip(keep['ekf'], keep['loop'])]
        res = {k: [] for k in fns}
        for _ in range(rounds):
            for k, f in fns.items():
                res[k].append(timed(f))
        med = {k: float(np.median(v)) for k, v in res.items()}
        print(json.dumps({'shape': [M, D, Do, N, T, Dy], 'rounds': rounds, 'form': gp._pack.gp_form(), 'ms_median': med,
                          'ms_min': {k: float(np.min(v)) for k, v in res.items()},
                          'ms_max': {k: float(np.max(v)) for k, v in res.items()},
                          'loop_over_ekf': med['loop'] / med['ekf'],
                          'launch_over_filter_launch': med['launch'] / med['filter_launch'],
                          'launch_over_lin_launches': med['launch'] / med['lin_launches'],
                          'max_rel_diff_means_covs_loglik_vs_loop': err}), flush=True)


if __name__ == '__main__':
    main()
