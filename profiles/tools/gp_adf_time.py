"""GPModel.adf against the per-step Python loop a caller wrote before it, against the kernels it is built from, and
against GPModel.ekf (what exactness costs over the first-order filter); GPModel.ads against adf alone.

    python profiles/tools/gp_adf_time.py [rounds]

Per shape (M, D, Do, N, T, Dy), float64, the shapes of the ekf record: HIP events around one call, the measurements
alternating over `rounds` (default 5) after two warm-up calls each; the median is reported.

    adf             GPModel.adf(m0, P0, a, y, var_x, var_y, cond)            one prepare, two pre-kernels, one launch
    adf_launch      cbfssm.hip.autograd.gp_adf_eval on the pack prepared beforehand
    loop            per step: GPModel.transition_moments (one prepare, two pre-kernels, one launch, about ten tensor-library
                    ops) and the Dy sequential scalar updates behind torch.where on the mask
    mm_launches     T launches of gp_moment_match_eval on N beliefs (the GP work of the T steps, alpha and W_d formed T
                    times, without the recursion)
    ekf             GPModel.ekf at the same shape
    ads             GPModel.ads(..., lag_one=False)

The loop's results are compared with adf's (1e-9 of the largest entry) before anything is timed.  The condition of the
record: adf's median below the smallest of the loop's values.  Prints one JSON line per shape."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'cbf-ssm_amd'), os.path.dirname(os.path.abspath(__file__))]

import numpy as np
import torch

from cbfssm.hip import autograd as ag
from cbfssm.model import gp_tf
from gp_ekf_time import DEV, SHAPES, make, timed


def python_loop(gp, i, Do, Dy, T):
    """what a caller of transition_moments writes: one prepare per step, batched tensor algebra for the update"""
    m, P = i['m0'], i['P0']
    N = m.shape[0]
    ll = torch.zeros(N, dtype=torch.float64, device=m.device)
    vx = torch.diag_embed(i['var_x'].expand(N, Do))
    means, covs = [], []
    for t in range(T):
        m, P, _, _ = gp.transition_moments(m, P, i['a'][t])
        P = P + vx
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
        mean = torch.cat([i['m0'], i['a'][0]], 1).contiguous()
        cov = torch.zeros(N, D, D, dtype=torch.float64, device=DEV)
        cov[:, :Do, :Do] = i['P0']
        keep = {}
        pack = gp._prepared()
        args = (i['m0'], i['P0'], i['a'], i['y'], i['var_x'], i['var_y'])

        def adf():
            keep['adf'] = gp.adf(*args, cond=i['cond'])

        def loop():
            keep['loop'] = python_loop(gp, i, Do, Dy, T)

        def mm_launches():
            for _ in range(T):
                ag.gp_moment_match_eval(pack, mean, cov)

        fns = {'adf': adf, 'adf_launch': lambda: ag.gp_adf_eval(pack, *args, cond=i['cond']), 'loop': loop,
               'mm_launches': mm_launches, 'ekf': lambda: gp.ekf(*args, cond=i['cond']),
               'ads': lambda: gp.ads(*args, cond=i['cond'])}
        for _ in range(2):
            for f in fns.values():
                f()
        torch.cuda.synchronize()
        assert int(keep['adf'].info.abs().sum()) == 0
        err = [float(((x - z).abs().max() / z.abs().max()).cpu()) for x, z in zip(keep['adf'][:3], keep['loop'])]
        assert max(err) <= 1e-9, err
        res = {k: [] for k in fns}
        for _ in range(rounds):
            for k, f in fns.items():
                res[k].append(timed(f))
        med = {k: float(np.median(v)) for k, v in res.items()}
        print(json.dumps({'shape': [M, D, Do, N, T, Dy], 'rounds': rounds, 'form': gp._pack.gp_form(), 'ms_median': med,
                          'ms_min': {k: float(np.min(v)) for k, v in res.items()},
                          'ms_max': {k: float(np.max(v)) for k, v in res.items()},
                          'loop_over_adf': med['loop'] / med['adf'], 'adf_below_every_loop_value': med['adf'] < min(res['loop']),
                          'adf_launch_over_mm_launches': med['adf_launch'] / med['mm_launches'],
                          'adf_over_ekf': med['adf'] / med['ekf'], 'ads_over_adf': med['ads'] / med['adf'],
                          'max_rel_diff_means_covs_loglik_vs_loop': err}), flush=True)


if __name__ == '__main__':
    main()
