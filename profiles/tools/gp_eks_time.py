"""GPModel.eks against GPModel.ekf alone and against what a caller wrote before it.

    python profiles/tools/gp_eks_time.py [rounds]

Per shape (M, D, Do, N, T, Dy), float64: HIP events around one call, the measurements alternating over `rounds` (default 5)
after two warm-up calls each; the median is reported.

    eks             GPModel.eks(m0, P0, a, y, var_x, var_y, cond)                  prepare, pre-kernel, filter kernel, sweep
    eks_lag         the same with lag_one=True
    ekf             GPModel.ekf on the same inputs                                 prepare, pre-kernel, filter kernel
    eks_launch, eks_lag_launch, ekf_launch   the same three through cbfssm.hip.autograd on the pack prepared beforehand
    loop            GPModel.ekf, then per step GPModel.transition_jacobians (one prepare each) at the filtered means, the
                    predicted covariance by batched matrix products, and a Python loop over T of torch.linalg.solve for
                    the gain with the smoothed moments and the lag-one covariances by batched products

The loop's results are compared with eks's.  Prints one JSON line per shape."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'cbf-ssm_amd'), os.path.dirname(os.path.abspath(__file__))]

import numpy as np
import torch

from cbfssm.hip import autograd as ag
from cbfssm.model import gp_tf
from gp_ekf_time import SHAPES, DEV, make, timed


def python_smoother(gp, i, T):
    """what a caller of ekf + transition_jacobians writes"""
    means, covs, _ = gp.ekf(i['m0'], i['P0'], i['a'], i['y'], i['var_x'], i['var_y'], cond=i['cond'])
    ms, Ps = means[T - 1], covs[T - 1]
    sm, sP, lag = [ms], [Ps], []
    for t in range(T - 1, -1, -1):
        mf, Pf = (means[t - 1], covs[t - 1]) if t > 0 else (i['m0'], i['P0'])
        x = torch.cat([mf, i['a'][t]], 1)
        fmean, fvar = gp.predict(x)
        A, _ = gp.transition_jacobians(mf, i['a'][t])
        cross = A @ Pf
        Pm = cross @ A.transpose(1, 2) + torch.diag_embed(fvar + i['var_x'])
        G = torch.linalg.solve(Pm, cross).transpose(1, 2)
        lag.append(G @ Ps)
        ms = mf + (G @ (ms - (mf + fmean))[:, :, None])[:, :, 0]
        Ps = Pf + G @ (Ps - Pm) @ G.transpose(1, 2)
        sm.append(ms)
        sP.append(Ps)
    sm.reverse(), sP.reverse(), lag.reverse()
    return torch.stack(sm[1:]), torch.stack(sP[1:]), sm[0], sP[0], torch.stack(lag)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    for M, D, Do, N, T, Dy in SHAPES:
        p, raw = make(M, D, Do, N, T, Dy)
        t = lambda x: torch.tensor(x, dtype=torch.float64, device=DEV)
        gp = gp_tf.GPModel(D, Do, M, 0.4, 1.0, 0.1, 1.0, 0.01, seed=0, device=DEV)
        gp.zeta_pos, gp.zeta_mean, gp.zeta_var_unc, gp.kern.variance_unc, gp.kern.lengthscales_unc = [t(x) for x in p]
        i = {k: t(v) for k, v in raw.items()}
        keep = {}
        pack = gp._prepared()
        args = (i['m0'], i['P0'], i['a'], i['y'], i['var_x'], i['var_y'])

        def eks_lag():
            keep['eks'] = gp.eks(*args, cond=i['cond'], lag_one=True)

        def loop():
            keep['loop'] = python_smoother(gp, i, T)

        fns = {'eks': lambda: gp.eks(*args, cond=i['cond']), 'eks_lag': eks_lag, 'ekf': lambda: gp.ekf(*args, cond=i['cond']),
               'eks_launch': lambda: ag.gp_eks_eval(pack, *args, cond=i['cond']),
               'eks_lag_launch': lambda: ag.gp_eks_eval(pack, *args, cond=i['cond'], lag_one=True),
               'ekf_launch': lambda: ag.gp_ekf_eval(pack, *args, cond=i['cond']), 'loop': loop}
        for _ in range(2):
            for f in fns.values():
                f()
        torch.cuda.synchronize()
        r = keep['eks']
        assert int(r.info.abs().sum()) == 0
        err = [float(((x - z).abs().max() / z.abs().max()).cpu())
               for x, z in zip((r.smeans, r.scovs, r.init_mean, r.init_cov, r.lag_one), keep['loop'])]
        res = {k: [] for k in fns}
        for _ in range(rounds):
            for k, f in fns.items():
                res[k].append(timed(f))
        med = {k: float(np.median(v)) for k, v in res.items()}
        print(json.dumps({'shape': [M, D, Do, N, T, Dy], 'rounds': rounds, 'form': gp._pack.gp_form(), 'ms_median': med,
                          'ms_min': {k: float(np.min(v)) for k, v in res.items()},
                          'ms_max': {k: float(np.max(v)) for k, v in res.items()},
                          'loop_over_eks_lag': med['loop'] / med['eks_lag'],
                          'eks_launch_minus_ekf_launch': med['eks_launch'] - med['ekf_launch'],
                          'eks_lag_launch_minus_ekf_launch': med['eks_lag_launch'] - med['ekf_launch'],
                          'max_rel_diff_smeans_scovs_initmean_initcov_lagone_vs_loop': err}), flush=True)


if __name__ == '__main__':
    main()
