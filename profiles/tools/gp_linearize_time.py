"""GPModel.linearize against the way the same Jacobians were obtained before it: backward calls through GPModel.predict
under grad with one-hot cotangents, one per output dimension for the mean and one more per dimension for the variance.

    python profiles/tools/gp_linearize_time.py [rounds]

Per shape (M, D, Do, npts), float64: HIP events around one call, the four measurements alternating over `rounds` (default 5)
after two warm-up calls each; the median is reported.

    linearize            GPModel.linearize(X)                      fmean, fvar, dmean, dvar
    linearize_mean       GPModel.linearize(X, variance=False)      fmean, fvar, dmean
    yardstick            predict(X) under grad (X alone requires grad), then 2 Do backward calls
    yardstick_mean       the same with the Do backward calls of the mean
    launch, launch_mean  cbfssm.hip.autograd.gp_linearize_eval on the pack prepared beforehand: the pre-kernel and the launch alone,
                         without the prepare kernel (K_mm, Cholesky, K^-1) that every GPModel call above runs first

The yardstick is code this tool does not touch (gp_predict_bwd_kernel behind cbfssm.hip.autograd.gp_predict).  Its results
are stacked into the same (npts, Do, D) tensors and compared with linearize's.  Prints one JSON line per shape."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'cbf-ssm_amd')]

import numpy as np
import torch

from cbfssm.hip import autograd as ag
from cbfssm.model import gp_tf

SHAPES = [(100, 21, 14, 65536), (200, 13, 7, 65536)]
DEV = 'cuda:0'


def softplus_inverse(y):
    y = np.asarray(y, dtype=np.float64) - 1e-10
    return y + np.log(-np.expm1(-y))


def make(M, D, Do, npts):
    rng = np.random.default_rng(M)
    ls = rng.uniform(0.8, 1.25, D) * max(1.0, 0.75 * np.sqrt(D))
    zv = 0.05 * np.exp(rng.uniform(-1, 1, (M, Do)))
    p = [rng.uniform(-2, 2, (M, D)), 0.5 * rng.standard_normal((M, Do)), softplus_inverse(zv), softplus_inverse(np.array([0.4])),
         softplus_inverse(ls)]
    return p, 1.4 * rng.standard_normal((npts, D))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    for M, D, Do, npts in SHAPES:
        p, X = make(M, D, Do, npts)
        t = lambda x: torch.tensor(x, dtype=torch.float64, device=DEV)
        gp = gp_tf.GPModel(D, Do, M, 0.4, 1.0, 0.1, 1.0, 0.01, seed=0, device=DEV)
        gp.zeta_pos, gp.zeta_mean, gp.zeta_var_unc, gp.kern.variance_unc, gp.kern.lengthscales_unc = [t(x) for x in p]
        Xd = t(X)
        Xg = t(X).requires_grad_()
        onehot = [torch.zeros(npts, Do, dtype=torch.float64, device=DEV) for _ in range(Do)]
        for d in range(Do):
            onehot[d][:, d] = 1.0
        zero = torch.zeros(npts, Do, dtype=torch.float64, device=DEV)
        keep = {}

        def linearize():
            keep['lin'] = gp.linearize(Xd)

        def linearize_mean():
            keep['lin_mean'] = gp.linearize(Xd, variance=False)

        def yardstick(variance=True):
            fmean, fvar = gp.predict(Xg)
            dm = [torch.autograd.grad((fmean, fvar), Xg, (onehot[d], zero), retain_graph=True)[0] for d in range(Do)]
            dv = [torch.autograd.grad((fmean, fvar), Xg, (zero, onehot[d]), retain_graph=True)[0] for d in range(Do)] if variance else None
            keep['yard'] = (torch.stack(dm, 1), torch.stack(dv, 1) if variance else None)

        pack = gp._prepared()
        fns = {'linearize': linearize, 'linearize_mean': linearize_mean, 'yardstick': yardstick,
               'yardstick_mean': lambda: yardstick(False), 'launch': lambda: ag.gp_linearize_eval(pack, Xd),
               'launch_mean': lambda: ag.gp_linearize_eval(pack, Xd, variance=False)}
        for _ in range(2):
            for f in fns.values():
                f()
        torch.cuda.synchronize()
        linearize(); yardstick()
        err = [float(((a - b).abs().max() / b.abs().max()).cpu()) for a, b in zip(keep['lin'][2:], keep['yard'])]
        res = {k: [] for k in fns}
        for _ in range(rounds):
            for k, f in fns.items():
                res[k].append(timed(f))
        med = {k: float(np.median(v)) for k, v in res.items()}
        print(json.dumps({'shape': [M, D, Do, npts], 'rounds': rounds, 'form': gp._pack.gp_form(), 'ms_median': med,
                          'ms_min': {k: float(np.min(v)) for k, v in res.items()},
                          'ms_max': {k: float(np.max(v)) for k, v in res.items()},
                          'yardstick_over_linearize': med['yardstick'] / med['linearize'],
                          'yardstick_mean_over_linearize_mean': med['yardstick_mean'] / med['linearize_mean'],
                          'max_rel_diff_dmean_dvar_vs_yardstick': err}), flush=True)


if __name__ == '__main__':
    main()
