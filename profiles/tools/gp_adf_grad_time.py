"""GPModel.adf(..., input_grads=True), forward under grad plus backward, against the per-step loop a caller wrote before it:
transition_moments(..., input_grads=True) per step plus the scalar updates in the tensor library, differentiated by the tape.

    python profiles/tools/gp_adf_grad_time.py [rounds]

Per shape (M, D, Do, N, T, Dy), float64, the shapes of the adf record: HIP events around one call, the measurements
alternating over `rounds` (default 5) after two warm-up calls each; the median is reported with min and max.  The loss is
sum Wm o means + sum Wc o covs + sum Wl o loglik with fixed random weights; the gradients go to m0, P0, a, y, var_x, var_y.

    fused           forward under grad and backward through GPModel.adf(..., input_grads=True)
    bwd_launch      cbfssm_gp_adf_bwd_f64 alone on the prepared pack and the forward's records (two pre-kernels, the
                    reverse-time launch, the fold of the variance sums), `work` allocated beforehand
    fwd_launch      cbfssm.hip.autograd.gp_adf_eval on the prepared pack
    loop            forward and backward of the per-step loop; it uses nothing this record's change adds

The gradients of the two paths are compared (1e-6 of the largest entry) before anything is timed.  The condition of the
record: the fused median below the smallest of the loop's values.  Prints one JSON line per shape."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'cbf-ssm_amd'), os.path.dirname(os.path.abspath(__file__))]

import numpy as np
import torch

from cbfssm.hip import autograd as ag
from cbfssm.hip import lib as hl
from cbfssm.hip.ops import _ptr, _stream
from cbfssm.model import gp_tf
from gp_ekf_time import DEV, SHAPES, make, timed

NAMES = ('m0', 'P0', 'a', 'y', 'var_x', 'var_y')


def python_loop(gp, lv, cond, Do, Dy, T):
    """what a caller of transition_moments(..., input_grads=True) writes: one adjoint launch per step on the way back"""
    m, P = lv['m0'], lv['P0']
    N = m.shape[0]
    ll = torch.zeros(N, dtype=torch.float64, device=m.device)
    vx = torch.diag_embed(lv['var_x'].expand(N, Do))
    means, covs = [], []
    for t in range(T):
        m, P, _, _ = gp.transition_moments(m, P, lv['a'][t], input_grads=True)
        P = P + vx
        on = cond[t] != 0
        for j in range(Dy):
            s = P[:, j, j] + lv['var_y'][j]
            dl = lv['y'][t, :, j] - m[:, j]
            g = P[:, :, j] / s[:, None]
            m = torch.where(on[:, None], m + g * dl[:, None], m)
            P = torch.where(on[:, None, None], P - s[:, None, None] * g[:, :, None] * g[:, None, :], P)
            ll = torch.where(on, ll - 0.5 * (torch.log(2.0 * np.pi * s) + dl * dl / s), ll)
        means.append(m)
        covs.append(P)
    return torch.stack(means), torch.stack(covs), ll


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    lib = hl.load()
    for M, D, Do, N, T, Dy in SHAPES:
        p, raw = make(M, D, Do, N, T, Dy)
        t = lambda x: torch.tensor(x, dtype=torch.float64, device=DEV)
        gp = gp_tf.GPModel(D, Do, M, 0.4, 1.0, 0.1, 1.0, 0.01, seed=0, device=DEV)
        gp.zeta_pos, gp.zeta_mean, gp.zeta_var_unc, gp.kern.variance_unc, gp.kern.lengthscales_unc = [t(x) for x in p]
        i = {k: t(raw[k]) for k in NAMES + ('cond',)}
        gen = torch.Generator(device='cpu').manual_seed(3)
        Wm, Wc, Wl = (torch.randn(s, dtype=torch.float64, generator=gen).to(DEV) for s in ((T, N, Do), (T, N, Do, Do), (N,)))
        loss = lambda means, covs, ll: (Wm * means).sum() + (Wc * covs).sum() + (Wl * ll).sum()
        pack = gp._prepared()
        lay = pack.layout
        keep = {}

        def leaves():
            return {k: i[k].clone().requires_grad_() for k in NAMES}

        def fused():
            lv = leaves()
            res = gp.adf(*[lv[k] for k in NAMES], cond=i['cond'], input_grads=True)
            loss(res.means, res.covs, res.loglik).backward()
            keep['fused'] = [lv[k].grad for k in NAMES]

        def loop():
            lv = leaves()
            loss(*python_loop(gp, lv, i['cond'], Do, Dy, T)).backward()
            keep['loop'] = [lv[k].grad for k in NAMES]

        rec = ag.gp_adf_eval(pack, *[i[k] for k in NAMES], cond=i['cond'])
        assert int(rec.info.abs().sum()) == 0
        info = rec.info.to(torch.float64)
        nwork = int(lib.cbfssm_gp_adf_bwd_work_elems(C.byref(lay), N))
        work = torch.full((nwork,), float('nan'), dtype=torch.float64, device=DEV)
        out = {k: torch.full_like(i[k], float('nan')) for k in NAMES}

        def bwd():
            hl.check(lib.cbfssm_gp_adf_bwd_f64(C.byref(lay), _ptr(pack.buf), _ptr(i['m0']), _ptr(i['P0']), _ptr(i['a']), _ptr(i['y']),
                                               _ptr(i['cond']), _ptr(i['var_x']), _ptr(i['var_y']), Dy, _ptr(rec.means),
                                               _ptr(rec.covs), _ptr(rec.pmeans), _ptr(rec.pcovs), _ptr(info), _ptr(Wm), _ptr(Wc),
                                               _ptr(Wl), N, T, _ptr(out['m0']), _ptr(out['P0']), _ptr(out['a']), _ptr(out['y']),
                                               _ptr(out['var_x']), _ptr(out['var_y']), _ptr(work), _stream()), 'bwd')

        fns = {'fused': fused, 'bwd_launch': bwd,
               'fwd_launch': lambda: ag.gp_adf_eval(pack, *[i[k] for k in NAMES], cond=i['cond']), 'loop': loop}
        for _ in range(2):
            for f in fns.values():
                f()
        torch.cuda.synchronize()
        err = [float(((x - z).abs().max() / z.abs().max()).cpu()) for x, z in zip(keep['fused'], keep['loop'])]
        assert max(err) <= 1e-6, err
        assert all(torch.equal(x, out[k]) for k, x in zip(NAMES, keep['fused']))
        res = {k: [] for k in fns}
        for _ in range(rounds):
            for k, f in fns.items():
                res[k].append(timed(f))
        med = {k: float(np.median(v)) for k, v in res.items()}
        print(json.dumps({'shape': [M, D, Do, N, T, Dy], 'rounds': rounds, 'form': gp._pack.gp_form(), 'ms_median': med,
                          'ms_min': {k: float(np.min(v)) for k, v in res.items()},
                          'ms_max': {k: float(np.max(v)) for k, v in res.items()},
                          'fused_median_below_every_loop_value': bool(med['fused'] < np.min(res['loop'])),
                          'loop_over_fused': med['loop'] / med['fused'],
                          'bwd_launch_over_fwd_launch': med['bwd_launch'] / med['fwd_launch'],
                          'work_bytes': 8 * nwork, 'max_rel_diff_of_the_six_gradients_vs_loop': err}), flush=True)


if __name__ == '__main__':
    main()
