"""The fused GP rollout against what the library offered before it: a Python loop of one `gp_predict` per step plus
tensor-library elementwise ops, under torch autograd, on the same GPU.

    python profiles/tools/gp_rollout_time.py [rounds] [reps]

Per shape (M, D, Do, N, T): forward under grad plus the full backward into h0, a, var_add and the five parameter tensors,
HIP events around `reps` calls, the two sides alternating over `rounds` after two warm-up calls each; plus the adjoint entry
point cbfssm_gp_rollout_bwd_f64 on its own and its share of the f64 matrix peak priced at 3 F per GP evaluation (the kernel
tile and A2 are recomputed).  Prints one JSON line per shape."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'cbf-ssm_amd')]

import numpy as np
import torch

from cbfssm.hip import autograd
from cbfssm.hip import lib as _l
from cbfssm.hip.ops import _ptr, _stream
from cbfssm.model import gp_tf

F64_MFMA_PEAK_TFLOPS = 78.6
SHAPES = [(100, 21, 14, 5120, 250), (20, 19, 6, 320, 64)]
DEV = 'cuda:0'
LOG2PIE = float(np.log(2.0 * np.pi * np.e))


def softplus_inverse(y):
    y = np.asarray(y, dtype=np.float64) - 1e-10
    return y + np.log(-np.expm1(-y))


def make(M, D, Do, N, T):
    rng = np.random.default_rng(M)
    ls = rng.uniform(0.8, 1.25, D) * max(1.0, 0.75 * np.sqrt(D))
    p = [rng.uniform(-2, 2, (M, D)), 0.1 * rng.standard_normal((M, Do)),
         softplus_inverse(0.05 * np.exp(rng.uniform(-1, 1, (M, Do)))), softplus_inverse(np.array([0.4])), softplus_inverse(ls)]
    return (p, 0.5 * rng.standard_normal((N, Do)), 1.4 * rng.standard_normal((T, N, D - Do)), rng.standard_normal((T, N)),
            0.02 * np.exp(rng.uniform(-1, 1, Do)), rng.standard_normal((T, N, Do)))


def loop_rollout(gp, h0, a, eps, var_add):
    """the per-step loop: T launches of the predict kernel, T prepares, T adjoint launches"""
    h, ent, rows = h0, 0.0, []
    for t in range(eps.shape[0]):
        fmean, fvar = autograd.gp_predict(gp._pack, torch.cat([h, a[t]], 1), *gp.parameters())
        v = fvar + var_add
        h = h + fmean + eps[t][:, None] * torch.sqrt(v)
        rows.append(h)
        ent = ent + 0.5 * torch.sum(LOG2PIE + torch.log(v))
    return torch.stack(rows), ent


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
        p, h0, a, eps, var_add, W = make(M, D, Do, N, T)
        t = lambda x: torch.tensor(x, dtype=torch.float64, device=DEV)
        gp = gp_tf.GPModel(D, Do, M, 0.4, 1.0, 0.1, 1.0, 0.01, seed=0, device=DEV)
        gp.zeta_pos, gp.zeta_mean, gp.zeta_var_unc, gp.kern.variance_unc, gp.kern.lengthscales_unc = [t(x) for x in p]
        leaves = gp.parameters()
        for q in leaves:
            q.requires_grad_()
        h0d, ad, vad = t(h0).requires_grad_(), t(a).requires_grad_(), t(var_add).requires_grad_()
        epsd, Wd = t(eps), t(W)
        wrt = [h0d, ad, vad] + leaves
        keep = {}

        def fused():
            traj, ent = gp.rollout(h0d, ad, epsd, vad)
            keep['f'] = torch.autograd.grad((Wd * traj).sum() + 0.7 * ent, wrt)

        def loop():
            traj, ent = loop_rollout(gp, h0d, ad, epsd, vad)
            keep['l'] = torch.autograd.grad((Wd * traj).sum() + 0.7 * ent, wrt)
        for _ in range(2):
            fused(); loop()
        torch.cuda.synchronize()
        err = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(keep['f'], keep['l']))
        res = {'fused': [], 'loop': []}
        for _ in range(rounds):
            res['fused'].append(timed(fused, reps))
            res['loop'].append(timed(loop, 1))
        # the two entry points on their own
        lib = _l.load()
        pack = gp._pack
        lay = pack.layout
        groups = int(lib.cbfssm_gp_rollout_partials(C.byref(lay), N))
        nwork = int(lib.cbfssm_gp_rollout_bwd_work_elems(C.byref(lay), N, T))
        traj, vsave = torch.empty(T, N, Do, dtype=torch.float64, device=DEV), torch.empty(T, N, Do, dtype=torch.float64, device=DEV)
        ent_part = torch.empty(groups + 32, dtype=torch.float64, device=DEV)
        gpart = torch.empty((groups + 32) * lay.rev_slab, dtype=torch.float64, device=DEV)
        work = torch.empty(nwork, dtype=torch.float64, device=DEV) if nwork else None
        image = torch.empty(lay.NBLK * lay.NBLK * 256, dtype=torch.float64, device=DEV) if lay.rev_stash else None
        gh0, ga, gent = torch.empty_like(h0d), torch.empty_like(ad), t([0.7])
        h0c, ac, vac = h0d.detach(), ad.detach(), vad.detach()

        def entry_fwd():
            _l.check(lib.cbfssm_gp_rollout_f64(C.byref(lay), _ptr(pack.buf), _ptr(h0c), _ptr(ac), _ptr(epsd), _ptr(vac), N, T, 0,
                                               _ptr(traj), _ptr(vsave), _ptr(ent_part), _stream()), 'cbfssm_gp_rollout_f64')

        def entry_bwd():
            _l.check(lib.cbfssm_gp_rollout_bwd_f64(C.byref(lay), _ptr(pack.buf), _ptr(h0c), _ptr(ac), _ptr(epsd), _ptr(traj),
                                                   _ptr(vsave), _ptr(Wd), _ptr(gent), N, T, 0, _ptr(gh0), _ptr(ga), _ptr(gpart),
                                                   _ptr(work), _ptr(image), _stream()), 'cbfssm_gp_rollout_bwd_f64')
        entry_fwd(); entry_bwd()
        torch.cuda.synchronize()
        ef = [timed(entry_fwd, reps) for _ in range(rounds)]
        eb = [timed(entry_bwd, reps) for _ in range(rounds)]
        flops = 3.0 * N * T * (2 * M * M + M * (2 * D + 5 * Do + 5))
        med = {k: float(np.median(v)) for k, v in res.items()}
        out = {'shape': [M, D, Do, N, T], 'rounds': rounds, 'reps': reps, 'ms_median': med,
               'ms_min': {k: float(np.min(v)) for k, v in res.items()}, 'ms_max': {k: float(np.max(v)) for k, v in res.items()},
               'loop_over_fused': med['loop'] / med['fused'],
               'fwd_entry_ms_median': float(np.median(ef)), 'bwd_entry_ms_median': float(np.median(eb)),
               'bwd_entry_ms_min': float(np.min(eb)),
               'bwd_entry_tflops_3F': flops / (float(np.median(eb)) * 1e-3) / 1e12,
               'bwd_entry_frac_f64_mfma_peak': flops / (float(np.median(eb)) * 1e-3) / 1e12 / F64_MFMA_PEAK_TFLOPS,
               'workgroups': groups, 'grad_max_rel_diff_fused_vs_loop': err}
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
