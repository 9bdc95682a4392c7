"""Differentiable GPModel against what a user could do before it existed: torch autograd of the same function written in
tensor-library ops (kernel matrix, torch.linalg.cholesky, two triangular solves) in float64 on the same GPU.

    python profiles/tools/gp_autograd_time.py [rounds] [reps]

Per shape (M, D, Do, npts): the predict-under-grad forward and the full backward of (fmean, fvar) into X and the five
parameter tensors, HIP events around `reps` calls, the two sides alternating over `rounds`; plus the backward entry point
cbfssm_gp_predict_bwd_f64 on its own and its share of the f64 matrix peak priced at 3 F per point (A2 is
recomputed).  Prints one JSON line per shape."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'cbf-ssm_amd')]

import numpy as np
import torch

from cbfssm.hip import lib as _l
from cbfssm.hip.ops import _ptr, _stream
from cbfssm.model import gp_tf

F64_MFMA_PEAK_TFLOPS = 78.6
SHAPES = [(100, 21, 14, 65536), (200, 13, 7, 65536)]
DEV = 'cuda:0'


def softplus_inverse(y):
    y = np.asarray(y, dtype=np.float64) - 1e-10
    return y + np.log(-np.expm1(-y))


def make(M, D, Do, npts):
    rng = np.random.default_rng(M)
    ls = rng.uniform(0.8, 1.25, D) * max(1.0, 0.75 * np.sqrt(D))
    p = [rng.uniform(-2, 2, (M, D)), 0.5 * rng.standard_normal((M, Do)),
         softplus_inverse(0.05 * np.exp(rng.uniform(-1, 1, (M, Do)))), softplus_inverse(np.array([0.4])), softplus_inverse(ls)]
    X = 1.4 * rng.standard_normal((npts, D))
    return p, X, rng.standard_normal((npts, Do)), rng.standard_normal((npts, Do))


def sp(x):
    return torch.nn.functional.softplus(x, beta=1.0, threshold=1e9) + 1e-10


def torch_predict(X, zp, zm, zvu, varu, lsu):
    """gp_tf.py:33-49,129-161 in tensor-library ops"""
    ls, var, zvar = sp(lsu), sp(varu), sp(zvu)

    def K(a, b):
        a, b = a / ls, b / ls
        return var * torch.exp(-0.5 * (-2 * a @ b.T + (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :]))
    M = zp.shape[0]
    L = torch.linalg.cholesky(K(zp, zp) + 1e-8 * torch.eye(M, dtype=torch.float64, device=zp.device))
    A = torch.linalg.solve_triangular(L, K(zp, X), upper=False)
    fvar0 = var.squeeze() - (A * A).sum(0)
    A = torch.linalg.solve_triangular(L.T, A, upper=True)
    return A.T @ zm, fvar0[:, None] + (A * A).T @ zvar


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
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    for M, D, Do, npts in SHAPES:
        p, X, Wm, Wv = make(M, D, Do, npts)
        t = lambda a: torch.tensor(a, dtype=torch.float64, device=DEV)
        gp = gp_tf.GPModel(D, Do, M, 0.4, 1.0, 0.1, 1.0, 0.01, seed=0, device=DEV)
        gp.zeta_pos, gp.zeta_mean, gp.zeta_var_unc, gp.kern.variance_unc, gp.kern.lengthscales_unc = [t(a) for a in p]
        leaves = gp.parameters()
        tl = [t(a).requires_grad_() for a in p]
        for q in leaves:
            q.requires_grad_()
        Xh, Xt = t(X).requires_grad_(), t(X).requires_grad_()
        Wm, Wv = t(Wm), t(Wv)
        keep = {}

        def hip_fwd():
            keep['h'] = gp.predict(Xh)

        def hip_bwd():
            keep['gh'] = torch.autograd.grad(keep['h'], [Xh] + leaves, [Wm, Wv], retain_graph=True)

        def torch_fwd():
            keep['t'] = torch_predict(Xt, *tl)

        def torch_bwd():
            keep['gt'] = torch.autograd.grad(keep['t'], [Xt] + tl, [Wm, Wv], retain_graph=True)
        for _ in range(3):
            hip_fwd(); hip_bwd(); torch_fwd(); torch_bwd()
        torch.cuda.synchronize()
        err = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(keep['gh'], keep['gt']))
        res = {k: [] for k in ('hip_fwd', 'hip_bwd', 'torch_fwd', 'torch_bwd')}
        for _ in range(rounds):
            for k, fn in (('hip_fwd', hip_fwd), ('torch_fwd', torch_fwd), ('hip_bwd', hip_bwd), ('torch_bwd', torch_bwd)):
                res[k].append(timed(fn, reps))
        # the backward entry point on its own (stash tile heights: clear + kernel + contraction)
        lib = _l.load()
        pack = gp._pack
        lay = pack.layout
        nwg = int(lib.cbfssm_gp_predict_bwd_workgroups(C.byref(lay), npts))
        nwork = int(lib.cbfssm_gp_predict_bwd_work_elems(C.byref(lay), npts))
        gpart = torch.empty((nwg + 32) * lay.rev_slab, dtype=torch.float64, device=DEV)
        work = torch.empty(nwork, dtype=torch.float64, device=DEV) if nwork else None
        image = torch.empty(lay.NBLK * lay.NBLK * 256, dtype=torch.float64, device=DEV) if lay.rev_stash else None
        gX, Xd = torch.empty_like(Xh), Xh.detach()

        def entry():
            _l.check(lib.cbfssm_gp_predict_bwd_f64(C.byref(lay), _ptr(pack.buf), _ptr(Xd), npts, _ptr(Wm), _ptr(Wv), _ptr(gX),
                                                   _ptr(gpart), _ptr(work), _ptr(image), _stream()), 'cbfssm_gp_predict_bwd_f64')
        entry()
        torch.cuda.synchronize()
        ent = [timed(entry, reps) for _ in range(rounds)]
        flops = 3.0 * npts * (2 * M * M + M * (2 * D + 5 * Do + 5))
        med = {k: float(np.median(v)) for k, v in res.items()}
        out = {'shape': [M, D, Do, npts], 'rounds': rounds, 'reps': reps, 'ms_median': med,
               'ms_min': {k: float(np.min(v)) for k, v in res.items()},
               'hip_total_ms': med['hip_fwd'] + med['hip_bwd'], 'torch_total_ms': med['torch_fwd'] + med['torch_bwd'],
               'bwd_entry_ms_median': float(np.median(ent)), 'bwd_entry_ms_min': float(np.min(ent)),
               'bwd_entry_tflops_3F': flops / (float(np.median(ent)) * 1e-3) / 1e12,
               'bwd_entry_frac_f64_mfma_peak': flops / (float(np.median(ent)) * 1e-3) / 1e12 / F64_MFMA_PEAK_TFLOPS,
               'workgroups': nwg, 'grad_max_rel_diff_hip_vs_torch': err}
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
