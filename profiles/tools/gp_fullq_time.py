"""The differentiable full-covariance conditional against the same function in tensor-library ops under torch autograd on
the same GPU (the yardstick of DESIGN 3.2b).

    python profiles/tools/gp_fullq_time.py [rounds] [reps]

Per shape (M, D, Do, npts): forward under grad plus the full backward into X, zeta_pos, zeta_mean, q_sqrt, variance_unc
and lengthscales_unc, of  sum(Wm o fmean) + sum(Wv o fvar) + 0.3 prior_kl.  HIP events around `reps` calls, the two sides
alternating over `rounds` after two warm-up calls each; the median is reported.  In the same rounds, on one prepared pack
and through the C ABI: the forward on the MFMA units (cbfssm_gp_fullq_predict_f64, S_d images built beforehand; and with
cbfssm_gp_fullq_prepare_f64 in the timed region) against the scalar-FMA forward cbfssm_gp_predict_fullq_f64.  Prints one JSON
line per shape."""
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

SHAPES = [(100, 21, 14, 65536), (200, 13, 7, 65536)]
DEV = 'cuda:0'
KL_WEIGHT = 0.3


def softplus_inverse(y):
    y = np.asarray(y, dtype=np.float64) - 1e-10
    return y + np.log(-np.expm1(-y))


def make(M, D, Do, npts):
    rng = np.random.default_rng(M)
    ls = rng.uniform(0.8, 1.25, D) * max(1.0, 0.75 * np.sqrt(D))
    q = np.tril(0.03 * rng.standard_normal((Do, M, M)), -1) + 0.2 * np.exp(rng.uniform(-0.5, 0.5, (Do, M)))[:, :, None] * np.eye(M)
    p = [rng.uniform(-2, 2, (M, D)), 0.5 * rng.standard_normal((M, Do)), q, softplus_inverse(np.array([0.4])), softplus_inverse(ls)]
    return p, 1.4 * rng.standard_normal((npts, D)), rng.standard_normal((npts, Do)), rng.standard_normal((npts, Do))


def torch_fullq(X, Z, f, q, var_unc, ls_unc):
    """the same function in tensor-library ops, in the reference's order (gp_tf.py:76-98) with the KL in closed form"""
    sp = torch.nn.functional.softplus
    var, ls = (sp(var_unc) + 1e-10).reshape(()), sp(ls_unc) + 1e-10
    M, Do = f.shape

    def rbf(a, b):
        a, b = a / ls, b / ls
        return var * torch.exp(-0.5 * (-2.0 * a @ b.T + (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :]))
    Lq = torch.tril(q)
    Lm = torch.linalg.cholesky(rbf(Z, Z) + 1e-8 * torch.eye(M, dtype=torch.float64, device=Z.device))
    A = torch.linalg.solve_triangular(Lm, rbf(Z, X), upper=False)
    fvar = var - (A * A).sum(0)
    A = torch.linalg.solve_triangular(Lm.T, A, upper=True)
    fmean = A.T @ f
    LTA = Lq.transpose(1, 2) @ A[None]
    fvar = fvar[None, :] + (LTA * LTA).sum(1)
    B = torch.linalg.solve_triangular(Lm, Lq, upper=False)
    a = torch.linalg.solve_triangular(Lm, f, upper=False)
    dq = torch.diagonal(Lq, dim1=1, dim2=2)
    kl = 0.5 * ((B * B).sum() + (a * a).sum() - Do * M + 2.0 * Do * torch.log(torch.diagonal(Lm)).sum() - torch.log(dq * dq).sum())
    return fmean, fvar.T, kl


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
    for M, D, Do, npts in SHAPES:
        p, X, Wm, Wv = make(M, D, Do, npts)
        t = lambda x: torch.tensor(x, dtype=torch.float64, device=DEV)
        gp = gp_tf.GPModel(D, Do, M, 0.4, 1.0, 0.1, 1.0, 0.01, seed=0, device=DEV, q_full=True)
        gp.zeta_pos, gp.zeta_mean, gp.zeta_sqrt, gp.kern.variance_unc, gp.kern.lengthscales_unc = [t(x) for x in p]
        leaves = gp.parameters()
        for q in leaves:
            q.requires_grad_()
        Xd, Wmd, Wvd = t(X).requires_grad_(), t(Wm), t(Wv)
        wrt = [Xd] + leaves
        keep = {}

        def hip():
            fmean, fvar = gp.predict(Xd)
            keep['h'] = torch.autograd.grad((Wmd * fmean).sum() + (Wvd * fvar).sum() + KL_WEIGHT * gp.prior_kl(), wrt)

        def lib_ops():
            fmean, fvar, kl = torch_fullq(Xd, *leaves)
            keep['t'] = torch.autograd.grad((Wmd * fmean).sum() + (Wvd * fvar).sum() + KL_WEIGHT * kl, wrt)

        lib, pack = _l.load(), gp._prepared()
        lay, Xc, qt = pack.layout, Xd.detach().contiguous(), torch.tril(gp.zeta_sqrt.detach()).contiguous()
        fm, fv = torch.empty(npts, Do, dtype=torch.float64, device=DEV), torch.empty(npts, Do, dtype=torch.float64, device=DEV)
        fm0, fv0 = torch.empty_like(fm), torch.empty_like(fv)
        qpack = torch.empty(lib.cbfssm_gp_fullq_pack_elems(C.byref(lay)), dtype=torch.float64, device=DEV)
        work = torch.empty(lib.cbfssm_gp_predict_fullq_work_elems(C.byref(lay), npts), dtype=torch.float64, device=DEV)

        def build_s():
            _l.check(lib.cbfssm_gp_fullq_prepare_f64(C.byref(lay), _ptr(qt), _ptr(qpack), _stream()), 'prepare')

        def forward_mfma():
            _l.check(lib.cbfssm_gp_fullq_predict_f64(C.byref(lay), _ptr(pack.buf), _ptr(qpack), _ptr(Xc), npts, _ptr(fm), _ptr(fv),
                                                     _stream()), 'forward')

        def forward_mfma_with_s():
            build_s(); forward_mfma()

        def forward_scalar():
            _l.check(lib.cbfssm_gp_predict_fullq_f64(C.byref(lay), _ptr(pack.buf), _ptr(qt), _ptr(Xc), npts, _ptr(fm0), _ptr(fv0),
                                                     _ptr(work), _stream()), 'old forward')
        build_s()
        for _ in range(2):
            forward_mfma(); forward_mfma_with_s(); forward_scalar()
        torch.cuda.synchronize()
        ferr = float(((fv - fv0).abs().max() / fv0.abs().max()).cpu())
        for _ in range(2):
            hip(); lib_ops()
        torch.cuda.synchronize()
        err = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(keep['h'], keep['t']))
        res = {'hip': [], 'tensor_library': [], 'forward_mfma': [], 'forward_mfma_with_s': [], 'forward_scalar': []}
        for _ in range(rounds):
            res['hip'].append(timed(hip, reps))
            res['tensor_library'].append(timed(lib_ops, reps))
            res['forward_mfma'].append(timed(forward_mfma, reps))
            res['forward_mfma_with_s'].append(timed(forward_mfma_with_s, reps))
            res['forward_scalar'].append(timed(forward_scalar, reps))
        med = {k: float(np.median(v)) for k, v in res.items()}
        out = {'shape': [M, D, Do, npts], 'rounds': rounds, 'reps': reps, 'ms_median': med,
               'ms_min': {k: float(np.min(v)) for k, v in res.items()}, 'ms_max': {k: float(np.max(v)) for k, v in res.items()},
               'tensor_library_over_hip': med['tensor_library'] / med['hip'],
               'forward_scalar_over_mfma': med['forward_scalar'] / med['forward_mfma'], 'fvar_max_rel_diff_mfma_vs_scalar': ferr, 'grad_max_rel_diff_hip_vs_tensor_library': err}
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
