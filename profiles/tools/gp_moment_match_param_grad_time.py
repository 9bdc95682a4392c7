"""GPModel.moment_match(..., differentiable=True), forward under grad plus the full backward into the five leaves, mean and
cov, against tensor-library autograd FROM THE LEAVES through the same closed form (gp_moment_match_time.torch_closed_form,
chunks of 1024 points).

    python profiles/tools/gp_moment_match_param_grad_time.py [rounds]

Per shape (M, D, Do, N), float64, the shapes of profiles/gp_moment_match/: HIP events around one call, the measurements
alternating over `rounds` (default 5) after two warm-up calls each; the median is reported.  The loss is
sum Wf o fmean + sum Wc o fcov + sum Wx o xcov with fixed random weights.

    hip              forward under grad and backward through GPModel.moment_match(mean, cov, differentiable=True)
    new_launches     cbfssm_gp_moment_match_params_bwd_f64 alone on the prepared pack (the launches this adjoint adds)
    input_launch     cbfssm_gp_moment_match_bwd_f64 alone (the input adjoint the backward runs first)
    tail             cbfssm_gp_tail_f64 alone on the slab
    torch            the tensor-library path: softplus, K_mm + jitter I and its inverse from the leaves once per call on the
                     tape; the closed form chunk by chunk over detached copies of those constants, each chunk's tape freed by
                     its own backward; then one backward from the copies' gradients into the leaves

The gradients of the two paths are compared.  Prints one JSON line per shape."""
import ctypes as C
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'cbf-ssm_amd'), os.path.dirname(os.path.abspath(__file__))]

import numpy as np
import torch

from cbfssm.hip import autograd as ag
from cbfssm.hip import lib as hl
from cbfssm.hip.ops import _ptr, _stream, tf_forward
from cbfssm.model import gp_tf
from gp_ekf_time import DEV, make, timed
from gp_moment_match_time import CHUNK, SHAPES, torch_closed_form

JITTER = 1e-8


def torch_from_leaves(leaves, mean, cov, weights):
    """loss.backward() of the tensor-library path; the gradients land in .grad of the leaves, mean and cov"""
    zp, zm, zv, var_u, ls_u = leaves
    M = zp.shape[0]
    ls, v, s2 = tf_forward(ls_u), tf_forward(var_u), tf_forward(zv)
    Zs = zp / ls
    d2 = ((Zs[:, None, :] - Zs[None, :, :]) ** 2).sum(-1)
    Kinv = torch.linalg.inv(v.reshape(()) * torch.exp(-0.5 * d2) + JITTER * torch.eye(M, dtype=torch.float64, device=zp.device))
    consts = (zp, ls, v, zm, s2, Kinv)
    cp = [c.detach().requires_grad_() for c in consts]
    shim = types.SimpleNamespace(zeta_pos=cp[0], zeta_mean=cp[3], zeta_var=cp[4],
                                 kern=types.SimpleNamespace(lengthscales=cp[1], variance=cp[2]))
    pk = types.SimpleNamespace(buf=cp[5].reshape(-1), layout=types.SimpleNamespace(Kinv=0))
    Wf, Wc, Wx = weights
    for c0 in range(0, mean.shape[0], CHUNK):
        s = slice(c0, c0 + CHUNK)
        cs = torch.tril(cov[s]) + torch.tril(cov[s], -1).transpose(1, 2)
        fm, fc, xc = torch_closed_form(shim, pk, mean[s], cs)
        ((Wf[s] * fm).sum() + (Wc[s] * fc).sum() + (Wx[s] * xc).sum()).backward()
    torch.autograd.backward([c for c in consts], [c.grad for c in cp])


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    lib = hl.load()
    for M, D, Do, N in SHAPES:
        p, raw = make(M, D, Do, N, 1, 1)
        t = lambda x: torch.tensor(x, dtype=torch.float64, device=DEV)
        gp = gp_tf.GPModel(D, Do, M, 0.4, 1.0, 0.1, 1.0, 0.01, seed=0, device=DEV)
        gp.zeta_pos, gp.zeta_mean, gp.zeta_var_unc, gp.kern.variance_unc, gp.kern.lengthscales_unc = [t(x) for x in p]
        mean = torch.cat([t(raw['m0']), t(raw['a'][0])], 1).contiguous()
        cov = torch.zeros(N, D, D, dtype=torch.float64, device=DEV)
        cov[:, :Do, :Do] = t(raw['P0'])
        gen = torch.Generator(device='cpu').manual_seed(3)
        Wf, Wc, Wx = (torch.randn(s, dtype=torch.float64, generator=gen).to(DEV) for s in ((N, Do), (N, Do, Do), (N, Do, D)))
        pack = gp._prepared()
        lay = pack.layout
        pflat, cflat = ag._gp_flat(gp.parameters())
        nan = float('nan')
        full = lambda n: torch.full((int(n),), nan, dtype=torch.float64, device=DEV)
        work_in = full(lib.cbfssm_gp_moment_match_bwd_work_elems(C.byref(lay)))
        nwork = int(lib.cbfssm_gp_moment_match_params_bwd_work_elems(C.byref(lay), N))
        work, twork = full(nwork), full(lib.cbfssm_train_tail_half_work_elems(C.byref(lay)))
        red, dense = full(lay.rev_slab), (full(M * M) if lay.rev_stash else None)
        gm, gc, gflat = torch.full_like(mean, nan), torch.full_like(cov, nan), torch.full_like(pflat, nan)
        xcov = ag.gp_moment_match_eval(pack, mean, cov)[2]
        keep = {}

        def hip():
            leaves = gp.parameters()
            for x in leaves:
                x.grad = None
                x.requires_grad_()
            m, c = mean.clone().requires_grad_(), cov.clone().requires_grad_()
            fm, fc, xc, _ = gp.moment_match(m, c, differentiable=True)
            ((Wf * fm).sum() + (Wc * fc).sum() + (Wx * xc).sum()).backward()
            keep['hip'] = [x.grad for x in leaves] + [m.grad, c.grad]
            for x in leaves:
                x.requires_grad_(False)

        def tl():
            leaves = [x.detach().clone().requires_grad_() for x in gp.parameters()]
            m, c = mean.clone().requires_grad_(), cov.clone().requires_grad_()
            torch_from_leaves(leaves, m, c, (Wf, Wc, Wx))
            keep['torch'] = [x.grad for x in leaves] + [m.grad, c.grad]

        def inp():
            hl.check(lib.cbfssm_gp_moment_match_bwd_f64(C.byref(lay), _ptr(pack.buf), _ptr(mean), _ptr(cov), N, _ptr(Wf), _ptr(Wc),
                                                        _ptr(Wx), _ptr(gm), _ptr(gc), None, _ptr(work_in), _stream()), 'bwd')

        def new():
            hl.check(lib.cbfssm_gp_moment_match_params_bwd_f64(C.byref(lay), _ptr(pack.buf), _ptr(cflat), _ptr(mean), _ptr(cov), N,
                                                               _ptr(Wf), _ptr(Wc), _ptr(Wx), _ptr(gm), _ptr(gc), _ptr(xcov),
                                                               _ptr(red), _ptr(dense), _ptr(work), _stream()), 'params bwd')

        def tail():
            hl.check(lib.cbfssm_gp_tail_f64(C.byref(lay), _ptr(pack.buf), _ptr(red), _ptr(dense), M if lay.rev_stash else 0, 0.0,
                                            _ptr(pflat), _ptr(cflat), _ptr(twork), _ptr(gflat), _stream()), 'tail')

        fns = {'hip': hip, 'input_launch': inp, 'new_launches': new, 'tail': tail, 'torch': tl}
        for _ in range(2):
            for f in fns.values():
                f()
        torch.cuda.synchronize()
        names = list(ag.GP_PARAM_NAMES) + ['mean', 'cov']
        err = {k: float(((x.reshape(z.shape) - z).abs().max() / z.abs().max()).cpu())
               for k, x, z in zip(names, keep['hip'], keep['torch'])}
        res = {k: [] for k in fns}
        for _ in range(rounds):
            for k, f in fns.items():
                res[k].append(timed(f))
        med = {k: float(np.median(v)) for k, v in res.items()}
        print(json.dumps({'shape': [M, D, Do, N], 'rounds': rounds, 'form': gp._pack.gp_form(), 'chunk': CHUNK, 'ms_median': med,
                          'ms_min': {k: float(np.min(v)) for k, v in res.items()},
                          'ms_max': {k: float(np.max(v)) for k, v in res.items()},
                          'hip_median_below_every_torch_value': bool(med['hip'] < np.min(res['torch'])),
                          'torch_over_hip': med['torch'] / med['hip'], 'work_MB': nwork * 8 / 1e6,
                          'max_rel_diff_vs_torch': err}), flush=True)


if __name__ == '__main__':
    main()
