"""GPModel.moment_match(..., input_grads=True), forward under grad plus backward, against tensor-library autograd through the
same closed form (gp_moment_match_time.torch_closed_form, chunks of 1024 points).

    python profiles/tools/gp_moment_match_grad_time.py [rounds]

Per shape (M, D, Do, N), float64, the shapes of profiles/gp_moment_match/: HIP events around one call, the measurements
alternating over `rounds` (default 5) after two warm-up calls each; the median is reported.  The loss is
sum Wf o fmean + sum Wc o fcov + sum Wx o xcov with fixed random weights.

    hip              forward under grad and backward through GPModel.moment_match(mean, cov, input_grads=True)
    bwd_launch       cbfssm_gp_moment_match_bwd_f64 alone on the prepared pack (two pre-kernels, one launch)
    fwd_launch       cbfssm.hip.autograd.gp_moment_match_eval on the prepared pack
    torch            forward and backward of the tensor-library closed form, chunk by chunk (each chunk's tape freed by its own
                     backward)

The gradients of the two paths are compared.  Prints one JSON line per shape."""
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
from gp_ekf_time import DEV, make, timed
from gp_moment_match_time import CHUNK, SHAPES, torch_closed_form


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
        work = torch.empty(int(lib.cbfssm_gp_moment_match_bwd_work_elems(C.byref(lay))), dtype=torch.float64, device=DEV)
        gm, gc = torch.empty_like(mean), torch.empty_like(cov)
        keep = {}

        def hip():
            m, c = mean.clone().requires_grad_(), cov.clone().requires_grad_()
            fm, fc, xc, _ = gp.moment_match(m, c, input_grads=True)
            ((Wf * fm).sum() + (Wc * fc).sum() + (Wx * xc).sum()).backward()
            keep['hip'] = (m.grad, c.grad)

        def tl():
            m, c = mean.clone().requires_grad_(), cov.clone().requires_grad_()
            for c0 in range(0, N, CHUNK):
                s = slice(c0, c0 + CHUNK)
                cs = torch.tril(c[s]) + torch.tril(c[s], -1).transpose(1, 2)
                fm, fc, xc = torch_closed_form(gp, pack, m[s], cs)
                ((Wf[s] * fm).sum() + (Wc[s] * fc).sum() + (Wx[s] * xc).sum()).backward()
            keep['torch'] = (m.grad, c.grad)

        def bwd():
            hl.check(lib.cbfssm_gp_moment_match_bwd_f64(C.byref(lay), _ptr(pack.buf), _ptr(mean), _ptr(cov), N, _ptr(Wf), _ptr(Wc),
                                                        _ptr(Wx), _ptr(gm), _ptr(gc), None, _ptr(work), _stream()), 'bwd')

        fns = {'hip': hip, 'bwd_launch': bwd, 'fwd_launch': lambda: ag.gp_moment_match_eval(pack, mean, cov), 'torch': tl}
        for _ in range(2):
            for f in fns.values():
                f()
        torch.cuda.synchronize()
        err = [float(((x - z).abs().max() / z.abs().max()).cpu()) for x, z in zip(keep['hip'], keep['torch'])]
        res = {k: [] for k in fns}
        for _ in range(rounds):
            for k, f in fns.items():
                res[k].append(timed(f))
        med = {k: float(np.median(v)) for k, v in res.items()}
        print(json.dumps({'shape': [M, D, Do, N], 'rounds': rounds, 'form': gp._pack.gp_form(), 'chunk': CHUNK, 'ms_median': med,
                          'ms_min': {k: float(np.min(v)) for k, v in res.items()},
                          'ms_max': {k: float(np.max(v)) for k, v in res.items()},
                          'hip_median_below_every_torch_value': bool(med['hip'] < np.min(res['torch'])),
                          'torch_over_hip': med['torch'] / med['hip'], 'bwd_launch_over_fwd_launch': med['bwd_launch'] / med['fwd_launch'],
                          'max_rel_diff_gmean_gcov_vs_torch': err}), flush=True)


if __name__ == '__main__':
    main()
