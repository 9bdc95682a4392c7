"""GPModel.moment_match against the same closed form written in the tensor library, and against GPModel.linearize (what
exactness costs over the first-order model).

    python profiles/tools/gp_moment_match_time.py [rounds]

Per shape (M, D, Do, N), float64, the shapes of the ekf record: HIP events around one call, the measurements alternating
over `rounds` (default 5) after two warm-up calls each; the median is reported.  The belief of every point is that of
transition_moments: x ~ N(concat(h, a), blockdiag(P, 0)).

    mm               GPModel.moment_match(mean, cov)                       prepare, two pre-kernels, one launch
    mm_nocross       the same with cross=False
    mm_launch, mm_nocross_launch     cbfssm.hip.autograd.gp_moment_match_eval on the pack prepared beforehand
    torch            the closed form in the tensor library on the device, from the prepared pack's K^-1: batched inverses and
                     determinants of I + S~ and I / 2 + S~, the (chunk, M, M) matrix of expected kernel products, matrix
                     products for the contractions; chunks of CHUNK points so that the intermediate fits
    lin              GPModel.linearize(mean)                               prepare, one pre-kernel, one launch
    lin_launch       cbfssm.hip.autograd.gp_linearize_eval on the prepared pack

torch's results are compared with mm's.  Prints one JSON line per shape."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'cbf-ssm_amd'), os.path.dirname(os.path.abspath(__file__))]

import numpy as np
import torch

from cbfssm.hip import autograd as ag
from cbfssm.model import gp_tf
from gp_ekf_time import DEV, make, timed

SHAPES = [(100, 21, 14, 5120), (20, 19, 6, 320)]
CHUNK = 1024


def torch_closed_form(gp, pack, mean, cov):
    """the formulas of csrc/cbfssm_gp_mm.hpp with (chunk, M, M) intermediates"""
    ls, v = gp.kern.lengthscales, gp.kern.variance.reshape(())
    M, D = gp.zeta_pos.shape
    Zs = gp.zeta_pos / ls
    Kinv = pack.buf[pack.layout.Kinv:pack.layout.Kinv + M * M].view(M, M)
    alpha = Kinv @ gp.zeta_mean
    s2 = gp.zeta_var
    W = Kinv[None] - (Kinv[None] * s2.t()[:, None, :]) @ Kinv                        # (Do, M, M)
    Wf = W.reshape(W.shape[0], M * M)
    d2 = ((Zs[:, None, :] - Zs[None, :, :]) ** 2).sum(-1)
    eye = torch.eye(D, dtype=torch.float64, device=mean.device)
    outs = []
    for c0 in range(0, mean.shape[0], CHUNK):
        m, S = mean[c0:c0 + CHUNK], cov[c0:c0 + CHUNK]
        St = S / ls[:, None] / ls[None, :]
        r = Zs[None] - (m / ls)[:, None, :]                                          # (C, M, D)
        A1, A2 = eye + St, 0.5 * eye + St
        B1, B2 = torch.linalg.inv(A1), torch.linalg.inv(A2)
        rb1 = r @ B1
        q = v / torch.sqrt(torch.linalg.det(A1))[:, None] * torch.exp(-0.5 * (rb1 * r).sum(-1))
        fm = q @ alpha
        rb2 = r @ B2
        g = (rb2 * r).sum(-1)
        quad = g[:, :, None] + g[:, None, :] + 2.0 * rb2 @ r.transpose(1, 2)
        Q = (v * v / torch.sqrt(torch.linalg.det(2.0 * A2)))[:, None, None] * torch.exp(-0.25 * d2[None] - 0.125 * quad)
        aQa = alpha.t()[None] @ Q @ alpha[None]
        tr = Q.reshape(Q.shape[0], M * M) @ Wf.t()
        fc = aQa - fm[:, :, None] * fm[:, None, :] + torch.diag_embed(v - tr)
        s = (alpha[None] * q[:, :, None]).transpose(1, 2) @ r                        # (C, Do, D)
        xc = (s @ B1 @ St) * ls
        outs.append((fm, fc, xc))
    return [torch.cat(x) for x in zip(*outs)]


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    for M, D, Do, N in SHAPES:
        p, raw = make(M, D, Do, N, 1, 1)
        t = lambda x: torch.tensor(x, dtype=torch.float64, device=DEV)
        gp = gp_tf.GPModel(D, Do, M, 0.4, 1.0, 0.1, 1.0, 0.01, seed=0, device=DEV)
        gp.zeta_pos, gp.zeta_mean, gp.zeta_var_unc, gp.kern.variance_unc, gp.kern.lengthscales_unc = [t(x) for x in p]
        mean = torch.cat([t(raw['m0']), t(raw['a'][0])], 1).contiguous()
        cov = torch.zeros(N, D, D, dtype=torch.float64, device=DEV)
        cov[:, :Do, :Do] = t(raw['P0'])
        keep = {}
        pack = gp._prepared()

        def mm():
            keep['mm'] = gp.moment_match(mean, cov)

        def tl():
            keep['torch'] = torch_closed_form(gp, pack, mean, cov)

        fns = {'mm': mm, 'mm_nocross': lambda: gp.moment_match(mean, cov, cross=False),
               'mm_launch': lambda: ag.gp_moment_match_eval(pack, mean, cov),
               'mm_nocross_launch': lambda: ag.gp_moment_match_eval(pack, mean, cov, cross=False),
               'torch': tl, 'lin': lambda: gp.linearize(mean), 'lin_launch': lambda: ag.gp_linearize_eval(pack, mean)}
        for _ in range(2):
            for f in fns.values():
                f()
        torch.cuda.synchronize()
        assert int(keep['mm'][3].abs().sum()) == 0
        err = [float(((x - z).abs().max() / z.abs().max()).cpu()) for x, z in zip(keep['mm'][:3], keep['torch'])]
        res = {k: [] for k in fns}
        for _ in range(rounds):
            for k, f in fns.items():
                res[k].append(timed(f))
        med = {k: float(np.median(v)) for k, v in res.items()}
        print(json.dumps({'shape': [M, D, Do, N], 'rounds': rounds, 'form': gp._pack.gp_form(), 'chunk': CHUNK, 'ms_median': med,
                          'ms_min': {k: float(np.min(v)) for k, v in res.items()},
                          'ms_max': {k: float(np.max(v)) for k, v in res.items()},
                          'torch_over_mm': med['torch'] / med['mm'], 'torch_over_mm_launch': med['torch'] / med['mm_launch'],
                          'mm_over_lin': med['mm'] / med['lin'], 'mm_launch_over_lin_launch': med['mm_launch'] / med['lin_launch'],
                          'max_rel_diff_fmean_fcov_xcov_vs_torch': err}), flush=True)


if __name__ == '__main__':
    main()
