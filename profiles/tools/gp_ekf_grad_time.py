"""GPModel.ekf(differentiable=True), forward under grad plus backward, against the evaluation alone and against the only way
to these gradients before it: the tensor library.

    python profiles/tools/gp_ekf_grad_time.py [rounds] [torch_chains]

Per shape (M, D, Do, N, T, Dy) of gp_ekf_time.SHAPES, float64: HIP events around one call, the measurements alternating over
`rounds` (default 5) after two warm-up calls each; the median is reported.

    ekf        GPModel.ekf on the inputs                                       prepare, pre-kernel, filter kernel
    fwd_grad   GPModel.ekf(differentiable=True) with every leaf and input requiring grad: the forward alone
               (prepare, pack copy, pre-kernel, filter kernel that also stores m-, P-, A P and J)
    grad       the same followed by backward() of sum(loglik) + sum(means) + sum(covs): the adjoint launch, the slab
               reduction and the parameter tail, gradients of all eleven tensors
    torch      the same loss and gradients from tensor-library ops on the same device: predict through a Cholesky factor
               and two triangular solves, J by torch.autograd.grad(create_graph=True) per output dimension, the Dy scalar
               updates chosen by torch.where, then backward() -- on the first `torch_chains` chains (default: all N)

The gradients of `grad` are compared with `torch`'s on those chains' inputs.  Prints one JSON line per shape."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'cbf-ssm_amd'), os.path.dirname(os.path.abspath(__file__))]

import numpy as np
import torch

from cbfssm.model import gp_tf
from gp_ekf_time import SHAPES, DEV, make, timed

JITTER = 1e-8
NAMES = ('m0', 'P0', 'a', 'y', 'var_x', 'var_y')


def softplus(x):
    return torch.nn.functional.softplus(x) + 1e-10


def torch_predict(params):
    """GPModel.predict (diagonal q(z)) in tensor-library ops on the parameters' device"""
    zp, zm, zvu, varu, lsu = params
    ls, var, s2 = softplus(lsu), softplus(varu), softplus(zvu)
    Zs = zp / ls
    M = zp.shape[0]

    def rbf(A, B):
        d2 = (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * A @ B.T
        return var * torch.exp(-0.5 * d2.clamp_min(0.0))

    L = torch.linalg.cholesky(rbf(Zs, Zs) + JITTER * torch.eye(M, dtype=torch.float64, device=zp.device))

    def predict(X):
        k = rbf(Zs, X / ls)
        A = torch.linalg.solve_triangular(L, k, upper=False)
        A2 = torch.linalg.solve_triangular(L.T, A, upper=True)
        return A2.T @ zm, (var - (A * A).sum(0))[:, None] + (A2 * A2).T @ s2
    return predict


def torch_ekf(predict, m0, P0, a, y, var_x, var_y, cond, Do, Dy):
    m = m0
    P = torch.tril(P0) + torch.tril(P0, -1).transpose(1, 2)
    eye = torch.eye(Do, dtype=torch.float64, device=m0.device)
    ll = torch.zeros(m0.shape[0], dtype=torch.float64, device=m0.device)
    means, covs = [], []
    for t in range(y.shape[0]):
        X = torch.cat([m, a[t]], 1)
        fmean, fvar = predict(X)
        J = torch.stack([torch.autograd.grad(fmean[:, d].sum(), X, create_graph=True)[0][:, :Do] for d in range(Do)], 1)
        A = eye[None] + J
        m = m + fmean
        P = A @ P @ A.transpose(1, 2) + torch.diag_embed(fvar + var_x)
        on = cond[t] != 0
        mc, Pc, lc = m, P, ll
        for j in range(Dy):
            s = Pc[:, j, j] + var_y[j]
            dl = y[t, :, j] - mc[:, j]
            g = Pc[:, :, j] / s[:, None]
            mc = mc + g * dl[:, None]
            Pc = Pc - s[:, None, None] * g[:, :, None] * g[:, None, :]
            lc = lc - 0.5 * (torch.log(2.0 * np.pi * s) + dl * dl / s)
        m, P, ll = torch.where(on[:, None], mc, m), torch.where(on[:, None, None], Pc, P), torch.where(on, lc, ll)
        means.append(m)
        covs.append(P)
    return torch.stack(means), torch.stack(covs), ll


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    for M, D, Do, N, T, Dy in SHAPES:
        nt = min(N, int(sys.argv[2])) if len(sys.argv) > 2 else N
        p, raw = make(M, D, Do, N, T, Dy)
        t = lambda x: torch.tensor(x, dtype=torch.float64, device=DEV)
        gp = gp_tf.GPModel(D, Do, M, 0.4, 1.0, 0.1, 1.0, 0.01, seed=0, device=DEV)
        gp.zeta_pos, gp.zeta_mean, gp.zeta_var_unc, gp.kern.variance_unc, gp.kern.lengthscales_unc = [t(x) for x in p]
        plain = gp_tf.GPModel(D, Do, M, 0.4, 1.0, 0.1, 1.0, 0.01, seed=0, device=DEV)
        plain.zeta_pos, plain.zeta_mean, plain.zeta_var_unc, plain.kern.variance_unc, plain.kern.lengthscales_unc = \
            [t(x) for x in p]
        for q in gp.parameters():
            q.requires_grad_()
        i = {k: t(v) for k, v in raw.items()}
        leaves = {k: i[k].clone().requires_grad_() for k in NAMES}
        args = [leaves[k] for k in NAMES]
        eval_args = [i[k] for k in NAMES]
        keep = {}

        def clear():
            for q in list(gp.parameters()) + args:
                q.grad = None

        def grad():
            clear()
            means, covs, ll = gp.ekf(*args, cond=i['cond'], differentiable=True)
            (ll.sum() + means.sum() + covs.sum()).backward()

        def grad_few(n):
            """the library's gradients on the first n chains, for the comparison with the tensor library"""
            sub = {k: (i[k][:n] if k in ('m0', 'P0') else i[k][:, :n] if k in ('a', 'y') else i[k]).clone().requires_grad_()
                   for k in NAMES}
            clear()
            means, covs, ll = gp.ekf(*[sub[k] for k in NAMES], cond=i['cond'][:, :n], differentiable=True)
            (ll.sum() + means.sum() + covs.sum()).backward()
            return [sub[k].grad.clone() for k in NAMES] + [q.grad.clone() for q in gp.parameters()]

        def torch_way():
            sub = {k: (i[k][:nt] if k in ('m0', 'P0') else i[k][:, :nt] if k in ('a', 'y') else i[k]).clone().requires_grad_()
                   for k in NAMES}
            params = [t(x).requires_grad_() for x in p]
            means, covs, ll = torch_ekf(torch_predict(params), *[sub[k] for k in NAMES], i['cond'][:, :nt], Do, Dy)
            (ll.sum() + means.sum() + covs.sum()).backward()
            keep['torch'] = [sub[k].grad for k in NAMES] + [q.grad for q in params]

        fns = {'ekf': lambda: plain.ekf(*eval_args, cond=i['cond']),
               'fwd_grad': lambda: gp.ekf(*args, cond=i['cond'], differentiable=True), 'grad': grad, 'torch': torch_way}
        for _ in range(2):
            for f in fns.values():
                f()
        torch.cuda.synchronize()
        err = [float(((x - z).abs().max() / z.abs().max()).cpu()) for x, z in zip(grad_few(nt), keep['torch'])]
        res = {k: [] for k in fns}
        for _ in range(rounds):
            for k, f in fns.items():
                res[k].append(timed(f))
        med = {k: float(np.median(v)) for k, v in res.items()}
        print(json.dumps({'shape': [M, D, Do, N, T, Dy], 'rounds': rounds, 'form': gp._pack.gp_form(), 'torch_chains': nt,
                          'ms_median': med, 'ms_min': {k: float(np.min(v)) for k, v in res.items()},
                          'ms_max': {k: float(np.max(v)) for k, v in res.items()},
                          'grad_over_ekf': med['grad'] / med['ekf'], 'fwd_grad_over_ekf': med['fwd_grad'] / med['ekf'],
                          'torch_over_grad_per_chain': (med['torch'] / nt) / (med['grad'] / N),
                          'max_rel_diff_of_the_eleven_gradients_vs_torch': err}), flush=True)


if __name__ == '__main__':
    main()
