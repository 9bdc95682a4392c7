"""Voliro's filter loop and the whole Voliro loss on the HIP kernels against the same functions in tensor-library ops under
torch autograd, on the same GPU, float64.

    python profiles/tools/rigid_filter_time.py [rounds] [warmups]

(a) the filter alone: cbfssm.hip.autograd.rigid_filter, forward under grad plus the full backward into x0, u, y, var_x, var_y,
    against the restatement below (a Python loop of tensor ops per step, voliro.py:188-242,314-338);
(b) the whole loss: cbfssm.hip.voliro.VoliroElbo.loss plus backward into its 13 leaves, against the same loss with the
    recognition run as a Python loop of one gp_predict per step and the filter run as the restatement -- what the library
    offered before the fused loops.
The reference's own shape: B = 16, samples = 20 (N = 320 chains), T = 64, M = 20.  One call per measurement between two HIP
events, the two sides alternating, `rounds` (5) measurements after `warmups` (2) calls each; the median is reported.
Prints one JSON line per comparison."""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'cbf-ssm_amd')]

import numpy as np
import torch

from cbfssm.hip import autograd, voliro
from cbfssm.hip import lib as _l

DEV = 'cuda:0'
B, SAMPLES, T, M = 16, 20, 64, 20
LOG2PIE = float(np.log(2.0 * np.pi * np.e))


# ---- the tensor-op restatement (the yardstick) -----------------------------------------------------------------------

def qmul(a, b):
    return torch.stack((a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1] - a[..., 2] * b[..., 2] - a[..., 3] * b[..., 3],
                        a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0] + a[..., 2] * b[..., 3] - a[..., 3] * b[..., 2],
                        a[..., 0] * b[..., 2] - a[..., 1] * b[..., 3] + a[..., 2] * b[..., 0] + a[..., 3] * b[..., 1],
                        a[..., 0] * b[..., 3] + a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1] + a[..., 3] * b[..., 0]), -1)


def pad(v):
    return torch.cat((torch.zeros_like(v[..., 0:1]), v), -1)


def rot_vec(v, q, conj):
    return qmul(qmul(q, pad(v)), q * conj)[..., 1:]


def torch_filter(c, x0, u, y, eps, var_x, var_y):
    """voliro.py:188-242,314-338 in tensor ops; c: dict of device constants"""
    x, kl, rows = x0, 0.0, []
    for t in range(eps.shape[0]):
        pos, rot, linvel, angvel = x[:, 0:3], x[:, 3:7], x[:, 7:10], x[:, 10:13]
        f_glob = rot_vec(u[t][:, :3], rot, c['conj'])
        t_glob = rot_vec(c['inertia_inv'] * u[t][:, 3:], rot, c['conj'])
        linvel = linvel + (c['mass_inv'] * f_glob + c['gravity']) * c['dt']
        angvel = angvel + t_glob * c['dt']
        rot_diff = 0.5 * qmul(pad(angvel), rot)
        pos = pos + linvel * c['dt']
        rot = rot + rot_diff * c['dt']
        rot = rot / torch.norm(rot, dim=-1, keepdim=True)
        fmean = torch.cat((pos, rot, linvel, angvel), -1)
        k = var_x / (var_y + var_x)
        mu = fmean + k * (y[t] - fmean)
        sig = (1.0 - k) ** 2 * var_x + k ** 2 * var_y
        x = mu + eps[t][:, None] * torch.sqrt(sig)
        rows.append(x)
        kl = kl + 0.5 * torch.sum(torch.log(var_x) - torch.log(sig) + (sig + (mu - fmean) ** 2) / var_x - 1.0)
    return torch.stack(rows), kl


def loop_rollout_reverse(gp, h0, a, eps):
    """voliro.py:139-186 as the library offered it before the fused rollout: one gp_predict per step"""
    h, ent = h0, 0.0
    rows = [None] * eps.shape[0]
    for t in range(eps.shape[0] - 1, -1, -1):
        fmean, fvar = autograd.gp_predict(gp._pack, torch.cat([h, a[t]], 1), *gp.parameters())
        h = h + fmean + eps[t][:, None] * torch.sqrt(fvar)
        rows[t] = h
        ent = ent + 0.5 * torch.sum(LOG2PIE + torch.log(fvar))
    return torch.stack(rows), ent


class LoopGP:
    """a GPModel whose rollout is the Python loop"""

    def __init__(self, gp):
        self.gp, self.kern = gp, gp.kern

    def predict(self, X):
        return self.gp.predict(X)

    def prior_kl(self):
        return self.gp.prior_kl()

    def rollout(self, h0, a, eps, var_add=None, reverse=False):
        assert var_add is None and reverse
        return loop_rollout_reverse(self.gp, h0, a, eps)


# ---- inputs ----------------------------------------------------------------------------------------------------------

def dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64, device=DEV)


def filter_inputs(N, S, rng):
    base = rng.standard_normal((N, 4))
    base /= np.linalg.norm(base, axis=1, keepdims=True)

    def state(lead):
        return np.concatenate([rng.standard_normal(lead + (N, 3)), base + 0.05 * rng.standard_normal(lead + (N, 4)),
                               0.5 * rng.standard_normal(lead + (N, 3)), 0.5 * rng.standard_normal(lead + (N, 3))], -1)
    sd = np.asarray([0.02] * 7 + [0.2] * 6)
    u = np.concatenate([3.0 * rng.standard_normal((S, N, 3)), 0.3 * rng.standard_normal((S, N, 3))], -1)
    return {'x0': state(()), 'u': u, 'y': state((S,)), 'eps': rng.standard_normal((S, N)), 'var_x': sd ** 2,
            'var_y': (1.3 * sd) ** 2, 'W': rng.standard_normal((S, N, 13))}


def voliro_config():
    sd = np.asarray([0.02] * 7 + [0.2] * 6)
    return {'ind_pnt_num': M, 'samples': SAMPLES, 'loglik_factor': np.asarray([20.0, 0.0, 200.0]), 'n_beta': [10.0, 2.0, 10.0],
            'l_beta': [1.0, 10.0, 10.0], 'zeta_pos': 2.0, 'zeta_mean': 0.05 ** 2, 'zeta_var': 0.01 ** 2, 'gp_var': 0.5 ** 2,
            'gp_len': 5.0, 'var_x': sd ** 2, 'var_y': sd ** 2, 'var_z': np.asarray([0.02] * 6)}


def voliro_inputs(rng):
    pwm, tilt = rng.uniform(0.3, 1.0, (B, T, 6)), rng.uniform(-0.5, 0.5, (B, T, 6))
    si = np.concatenate([pwm, tilt, np.broadcast_to(0.01 * np.arange(T)[None, :, None], (B, T, 1))], -1)
    base = rng.standard_normal((B, 1, 4))
    base /= np.linalg.norm(base, axis=-1, keepdims=True)
    so = rng.standard_normal((B, T, 16))
    so[..., 12:16] = base + 0.05 * rng.standard_normal((B, T, 4))
    N = B * SAMPLES
    noise = {'gp': rng.standard_normal((B, T, SAMPLES)), 'b': rng.standard_normal((T, N)), 'f': rng.standard_normal((T - 1, N))}
    return dev(si), dev(so), {k: dev(v) for k, v in noise.items()}


# ---- timing ----------------------------------------------------------------------------------------------------------

def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def compare(name, hip, ref, rounds, warm, extra):
    for _ in range(warm):
        hip(); ref()
    torch.cuda.synchronize()
    res = {'hip': [], 'torch': []}
    for _ in range(rounds):
        res['hip'].append(timed(hip))
        res['torch'].append(timed(ref))
    med = {k: float(np.median(v)) for k, v in res.items()}
    out = {'what': name, 'B': B, 'samples': SAMPLES, 'T': T, 'M': M, 'rounds': rounds, 'warmups': warm, 'ms_median': med,
           'ms_min': {k: float(np.min(v)) for k, v in res.items()}, 'ms_max': {k: float(np.max(v)) for k, v in res.items()},
           'torch_over_hip': med['torch'] / med['hip']}
    out.update(extra())
    print(json.dumps(out), flush=True)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    warm = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    rng = np.random.default_rng(0)
    N, S = B * SAMPLES, T - 1
    dt = 0.01
    # (a) the filter alone
    inp = filter_inputs(N, S, rng)
    lv = [dev(inp[k]).requires_grad_() for k in ('x0', 'u', 'y', 'var_x', 'var_y')]
    eps, W = dev(inp['eps']), dev(inp['W'])
    body = _l.rigid_body(voliro.MASS_INV, voliro.INERTIA_INV, voliro.GRAVITY, dt)
    c = {'mass_inv': voliro.MASS_INV, 'inertia_inv': dev(voliro.INERTIA_INV), 'gravity': dev(voliro.GRAVITY), 'dt': dt,
         'conj': dev([1.0, -1.0, -1.0, -1.0])}
    keep = {}

    def hip_a():
        traj, kl = autograd.rigid_filter(body, lv[0], lv[1], lv[2], eps, lv[3], lv[4])
        keep['h'] = torch.autograd.grad((W * traj).sum() + 0.7 * kl, lv)

    def ref_a():
        traj, kl = torch_filter(c, lv[0], lv[1], lv[2], eps, lv[3], lv[4])
        keep['t'] = torch.autograd.grad((W * traj).sum() + 0.7 * kl, lv)

    def err_a():
        return {'grad_max_rel_diff': max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(keep['h'], keep['t']))}
    compare('filter: forward under grad + backward', hip_a, ref_a, rounds, warm, err_a)

    # (b) the whole loss
    cfg = voliro_config()
    si, so, noise = voliro_inputs(rng)
    eng = voliro.VoliroElbo(cfg, DEV, seed=0).requires_grad_()
    leaves = eng.parameters()
    other = voliro.VoliroElbo(cfg, DEV, seed=0)
    other.gp_f, other.gp_b = eng.gp_f, LoopGP(eng.gp_b)
    other.var_x_unc, other.var_y_unc, other.var_z_unc = eng.var_x_unc, eng.var_y_unc, eng.var_z_unc
    dtv = 0.01 * (T - 1) / T

    def hip_b():
        loss, _ = eng.loss(si, so, noise, dt=dtv)
        keep['h'] = (loss.detach(),) + torch.autograd.grad(loss, leaves)

    def ref_b():
        saved = autograd.rigid_filter
        autograd.rigid_filter = lambda bd, x0, u, y, e, vx, vy: torch_filter(
            {'mass_inv': bd.mass_inv, 'inertia_inv': c['inertia_inv'], 'gravity': c['gravity'], 'dt': bd.dt, 'conj': c['conj']},
            x0, u, y, e, vx, vy)
        try:
            loss, _ = other.loss(si, so, noise, dt=dtv)
        finally:
            autograd.rigid_filter = saved
        keep['t'] = (loss.detach(),) + torch.autograd.grad(loss, leaves)

    def err_b():
        return {'loss_rel_diff': float((keep['h'][0] - keep['t'][0]).abs() / keep['t'][0].abs()),
                'grad_max_rel_diff': max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(keep['h'][1:], keep['t'][1:]))}
    compare('VoliroElbo.loss + backward into 13 leaves', hip_b, ref_b, rounds, warm, err_b)


if __name__ == '__main__':
    main()
