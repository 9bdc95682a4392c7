"""Shared by the Voliro-ELBO tests: the complete loss of the reference's Voliro model (cbfssm/model/voliro.py:21-32,
88-291) restated in float64 torch on the CPU over the oracle's GPModel (gp_autograd_cases.oracle_model), the rollout
recurrence of gp_rollout_cases and the filter restatement of rigid_filter_cases; reverse-mode autodiff gives the
reference gradients of all 13 leaves.

Cases (B, samples, T, M).  Inputs, from default_rng(5 + B + 10 T) in this order: pwm U(0.3, 1) (B, T, 6), tilt
U(-0.5, 0.5) (B, T, 6); sample_in = (pwm, tilt, 0.01 t).  One random unit quaternion per sequence; sample_out (B, T, 16):
N(0, 1) everywhere, columns 12:16 = that base + 0.05 N.  Noise: 'gp' (B, T, S), 'b' (T, N), 'f' (T-1, N) standard
normals.  Config: run/run_voliro.py with ind_pnt_num = M and loglik_factor = [20, 0.3, 200] (the entropy path carries
weight).  Parameters ("perturbed"): gp_f from gp_autograd_cases.make_inputs(M, 12, 3, 1); gp_b from
gp_autograd_cases.make_inputs(M, 19, 6, 1) with its inducing inputs and lengthscales moved to where gp_b's inputs
(h, force/torque, observation) lie -- the rotor forces are of order 100 N, and with inducing points in [-2, 2]^19 every
kernel value underflows to zero and gp_b's gradients vanish identically; the noise variances are the config's times
exp(U(-0.3, 0.3)).

Rules as tests/gp_rollout_cases.py: scalars 1e-9 relative, pred_mean / pred_var within 1e-8 of their largest entry,
every gradient entry within 1e-6 of its tensor's largest entry."""
import functools
import math

import numpy as np
import torch

import gp_autograd_cases as gc
import gp_rollout_cases as roll
import rigid_filter_cases as rf
from gp_autograd_cases import PARAMS, within_rule             # noqa: F401
from gp_rollout_cases import traj_rule                        # noqa: F401
from rigid_filter_cases import scalar_rule                    # noqa: F401

CASES = [(3, 7, 6, 20), (5, 16, 4, 20)]
TERMS = ('loglik', 'kl_x', 'entropy', 'n_reg', 'l_reg', 'kl_z_f', 'kl_z_b')
LEAVES = tuple('gp_f.' + k for k in PARAMS) + tuple('gp_b.' + k for k in PARAMS) + ('var_x_unc', 'var_y_unc', 'var_z_unc')
# centre and spread of gp_b's 19 inputs: h (6), force (3), torque (3), position (3), quaternion (4)
B_CENTRE = np.asarray([0.0] * 6 + [0.0, 0.0, -95.0] + [0.0] * 3 + [0.0] * 7)
B_SPREAD = np.asarray([1.0] * 6 + [15.0, 15.0, 30.0] + [8.0] * 3 + [1.0] * 7)


def config(M, samples):
    sd = np.asarray([0.02] * 7 + [0.2] * 6)
    return {'batch_size': 16, 'ind_pnt_num': M, 'samples': samples, 'learning_rate': 0.01,
            'loglik_factor': np.asarray([20.0, 0.3, 200.0]), 'n_beta': [10.0, 2.0, 10.0], 'l_beta': [1.0, 10.0, 10.0],
            'zeta_pos': 2.0, 'zeta_mean': 0.05 ** 2, 'zeta_var': 0.01 ** 2, 'gp_var': 0.5 ** 2, 'gp_len': 5.0,
            'var_x': sd ** 2, 'var_y': sd ** 2, 'var_z': np.asarray([0.02] * 6)}


def make_case(case):
    """(config, dict of the 13 leaf arrays by LEAVES name, sample_in, sample_out, noise dict) as numpy"""
    B, S, T, M = case
    cfg = config(M, S)
    rng = np.random.default_rng(5 + B + 10 * T)
    pwm = rng.uniform(0.3, 1.0, (B, T, 6))
    tilt = rng.uniform(-0.5, 0.5, (B, T, 6))
    sample_in = np.concatenate([pwm, tilt, np.broadcast_to(0.01 * np.arange(T)[None, :, None], (B, T, 1))], -1)
    base = rng.standard_normal((B, 1, 4))
    base /= np.linalg.norm(base, axis=-1, keepdims=True)
    sample_out = rng.standard_normal((B, T, 16))
    sample_out[..., 12:16] = base + 0.05 * rng.standard_normal((B, T, 4))
    N = B * S
    noise = {'gp': rng.standard_normal((B, T, S)), 'b': rng.standard_normal((T, N)), 'f': rng.standard_normal((T - 1, N))}
    pf, _, _, _ = gc.make_inputs(M, 12, 3, 1)
    pb, _, _, _ = gc.make_inputs(M, 19, 6, 1)
    pb = dict(pb)
    pb['zeta_pos'] = B_CENTRE + B_SPREAD * pb['zeta_pos']
    ls = np.log1p(np.exp(pb['lengthscales_unc'])) + 1e-10
    pb['lengthscales_unc'] = gc.softplus_inverse(ls * B_SPREAD)
    leaves = {'gp_f.' + k: pf[k] for k in PARAMS}
    leaves.update({'gp_b.' + k: pb[k] for k in PARAMS})
    for k in ('var_x', 'var_y', 'var_z'):
        v = np.asarray(cfg[k], dtype=np.float64)
        leaves[k + '_unc'] = gc.softplus_inverse(v * np.exp(rng.uniform(-0.3, 0.3, v.shape)))
    return cfg, leaves, sample_in, sample_out, noise


def alloc_matrix():
    """voliro.py:295-312"""
    angles = np.asarray([0.5, -0.5, -1. / 6., 5. / 6., 1. / 6., 7. / 6.]) * math.pi
    arm_length = 0.3
    a = np.zeros((6, 12))
    for i in range(6):
        a[0, 2 * i] = -math.cos(angles[i])
        a[1, 2 * i] = -math.sin(angles[i])
        a[2, 2 * i + 1] = -1
        a[3, 2 * i + 1] = -arm_length * math.cos(angles[i])
        a[4, 2 * i + 1] = -arm_length * math.sin(angles[i])
        a[5, 2 * i] = -arm_length
    return a


def out_to_hidden(y):
    return torch.cat((y[..., 0:3], y[..., 12:16]), -1)


def softplus(x):
    return torch.nn.functional.softplus(x, beta=1.0, threshold=1e9) + 1e-10


def loss_cpu(cfg, t, sample_in, sample_out, noise):
    """voliro.py:34-291 on CPU tensors; t: dict of the 13 leaf tensors.  Returns (loss, terms, pred_mean, pred_var)."""
    from oracle import cbfssm_torch_ref as tref
    S = cfg['samples']
    si, so = torch.tensor(sample_in), torch.tensor(sample_out)
    B, T = si.shape[:2]
    N = B * S
    gp_f = tref.GPModel(*[t['gp_f.' + k] for k in PARAMS])
    gp_b = tref.GPModel(*[t['gp_b.' + k] for k in PARAMS])
    var_x, var_y, var_z = softplus(t['var_x_unc']), softplus(t['var_y_unc']), softplus(t['var_z_unc'])
    ts = si[0, :, 12]
    dt = float(ts[-1] - ts[0]) / T                                                           # :44-45
    # :88-104
    pwm, tilt = si[:, :, :6], si[:, :, 6:]
    coo = []
    for k in range(6):
        fac = pwm[..., k] ** 2
        coo.append(torch.sin(tilt[..., k]) * fac)
        coo.append(torch.cos(tilt[..., k]) * fac)
    coo = torch.stack(coo, -1)
    post_scale = 0.000012 * 1700.0 ** 2
    ft = (torch.tensor(alloc_matrix()) @ coo[..., None])[..., 0] * post_scale
    # :106-123
    fmean, fvar = gp_f.predict(coo.reshape(B * T, 12))
    fmean = fmean.reshape(B, T, 3) + ft[..., :3]
    out_mean = torch.cat((fmean, ft[..., 3:]), 2)
    out_var = torch.cat((fvar.reshape(B, T, 3), torch.zeros_like(ft[..., 3:])), 2) + var_z
    eps = torch.tensor(noise['gp'])[..., None]
    ft_gp = out_mean[:, :, None, :] + eps * torch.sqrt(out_var)[:, :, None, :]               # (B, T, S, 6)
    # :125-186
    y_dub = out_to_hidden(so).permute(1, 0, 2)[:, :, None, :].repeat(1, 1, S, 1).reshape(T, N, 7)
    u = ft_gp.permute(1, 0, 2, 3).reshape(T, N, 6)
    y2, entropy = roll.rollout(gp_b.predict, torch.zeros(N, 6, dtype=torch.float64), torch.cat((u, y_dub), 2),
                               torch.tensor(noise['b']), None, True)
    y_tilde = torch.cat((y_dub, y2), 2)
    # :188-242
    bd = rf.body(dt)
    traj, kl_x = rf.rigid_filter(bd, y_tilde[0], u[:-1], y_tilde[1:], torch.tensor(noise['f']), var_x, var_y)
    x_final = torch.cat((y_tilde[0:1], traj), 0)
    # :247-271
    dist = torch.distributions.Independent(torch.distributions.Normal(x_final[..., :7], torch.sqrt(var_y[:7])), 1)
    loglik = dist.log_prob(y_dub).sum()
    kl_z_f, kl_z_b = gp_f.prior_kl(), gp_b.prior_kl()
    nb, lb = cfg['n_beta'], cfg['l_beta']
    dd = torch.float64
    n_reg = torch.distributions.Beta(torch.tensor(nb[0], dtype=dd), torch.tensor(nb[1], dtype=dd)).log_prob(var_z / nb[2]).sum()
    l_reg = torch.distributions.Beta(torch.tensor(lb[0], dtype=dd), torch.tensor(lb[1], dtype=dd)).log_prob(
        gp_f.kern.lengthscales / lb[2]).sum()
    # :273-288
    xs = x_final.reshape(T, B, S, 13).permute(1, 0, 2, 3)
    pred_mean, pred_var = xs.mean(2), xs.var(2, unbiased=False) + var_y
    lf = cfg['loglik_factor']
    div = 1.0 / S
    elbo = (loglik * lf[0] * div - kl_x * lf[0] * div + entropy * lf[1] * div + n_reg * lf[2] + l_reg * lf[2]
            - kl_z_f - kl_z_b)
    terms = {'loglik': loglik, 'kl_x': kl_x, 'entropy': entropy, 'n_reg': n_reg, 'l_reg': l_reg, 'kl_z_f': kl_z_f,
             'kl_z_b': kl_z_b}
    return -elbo, terms, pred_mean, pred_var


def leaf_tensors(leaves):
    return {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in leaves.items()}


@functools.lru_cache(maxsize=None)
def reference(case):
    """dict: loss, the seven terms, pred_mean, pred_var and 'g_' + leaf name; computed once and shared (read-only)"""
    cfg, leaves, si, so, noise = make_case(case)
    t = leaf_tensors(leaves)
    loss, terms, pm, pv = loss_cpu(cfg, t, si, so, noise)
    loss.backward()
    out = {'loss': float(loss.detach()), 'pred_mean': pm.detach().numpy(), 'pred_var': pv.detach().numpy()}
    out.update({k: float(v.detach()) for k, v in terms.items()})
    out.update({'g_' + k: t[k].grad.numpy().copy() for k in LEAVES})
    return out
