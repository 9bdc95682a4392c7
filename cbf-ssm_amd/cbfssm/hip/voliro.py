"""The ELBO of the reference's Voliro model (cbfssm/model/voliro.py:21-32,244-291) as one differentiable function on the
HIP kernels.  Nothing here runs a Python time loop: the three loops of the model are three launches,

    gp_f.predict over all B T points plus the physics term            voliro.py:88-123   cbfssm.hip.autograd.gp_predict
    the recognition run of gp_b, backwards in time from h = 0         voliro.py:139-186  cbfssm.hip.autograd.gp_rollout
    the rigid-body filter run against y_tilde                         voliro.py:188-242  cbfssm.hip.autograd.rigid_filter

each with a hand-written adjoint; the glue between them (sampling the force/torque, concatenations, the log-likelihood,
the two Beta priors, the combination) is a handful of tensor-library ops over whole arrays.

    elbo = VoliroElbo(config, 'cuda:0')
    loss, terms = elbo.loss(sample_in, sample_out, noise)
    loss.backward()                       # reaches all 13 leaves of elbo.parameters()
    pred_mean, pred_var = elbo.predict_moments()

This is the loss alone.  The model class with its session plumbing (`cbfssm.model.Voliro`), the dataset and the plots are
not part of it."""
import math

import numpy as np
import torch

from . import autograd as _ag
from . import lib as _l
from .ops import tf_forward
from ..synthetic import softplus_inverse

ROTOR_FORCE_CONSTANT = 0.000012                                        # voliro.py:37
ROTOR_SPEED_MAX = 1700.0                                               # voliro.py:38
POST_SCALE = ROTOR_FORCE_CONSTANT * ROTOR_SPEED_MAX ** 2               # voliro.py:42
MASS_INV = 1.0 / 4.04                                                  # voliro.py:39
INERTIA_INV = (1.0 / 0.078359127, 1.0 / 0.081797886, 1.0 / 0.1533554115)   # voliro.py:40
GRAVITY = (0.0, 0.0, 9.81)                                             # voliro.py:41
TERMS = ('loglik', 'kl_x', 'entropy', 'n_reg', 'l_reg', 'kl_z_f', 'kl_z_b')
# the order of VoliroElbo.parameters(): the five leaves of gp_f, the five of gp_b (each in the order of
# cbfssm.hip.autograd.GP_PARAM_NAMES), then the three noise leaves
PARAM_NAMES = tuple('gp_f.' + k for k in _ag.GP_PARAM_NAMES) + tuple('gp_b.' + k for k in _ag.GP_PARAM_NAMES) + \
    ('var_x_unc', 'var_y_unc', 'var_z_unc')


def alloc_matrix():
    """the (6, 12) allocation matrix of the tilt-rotor hexacopter (voliro.py:295-312), numpy"""
    angles = np.asarray([0.5, -0.5, -1.0 / 6.0, 5.0 / 6.0, 1.0 / 6.0, 7.0 / 6.0]) * math.pi
    arm = 0.3
    a = np.zeros((6, 12))
    for i in range(6):
        a[0, 2 * i] = -math.cos(angles[i])
        a[1, 2 * i] = -math.sin(angles[i])
        a[2, 2 * i + 1] = -1.0
        a[3, 2 * i + 1] = -arm * math.cos(angles[i])
        a[4, 2 * i + 1] = -arm * math.sin(angles[i])
        a[5, 2 * i] = -arm
    return a


def local_coord(sample_in):
    """(..., 13) inputs (pwm 0:6, tilt 6:12, time 12) -> (..., 12): sin(tilt_k) pwm_k^2, cos(tilt_k) pwm_k^2 (voliro.py:88-95)"""
    fac = sample_in[..., 0:6] ** 2
    tilt = sample_in[..., 6:12]
    return torch.stack((torch.sin(tilt) * fac, torch.cos(tilt) * fac), dim=-1).reshape(sample_in.shape[:-1] + (12,))


def force_torque(local_coo):
    """(..., 12) -> (..., 6): the physics model's force and torque (voliro.py:97-104)"""
    a = torch.as_tensor(alloc_matrix(), dtype=local_coo.dtype, device=local_coo.device)
    return (local_coo @ a.T) * POST_SCALE


def out_to_hidden(y):
    """(..., 16) outputs -> (..., 7): position and orientation (voliro.py:340-343)"""
    return torch.cat((y[..., 0:3], y[..., 12:16]), dim=-1)


def _beta_log_prob(x, alpha, beta):
    lbeta = math.lgamma(alpha) + math.lgamma(beta) - math.lgamma(alpha + beta)
    return (alpha - 1.0) * torch.log(x) + (beta - 1.0) * torch.log1p(-x) - lbeta


class VoliroElbo:
    """Holds gp_f (12 -> 3) and gp_b (19 -> 6), both cbfssm.model.gp_tf.GPModel with config['ind_pnt_num'] points, and
    the leaves var_x_unc (13), var_y_unc (13), var_z_unc (6) (voliro.py:34-72; initial values through the softplus
    inverse of the other models).  parameters() returns the 13 leaves in the order of PARAM_NAMES."""

    def __init__(self, config, device, seed=None):
        from ..model import gp_tf
        self.config = config
        self.device = torch.device(device)
        self.samples = int(config['samples'])
        gp = dict(num_points=config['ind_pnt_num'], gp_var=config['gp_var'], gp_len=config['gp_len'],
                  zeta_mean=config['zeta_mean'], zeta_pos=config['zeta_pos'], zeta_var=config['zeta_var'], device=self.device)
        self.gp_f = gp_tf.GPModel(in_dim=12, out_dim=3, seed=seed, **gp)
        self.gp_b = gp_tf.GPModel(in_dim=19, out_dim=6, seed=None if seed is None else seed + 1, **gp)

        def leaf(v, n):
            return torch.tensor(np.broadcast_to(softplus_inverse(v), (n,)).copy(), dtype=torch.float64, device=self.device)
        self.var_x_unc = leaf(config['var_x'], 13)
        self.var_y_unc = leaf(config['var_y'], 13)
        self.var_z_unc = leaf(config['var_z'], 6)
        self._moments = None

    def parameters(self):
        """The 13 trainable leaves in the order of PARAM_NAMES."""
        return self.gp_f.parameters() + self.gp_b.parameters() + [self.var_x_unc, self.var_y_unc, self.var_z_unc]

    def requires_grad_(self, flag=True):
        for p in self.parameters():
            p.requires_grad_(flag)
        return self

    @staticmethod
    def time_step(sample_in):
        """dt of voliro.py:44-45 from column 12 of the first sequence, as a host float"""
        t = sample_in[0, :, 12]
        return float(t[-1] - t[0]) / t.shape[0]

    @staticmethod
    def noise_from(draw, B, T, S):
        """the three noise arrays from one cbfssm.hip.ops.NoisePipeline(...).next(T, B * S) draw"""
        N = B * S
        return {'gp': draw['hid_b'][:T * N].reshape(B, T, S), 'b': draw['eps_b'][:T * N].reshape(T, N),
                'f': draw['eps_f'].reshape(T - 1, N)}

    def loss(self, sample_in, sample_out, noise, dt=None):
        """sample_in (B, T, 13), sample_out (B, T, 16); noise = {'gp': (B, T, S), 'b': (T, N), 'f': (T-1, N)} standard
        normals with N = B S and chain order n = b S + s.  Returns (loss, terms): the negative ELBO of voliro.py:277-288
        and the dict of its seven terms (TERMS), all 0-d device tensors.  `dt` defaults to time_step(sample_in), which
        reads two numbers of sample_in on the host (pass sample_in as a host array, or dt itself, to avoid the copy)."""
        cfg, S, dev = self.config, self.samples, self.device
        if dt is None:
            dt = self.time_step(sample_in)
        sample_in = torch.as_tensor(sample_in, dtype=torch.float64).to(dev)
        sample_out = torch.as_tensor(sample_out, dtype=torch.float64).to(dev)
        B, T = sample_in.shape[:2]
        N = B * S
        if T < 2:
            raise ValueError('VoliroElbo.loss: at least two time steps')
        e_gp, e_b, e_f = (torch.as_tensor(noise[k], dtype=torch.float64).to(dev) for k in ('gp', 'b', 'f'))
        assert tuple(e_gp.shape) == (B, T, S) and tuple(e_b.shape) == (T, N) and tuple(e_f.shape) == (T - 1, N), \
            "noise: 'gp' (B, T, S), 'b' (T, B S), 'f' (T - 1, B S)"
        var_x, var_y, var_z = tf_forward(self.var_x_unc), tf_forward(self.var_y_unc), tf_forward(self.var_z_unc)

        # gp_f over all B T points plus the physics term, one force/torque sample per particle (voliro.py:88-123)
        coo = local_coord(sample_in)
        ft = force_torque(coo)
        fmean, fvar = self.gp_f.predict(coo.reshape(B * T, 12))
        out_mean = torch.cat((fmean.reshape(B, T, 3) + ft[..., :3], ft[..., 3:]), dim=2)
        out_var = torch.cat((fvar.reshape(B, T, 3), torch.zeros_like(ft[..., 3:])), dim=2) + var_z
        ft_gp = out_mean[:, :, None, :] + e_gp[..., None] * torch.sqrt(out_var)[:, :, None, :]       # (B, T, S, 6)
        u = ft_gp.permute(1, 0, 2, 3).reshape(T, N, 6)

        # recognition run (voliro.py:125-186)
        obs = out_to_hidden(sample_out)                                                              # (B, T, 7)
        y_dub = obs.permute(1, 0, 2)[:, :, None, :].expand(T, B, S, 7).reshape(T, N, 7)
        h0 = torch.zeros(N, 6, dtype=torch.float64, device=dev)
        y2, entropy = self.gp_b.rollout(h0, torch.cat((u, y_dub), dim=2), e_b, None, reverse=True)
        y_tilde = torch.cat((y_dub, y2), dim=2)                                                      # (T, N, 13)

        # filter run (voliro.py:188-242)
        body = _l.rigid_body(MASS_INV, INERTIA_INV, GRAVITY, dt)
        traj, kl_x = _ag.rigid_filter(body, y_tilde[0], u[:-1], y_tilde[1:], e_f, var_x, var_y)
        x_final = torch.cat((y_tilde[0:1], traj), dim=0)                                             # (T, N, 13)

        # likelihood over all T rows (voliro.py:247-255)
        vy = var_y[:7]
        resid = y_dub - x_final[..., :7]
        loglik = -0.5 * torch.sum(resid * resid / vy) - 0.5 * T * N * torch.sum(torch.log(2.0 * math.pi * vy))
        kl_z_f, kl_z_b = self.gp_f.prior_kl(), self.gp_b.prior_kl()
        n_a, n_b, n_s = (float(v) for v in cfg['n_beta'])
        l_a, l_b, l_s = (float(v) for v in cfg['l_beta'])
        n_reg = torch.sum(_beta_log_prob(var_z / n_s, n_a, n_b))                                     # voliro.py:261-265
        l_reg = torch.sum(_beta_log_prob(self.gp_f.kern.lengthscales / l_s, l_a, l_b))               # voliro.py:267-271

        lf = [float(v) for v in cfg['loglik_factor']]
        div = 1.0 / S
        elbo = (loglik * (lf[0] * div) - kl_x * (lf[0] * div) + entropy * (lf[1] * div) + n_reg * lf[2] + l_reg * lf[2]
                - kl_z_f - kl_z_b)                                                                   # voliro.py:277-288
        with torch.no_grad():                                                                        # voliro.py:273-275
            xs = x_final.reshape(T, B, S, 13).permute(1, 0, 2, 3)
            self._moments = (xs.mean(dim=2), xs.var(dim=2, unbiased=False) + var_y)
        terms = {'loglik': loglik, 'kl_x': kl_x, 'entropy': entropy, 'n_reg': n_reg, 'l_reg': l_reg, 'kl_z_f': kl_z_f,
                 'kl_z_b': kl_z_b}
        return -elbo, terms

    def predict_moments(self):
        """(pred_mean, pred_var), each (B, T, 13): mean and variance over the particles of the filtered states of the last
        loss evaluation, the variance plus var_y (voliro.py:273-275)"""
        if self._moments is None:
            raise RuntimeError('VoliroElbo.predict_moments: no loss has been evaluated yet')
        return self._moments
