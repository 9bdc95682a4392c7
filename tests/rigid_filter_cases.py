"""Shared by the rigid-filter tests: the cases, their inputs, and the reference -- Voliro's forward filter run
(cbfssm/model/voliro.py:188-242,314-338 with cbfssm/utils/quaternions.py) restated in float64 torch on the CPU and
differentiated by reverse-mode autodiff with x0, u, y, var_x and var_y requiring grad:

    q = var_x, r = var_y, k = q / (q + r), sig = (1-k)^2 q + k^2 r
    for t in 0..S-1:  f = symplectic_euler(x, u[t]);  mu = f + k (y[t] - f);  x = mu + eps[t][:, None] sqrt(sig);  traj[t] = x
                      kl += 0.5 sum(log q - log sig + (sig + (mu - f)^2) / q - 1)

Inputs, from default_rng(11 + 7 N + S) in this order: one random unit quaternion per chain (`base`); x0 = (N(0,1) position,
base + 0.05 N, 0.5 N linear velocity, 0.5 N angular velocity); y[t] likewise at every step with the same base; u = (3 N force,
0.3 N torque); eps = N; W = N (S, N, 13).  With a per-chain base the norm of the filtered quaternion stays above 0.9, so
the normalisation is well conditioned (independent quaternions per step would let it fall to 0.25).  Constants of
voliro.py:39-41 with dt = 0.01; var_x = sd^2, var_y = (1.3 sd)^2 with sd = [0.02] * 7 + [0.2] * 6.
The loss of every case is  sum(W o traj) + 0.7 kl.

Measured on the CPU (second_coding below: rot_vec through the rotation matrix of the quaternion, the gain written as
(1-k) f + k y, the KL split into its data and its constant part): at N = 37, S = 8 the two codings agree to 1.4e-15 of the
largest entry on every gradient tensor (the worst is var_x), to 1.6e-16 on the trajectory and to 1.4e-16 relative on
kl, and min |rot| over the trajectory is 0.905: the reference sits eight orders inside the rules.

Rules (those of tests/gp_rollout_cases.py): gradients -- every entry within 1e-6 of the largest entry of its tensor;
trajectories -- within 1e-8 of max |traj|; scalars -- 1e-9 relative."""
import functools

import numpy as np
import torch

from gp_autograd_cases import within_rule            # noqa: F401  (re-exported)
from gp_rollout_cases import traj_rule               # noqa: F401  (re-exported)

KL_WEIGHT = 0.7
MASS_INV = 1.0 / 4.04                                              # voliro.py:39
INERTIA_INV = (1.0 / 0.078359127, 1.0 / 0.081797886, 1.0 / 0.1533554115)   # voliro.py:40
GRAVITY = (0.0, 0.0, 9.81)                                         # voliro.py:41
DT = 0.01
SD = np.asarray([0.02] * 7 + [0.2] * 6)
GRADS = ('x0', 'u', 'y', 'var_x', 'var_y')

# (N, S)
CASES = [
    (1, 1),
    (37, 8),
    (64, 2),        # exactly one workgroup
    (65, 3),        # one lane in the second
    (130, 5),       # three workgroups, a ragged last one
    (320, 4),       # the reference's chain count
]


def body(dt=DT):
    """the constants as a plain dict"""
    return {'mass_inv': MASS_INV, 'inertia_inv': INERTIA_INV, 'gravity': GRAVITY, 'dt': float(dt)}


def make_inputs(N, S):
    """dict of numpy arrays: x0 (N,13), u (S,N,6), y (S,N,13), eps (S,N), var_x, var_y (13), W (S,N,13)"""
    rng = np.random.default_rng(11 + 7 * N + S)
    base = rng.standard_normal((N, 4))
    base /= np.linalg.norm(base, axis=1, keepdims=True)

    def state(lead):
        return np.concatenate([rng.standard_normal(lead + (N, 3)), base + 0.05 * rng.standard_normal(lead + (N, 4)),
                               0.5 * rng.standard_normal(lead + (N, 3)), 0.5 * rng.standard_normal(lead + (N, 3))], -1)
    x0 = state(())
    y = state((S,))
    u = np.concatenate([3.0 * rng.standard_normal((S, N, 3)), 0.3 * rng.standard_normal((S, N, 3))], -1)
    eps = rng.standard_normal((S, N))
    W = rng.standard_normal((S, N, 13))
    return {'x0': x0, 'u': u, 'y': y, 'eps': eps, 'var_x': SD ** 2, 'var_y': (1.3 * SD) ** 2, 'W': W}


# ---- the reference: the operations of voliro.py / quaternions.py in their own order ---------------------------------

def quat_multiply(a, b):
    """quaternions.py:8-13"""
    e0 = a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1] - a[..., 2] * b[..., 2] - a[..., 3] * b[..., 3]
    e1 = a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0] + a[..., 2] * b[..., 3] - a[..., 3] * b[..., 2]
    e2 = a[..., 0] * b[..., 2] - a[..., 1] * b[..., 3] + a[..., 2] * b[..., 0] + a[..., 3] * b[..., 1]
    e3 = a[..., 0] * b[..., 3] + a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1] + a[..., 3] * b[..., 0]
    return torch.stack((e0, e1, e2, e3), -1)


def quat_invert(a):
    return a * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=a.dtype)


def pad_to_quat(v):
    return torch.cat((torch.zeros_like(v[..., 0:1]), v), -1)


def rot_vec(v, q):
    """quaternions.py:37-40"""
    return quat_multiply(quat_multiply(q, pad_to_quat(v)), quat_invert(q))[..., 1:]


def symplectic_euler(x, u, bd):
    """voliro.py:314-338"""
    pos, rot, linvel, angvel = x[..., 0:3], x[..., 3:7], x[..., 7:10], x[..., 10:13]
    inertia_inv = torch.tensor(bd['inertia_inv'], dtype=x.dtype)
    gravity = torch.tensor(bd['gravity'], dtype=x.dtype)
    dt = bd['dt']
    f_glob = rot_vec(u[..., :3], rot)
    t_glob = rot_vec(inertia_inv * u[..., 3:], rot)
    linvel = linvel + (bd['mass_inv'] * f_glob + gravity) * dt
    angvel = angvel + t_glob * dt
    rot_diff = 0.5 * quat_multiply(pad_to_quat(angvel), rot)
    pos = pos + linvel * dt
    rot = rot + rot_diff * dt
    rot = rot / torch.norm(rot, dim=-1, keepdim=True)
    return torch.cat((pos, rot, linvel, angvel), -1)


def rigid_filter(bd, x0, u, y, eps, var_x, var_y, step=symplectic_euler):
    """voliro.py:188-242 on torch tensors (any device); returns (traj (S, N, 13), kl ())"""
    S = eps.shape[0]
    x, kl, rows = x0, 0.0, []
    for t in range(S):
        fmean = step(x, u[t], bd)
        k = var_x / (var_y + var_x)
        mu = fmean + k * (y[t] - fmean)
        sig = (1.0 - k) ** 2 * var_x + k ** 2 * var_y
        x = mu + eps[t][:, None] * torch.sqrt(sig)
        rows.append(x)
        kl = kl + 0.5 * torch.sum(torch.log(var_x) - torch.log(sig) + (sig + (mu - fmean) ** 2) / var_x - 1.0)
    return torch.stack(rows), kl


# ---- a second coding of the same function, in another operation order (checks the reference against itself) ----------

def _rotmat_step(x, u, bd):
    a, b, c, d = x[..., 3], x[..., 4], x[..., 5], x[..., 6]
    R = torch.stack([torch.stack([a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)], -1),
                     torch.stack([2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)], -1),
                     torch.stack([2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d], -1)], -2)
    iinv = torch.tensor(bd['inertia_inv'], dtype=x.dtype)
    g = torch.tensor(bd['gravity'], dtype=x.dtype)
    dt = bd['dt']
    fg = (R @ u[..., :3, None])[..., 0]
    tg = (R @ (iinv * u[..., 3:])[..., None])[..., 0]
    v = x[..., 7:10] + dt * g + (dt * bd['mass_inv']) * fg
    w = x[..., 10:13] + dt * tg
    r = x[..., 3:7]
    wx, wy, wz = w[..., 0], w[..., 1], w[..., 2]
    e = torch.stack([-wx * b - wy * c - wz * d, wx * a + wy * d - wz * c, -wx * d + wy * a + wz * b,
                     wx * c - wy * b + wz * a], -1)
    q = r + (0.5 * dt) * e
    q = q * torch.rsqrt((q * q).sum(-1, keepdim=True))
    return torch.cat((x[..., 0:3] + dt * v, q, v, w), -1)


def second_coding(bd, x0, u, y, eps, var_x, var_y):
    S, N = eps.shape
    k = var_x / (var_x + var_y)
    sig = (1 - k) * (1 - k) * var_x + k * k * var_y
    sd = torch.sqrt(sig)
    x, rows, data = x0, [], 0.0
    for t in range(S):
        f = _rotmat_step(x, u[t], bd)
        data = data + (((y[t] - f) ** 2).sum(0) * (k * k / var_x)).sum()
        x = (1 - k) * f + k * y[t] + eps[t][:, None] * sd
        rows.append(x)
    kl = 0.5 * data + S * N * 0.5 * (torch.log(var_x / sig) + sig / var_x - 1.0).sum()
    return torch.stack(rows), kl


def evaluate(case, coding=rigid_filter):
    """dict: traj, kl, loss and the gradients 'g_' + name (GRADS) of the case's loss"""
    inp = make_inputs(*case)
    lv = {k: torch.tensor(inp[k], requires_grad=True) for k in GRADS}
    traj, kl = coding(body(), lv['x0'], lv['u'], lv['y'], torch.tensor(inp['eps']), lv['var_x'], lv['var_y'])
    loss = (torch.tensor(inp['W']) * traj).sum() + KL_WEIGHT * kl
    loss.backward()
    out = {'traj': traj.detach().numpy(), 'kl': float(kl.detach()), 'loss': float(loss.detach())}
    for k in GRADS:
        out['g_' + k] = lv[k].grad.numpy().copy()
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    """computed once per case and shared (treat as read-only)"""
    return evaluate(case)


def scalar_rule(name, x, r, tol=1e-9):
    err = abs(float(x) - float(r)) / abs(float(r))
    print('%-34s ref %.6e  rel err %.2e' % (name, float(r), err))
    assert np.isfinite(float(x)) and err < tol, (name, err)
    return err
