"""The float64 restatement of Voliro's forward filter run (tests/rigid_filter_cases.py) checked against itself on the CPU:
properties of one rigid-body step, the quaternion conventions, and cbfssm.utils.quaternions against the restatement."""
import numpy as np
import torch

import rigid_filter_cases as rc


def _state(n, seed=0):
    i = rc.make_inputs(n, 1)
    return torch.tensor(i['x0']), torch.tensor(i['u'][0])


def test_quaternion_stays_unit_after_a_step_without_noise():
    x, u = _state(37)
    f = rc.symplectic_euler(x, u, rc.body())
    assert torch.allclose(torch.norm(f[:, 3:7], dim=1), torch.ones(37, dtype=torch.float64), rtol=0, atol=1e-15)
    # and through the filter with zero noise and y = f: the state is f itself
    inp = rc.make_inputs(37, 1)
    traj, _ = rc.rigid_filter(rc.body(), x, u[None], f[None], torch.zeros(1, 37, dtype=torch.float64),
                              torch.tensor(inp['var_x']), torch.tensor(inp['var_y']))
    assert torch.allclose(torch.norm(traj[0, :, 3:7], dim=1), torch.ones(37, dtype=torch.float64), rtol=0, atol=1e-15)


def test_free_step_moves_the_position_by_linvel_dt():
    x, u = _state(21)
    bd = rc.body()
    bd['gravity'] = (0.0, 0.0, 0.0)
    f = rc.symplectic_euler(x, torch.zeros_like(u), bd)
    assert torch.equal(f[:, 7:13], x[:, 7:13])
    assert torch.allclose(f[:, 0:3], x[:, 0:3] + x[:, 7:10] * bd['dt'], rtol=0, atol=1e-16)


def test_rot_vec_conventions():
    v = torch.tensor(np.random.default_rng(1).standard_normal((9, 3)))
    ident = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64).expand(9, 4)
    assert torch.equal(rc.rot_vec(v, ident), v)
    c = np.sqrt(0.5)
    qz = torch.tensor([c, 0.0, 0.0, c], dtype=torch.float64)            # 90 degrees about z
    ex = torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64)
    assert torch.allclose(rc.rot_vec(ex, qz), torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), rtol=0, atol=1e-15)


def test_the_two_codings_agree():
    r1 = rc.reference((37, 8))
    r2 = rc.evaluate((37, 8), rc.second_coding)
    rc.traj_rule('traj', r2['traj'], r1['traj'], tol=1e-13)
    rc.scalar_rule('kl', r2['kl'], r1['kl'], tol=1e-13)
    for k in rc.GRADS:
        rc.within_rule(k, r2['g_' + k], r1['g_' + k], rtol=1e-13)
    assert np.linalg.norm(r1['traj'][..., 3:7], axis=-1).min() > 0.9


def test_utils_quaternions_agree_with_the_restatement():
    from cbfssm.utils.quaternions import Quaternion
    from cbfssm.utils import Quaternion as Q2
    assert Q2 is Quaternion
    rng = np.random.default_rng(2)
    a, b, v = rng.standard_normal((5, 7, 4)), rng.standard_normal((5, 7, 4)), rng.standard_normal((5, 7, 3))
    ta, tb, tv = torch.tensor(a), torch.tensor(b), torch.tensor(v)
    want = rc.quat_multiply(ta, tb)
    assert torch.equal(Quaternion.multiply(ta, tb), want)
    got_np = Quaternion.multiply_np(a, b)
    assert isinstance(got_np, np.ndarray) and np.array_equal(got_np, want.numpy())
    assert isinstance(Quaternion.multiply(a, b), np.ndarray)
    assert torch.equal(Quaternion.invert(ta), rc.quat_invert(ta)) and np.array_equal(Quaternion.invert_np(a), rc.quat_invert(ta).numpy())
    assert torch.equal(Quaternion.pad_to_quat(tv), rc.pad_to_quat(tv)) and Quaternion.pad_to_quat(v).shape == (5, 7, 4)
    assert np.all(Quaternion.pad_to_quat(v)[..., 0] == 0.0)
    assert torch.equal(Quaternion.rot_vec(tv, ta), rc.rot_vec(tv, ta))
    assert np.array_equal(Quaternion.rot_vec(v, a), rc.rot_vec(tv, ta).numpy())
    # q (x) conj(q) = |q|^2
    n2 = Quaternion.multiply_np(a, Quaternion.invert_np(a))
    assert np.allclose(n2[..., 0], (a * a).sum(-1), rtol=1e-14) and np.allclose(n2[..., 1:], 0.0, atol=1e-14)
