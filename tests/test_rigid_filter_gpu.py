"""Voliro's forward filter run on the GPU: cbfssm_rigid_filter_f64 and cbfssm_rigid_filter_bwd_f64 ->
cbfssm_reduce_partials_f64 through the C ABI, and cbfssm.hip.autograd.rigid_filter / rigid_filter_eval, against
reverse-mode autodiff of the float64 CPU restatement (tests/rigid_filter_cases.py, which states the rules: gradients
within 1e-6 of their tensor's largest entry, trajectories within 1e-8 of max |traj|, kl 1e-9 relative)."""
import ctypes as C

import numpy as np
import pytest
import torch

import rigid_filter_cases as rc
from rigid_filter_cases import CASES, GRADS, within_rule, traj_rule, scalar_rule

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')


def _dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64, device=DEV)


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float64, device=DEV)


def _body():
    from cbfssm.hip import lib as _l
    b = rc.body()
    return _l.rigid_body(b['mass_inv'], b['inertia_inv'], b['gravity'], b['dt'])


def _abi(case, gtraj=None, g_kl=rc.KL_WEIGHT):
    """forward and adjoint through the C ABI on NaN-prefilled outputs; returns a dict of device tensors"""
    from cbfssm.hip import lib as _l
    from cbfssm.hip.ops import _ptr, _stream
    N, S = case
    lib = _l.load()
    inp = rc.make_inputs(N, S)
    d = {k: _dev(inp[k]) for k in ('x0', 'u', 'y', 'eps', 'var_x', 'var_y')}
    body = _body()
    nwg = lib.cbfssm_rigid_filter_partials(N)
    assert nwg == (N + 63) // 64
    traj, kl_part = _nan(S, N, 13), _nan(nwg + 32)
    _l.check(lib.cbfssm_rigid_filter_f64(C.byref(body), _ptr(d['x0']), _ptr(d['u']), _ptr(d['y']), _ptr(d['eps']),
                                         _ptr(d['var_x']), _ptr(d['var_y']), N, S, _ptr(traj), _ptr(kl_part), _stream()),
             'cbfssm_rigid_filter_f64')
    kl = _nan(1)
    _l.check(lib.cbfssm_reduce_partials_f64(_ptr(kl_part), 1, nwg, _ptr(kl), _stream()), 'reduce')
    gt = _dev(inp['W']) if gtraj is None else gtraj
    gkl = _dev([g_kl])
    gx0, gu, gy, gpart = _nan(N, 13), _nan(S, N, 6), _nan(S, N, 13), _nan((nwg + 32) * 32)
    _l.check(lib.cbfssm_rigid_filter_bwd_f64(C.byref(body), _ptr(d['x0']), _ptr(d['u']), _ptr(d['y']), _ptr(d['eps']),
                                             _ptr(d['var_x']), _ptr(d['var_y']), _ptr(traj), _ptr(gt), _ptr(gkl), N, S,
                                             _ptr(gx0), _ptr(gu), _ptr(gy), _ptr(gpart), _stream()), 'cbfssm_rigid_filter_bwd_f64')
    red = _nan(32)
    _l.check(lib.cbfssm_reduce_partials_f64(_ptr(gpart), 32, nwg, _ptr(red), _stream()), 'reduce')
    torch.cuda.synchronize()
    assert bool(torch.all(red[26:] == 0.0))                    # the padding of the slab is written, as zeros
    return {'traj': traj, 'kl': kl[0], 'x0': gx0, 'u': gu, 'y': gy, 'var_x': red[0:13].clone(), 'var_y': red[13:26].clone()}


def _autograd(case, grad=True):
    from cbfssm.hip import autograd
    inp = rc.make_inputs(*case)
    lv = {k: _dev(inp[k]).requires_grad_(grad) for k in GRADS}
    traj, kl = autograd.rigid_filter(_body(), lv['x0'], lv['u'], lv['y'], _dev(inp['eps']), lv['var_x'], lv['var_y'])
    return inp, lv, traj, kl


@pytest.mark.parametrize('case', CASES, ids=str)
def test_c_abi_against_the_reference(case):
    ref = rc.reference(case)
    o1, o2 = _abi(case), _abi(case)
    traj_rule('traj', o1['traj'].cpu().numpy(), ref['traj'])
    scalar_rule('kl', float(o1['kl']), ref['kl'])
    for k in GRADS:
        within_rule(k, o1[k].cpu().numpy(), ref['g_' + k])
    for k in o1:
        assert torch.equal(o1[k], o2[k]), 'two calls differ: ' + k


@pytest.mark.parametrize('case', CASES, ids=str)
def test_autograd_function_gives_the_bits_of_the_c_abi(case):
    o = _abi(case)
    inp, lv, traj, kl = _autograd(case)
    assert traj.grad_fn is not None and kl.grad_fn is not None and traj.shape == (case[1], case[0], 13) and kl.shape == ()
    assert torch.equal(traj.detach(), o['traj']) and torch.equal(kl.detach(), o['kl'])
    ((_dev(inp['W']) * traj).sum() + rc.KL_WEIGHT * kl).backward()
    for k in GRADS:
        assert torch.equal(lv[k].grad, o[k]), k


@pytest.mark.parametrize('case', [CASES[1], CASES[4]], ids=str)
def test_eval_returns_the_forward_bits_without_a_grad_fn(case):
    from cbfssm.hip import autograd
    inp, lv, traj, kl = _autograd(case)
    t0, k0 = autograd.rigid_filter_eval(_body(), lv['x0'], lv['u'], lv['y'], _dev(inp['eps']), lv['var_x'], lv['var_y'])
    assert t0.grad_fn is None and k0.grad_fn is None and not t0.requires_grad
    assert torch.equal(t0, traj.detach()) and torch.equal(k0, kl.detach())
    # no gradient request: the function itself returns plain tensors
    _, _, t1, k1 = _autograd(case, grad=False)
    assert t1.grad_fn is None and k1.grad_fn is None and torch.equal(t1, t0) and torch.equal(k1, k0)


def test_eps_receives_no_gradient():
    from cbfssm.hip import autograd
    case = CASES[1]
    inp = rc.make_inputs(*case)
    eps = _dev(inp['eps']).requires_grad_()
    x0 = _dev(inp['x0']).requires_grad_()
    traj, kl = autograd.rigid_filter(_body(), x0, _dev(inp['u']), _dev(inp['y']), eps, _dev(inp['var_x']), _dev(inp['var_y']))
    (traj.sum() + kl).backward()
    assert eps.grad is None and x0.grad is not None


@pytest.mark.parametrize('case,chain', [(CASES[4], 70), (CASES[5], 319), (CASES[3], 64)], ids=str)
def test_chains_do_not_interact(case, chain):
    """g_kl = 0 and gtraj zero except on one chain: every other chain's gx0, gu, gy are exactly zero"""
    N, S = case
    gt = torch.zeros(S, N, 13, dtype=torch.float64, device=DEV)
    gt[:, chain] = _dev(rc.make_inputs(N, S)['W'][:, chain])
    o = _abi(case, gtraj=gt, g_kl=0.0)
    others = torch.ones(N, dtype=torch.bool, device=DEV)
    others[chain] = False
    assert bool(torch.all(o['x0'][others] == 0.0)) and bool(torch.all(o['u'][:, others] == 0.0))
    assert bool(torch.all(o['y'][:, others] == 0.0))
    assert float(o['x0'][chain].abs().max()) > 0.0 and float(o['u'][:, chain].abs().max()) > 0.0


def test_no_chains_launch_nothing():
    from cbfssm.hip import autograd
    z = torch.zeros
    x0 = z(0, 13, dtype=torch.float64, device=DEV).requires_grad_()
    vx = _dev(rc.SD ** 2).requires_grad_()
    traj, kl = autograd.rigid_filter(_body(), x0, z(3, 0, 6, dtype=torch.float64, device=DEV),
                                     z(3, 0, 13, dtype=torch.float64, device=DEV), z(3, 0, dtype=torch.float64, device=DEV),
                                     vx, _dev((1.3 * rc.SD) ** 2))
    assert traj.shape == (3, 0, 13) and float(kl) == 0.0
    (traj.sum() + kl).backward()
    assert x0.grad.shape == (0, 13) and bool(torch.all(vx.grad == 0.0))
