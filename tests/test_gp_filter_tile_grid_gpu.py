"""Every row of the GP tile grid on the fused filter loop (tests/gp_filter_fullq_grid.py), through the C ABI on
NaN-prefilled outputs: cbfssm_gp_filter_f64 in its dense form with cbfssm_gp_filter_bwd_f64 -> cbfssm_reduce_partials_f64 ->
cbfssm_gp_tail_f64, and the two-triangular forward feeding the same adjoint -- against reverse-mode autodiff of the
recurrence over the CPU oracle (tests/gp_filter_cases.py).  Every row runs the random mask: both branches of the conditioned
epilogue and of its adjoint in every leaf, ytilde NaN where the mask is 0.
Rules (tests/gp_filter_cases.py): trajectories within 1e-8 of max |traj|, kl 1e-9 relative, gradients within 1e-6 of their
tensor's largest entry; two calls are bitwise equal.  tests/test_gp_filter_fullq_grid_cpu.py proves that the rows reach
every compiled leaf and that the reference sits 100 times inside these rules.  Every comparison prints what it achieved."""
import numpy as np
import pytest
import torch

import gp_filter_cases as fc
import gp_filter_fullq_grid as fg
from gp_filter_cases import traj_rule, kl_rule
from test_gp_filter_gpu import _abi, _check_grads, _dev, _model

pytestmark = pytest.mark.gpu


def _check_saves_and_mask(o, cond):
    assert np.all(np.isfinite(o['msave'])) and np.all(np.isfinite(o['vsave'])) and np.all(o['vsave'] > 0)
    assert np.all(np.isfinite(o['ytilde']))
    assert not np.any(o['ytilde'][cond == 0.0]), 'gytilde must be exactly 0 where cond = 0'


@pytest.mark.parametrize('name', fg.ROW_IDS)
def test_filter_dense_form(name):
    case = fg.filter_case(fg.ROW_BY_NAME[name])
    ref = fc.reference(case)
    cond = fc.make_inputs(*case)[4]
    o1, o2 = _abi(case), _abi(case)
    traj_rule('traj', o1['traj'], ref['traj'])
    kl_rule(o1['kl'], ref['kl'])
    _check_saves_and_mask(o1, cond)
    _check_grads(o1, ref, case)
    for k in ('traj', 'msave', 'vsave', 'h0', 'a', 'ytilde', 'var_x', 'var_y', 'gflat'):
        assert np.all(np.isfinite(o1[k])), k
        assert np.array_equal(o1[k], o2[k]), 'two calls differ: ' + k
    assert o1['kl'] == o2['kl']


@pytest.mark.parametrize('name', fg.ROW_IDS)
def test_two_triangular_filter_feeds_the_adjoint(name):
    """what GPModel.filter runs once the automatic rule has switched form: the adjoint takes traj / msave / vsave of the
    two-triangular forward"""
    case = fg.filter_case(fg.ROW_BY_NAME[name])
    ref = fc.reference(case)
    cond = fc.make_inputs(*case)[4]
    od, ot = _abi(case, 'dense', backward=False), _abi(case, 'tri')
    traj_rule('tri against dense', ot['traj'], od['traj'])
    traj_rule('dense against the reference', od['traj'], ref['traj'])
    traj_rule('tri against the reference', ot['traj'], ref['traj'])
    kl_rule(ot['kl'], od['kl'])
    kl_rule(od['kl'], ref['kl'])
    kl_rule(ot['kl'], ref['kl'])
    _check_saves_and_mask(ot, cond)
    _check_grads(ot, ref, case)


@pytest.mark.parametrize('name', fg.CHAIN_GROUP_ROWS)
def test_chain_groups_do_not_interact(name):
    """chains 0..15 of the N = 21 run equal an N = 16 run of the same chains bitwise, on the trajectory, ga and gytilde"""
    case = fg.filter_case(fg.ROW_BY_NAME[name])
    M, D, Do, N, T, reverse, with_vx, k_factor, mask = case
    p, h0, a, ytilde, cond, eps, var_x, var_y, W = fc.make_inputs(*case)

    def run(n):
        gp, _ = _model(p, M, D, Do)
        ad, yd = _dev(a[:, :n]).requires_grad_(), _dev(ytilde[:, :n]).requires_grad_()
        traj, kl = gp.filter(_dev(h0[:n]), ad, yd, _dev(eps[:, :n]), _dev(var_x) if with_vx else None, _dev(var_y),
                             cond=_dev(cond[:, :n]), k_factor=k_factor, reverse=reverse)
        ((_dev(W[:, :n]) * traj).sum() + fc.KL_WEIGHT * kl).backward()
        return traj.detach(), ad.grad, yd.grad
    t21, ga21, gy21 = run(N)
    t16, ga16, gy16 = run(16)
    assert N > 16 and D > Do and t21.shape == (T, N, Do) and ga16.shape == (T, 16, D - Do) and gy16.shape == (T, 16, Do)
    assert bool(torch.isfinite(t21).all()) and bool(torch.isfinite(ga21).all()) and bool(torch.isfinite(gy21).all())
    assert torch.equal(t21[:, :16], t16) and torch.equal(ga21[:, :16], ga16) and torch.equal(gy21[:, :16], gy16)
