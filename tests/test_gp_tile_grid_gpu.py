"""Every row of the GP-surface tile grid (tests/gp_tile_grid.py) on the GPU, through the C ABI: the batch adjoint
cbfssm_gp_predict_bwd_f64 -> cbfssm_reduce_partials_f64 -> cbfssm_gp_tail_f64, the fused rollout in its dense form with
its adjoint, and the two-triangular rollout feeding the same adjoint -- against reverse-mode autodiff of the CPU oracle.
Rules (tests/gp_autograd_cases.py, tests/gp_rollout_cases.py): gradients within 1e-6 of their tensor's largest entry,
trajectories within 1e-8 of max |traj|, entropy 1e-9 relative; two calls are bitwise equal.
tests/test_gp_tile_grid_cpu.py proves that the rows reach every compiled leaf and that the reference sits 100 times
inside these rules.  Every comparison prints what it achieved."""
import numpy as np
import pytest
import torch

import gp_autograd_cases as gc
import gp_rollout_cases as rc
import gp_tile_grid as gg
from gp_autograd_cases import PARAMS, within_rule
from gp_rollout_cases import traj_rule, entropy_rule
from test_gp_autograd_gpu import _abi_grads
from test_gp_rollout_gpu import _abi, _check_grads, _dev, _model

pytestmark = pytest.mark.gpu


def _batch_adjoint(case):
    """the three C calls on NaN-prefilled outputs, twice: the rule on gX and the five parameter gradients, bitwise repeat"""
    M, D, Do, npts = case
    ref = gg.predict_reference(case)
    p, X, Wm, Wv = gc.make_inputs(*case)
    g, gX, gflat = _abi_grads(M, D, Do, npts, p, X, Wm, Wv, gc.KL_WEIGHT)
    g2, gX2, gflat2 = _abi_grads(M, D, Do, npts, p, X, Wm, Wv, gc.KL_WEIGHT)
    assert gX.shape == (npts, D) and not np.isnan(gX).any(), 'an entry of gX was never written'
    within_rule('gX', gX, ref['g_X'])
    for k in PARAMS:
        within_rule('predict: ' + k, g[k], ref['g_' + k].reshape(g[k].shape))
    assert np.array_equal(gX, gX2) and torch.equal(gflat, gflat2), 'two calls differ'
    return p, X, Wm, Wv, gX


def _rollout_names(case):
    return ('h0', 'a') + (('var_add',) if case[6] else ()) + PARAMS


@pytest.mark.parametrize('name', gg.ROW_IDS)
def test_batch_adjoint(name):
    _batch_adjoint(gg.predict_case(gg.ROW_BY_NAME[name]))


@pytest.mark.parametrize('name', gg.ROW_IDS)
def test_rollout_dense_form(name):
    case = gg.rollout_case(gg.ROW_BY_NAME[name])
    ref = rc.reference(case)
    o1, o2 = _abi(case), _abi(case)
    traj_rule('traj', o1['traj'], ref['traj'])
    entropy_rule(o1['entropy'], ref['entropy'])
    assert np.all(np.isfinite(o1['vsave'])) and np.all(o1['vsave'] > 0)
    _check_grads(o1, ref, _rollout_names(case))
    for k in ('traj', 'vsave', 'h0', 'a', 'var_add', 'gflat'):
        assert np.array_equal(o1[k], o2[k]), 'two calls differ: ' + k
    assert o1['entropy'] == o2['entropy']


@pytest.mark.parametrize('name', gg.ROW_IDS)
def test_two_triangular_rollout_feeds_the_adjoint(name):
    """what GPModel.rollout runs once the automatic rule has switched form: the adjoint takes traj / vsave of the
    two-triangular forward"""
    case = gg.rollout_case(gg.ROW_BY_NAME[name])
    ref = rc.reference(case)
    od, ot = _abi(case, 'dense', backward=False), _abi(case, 'tri')
    traj_rule('tri against dense', ot['traj'], od['traj'])
    traj_rule('tri against the reference', ot['traj'], ref['traj'])
    entropy_rule(ot['entropy'], od['entropy'])
    entropy_rule(ot['entropy'], ref['entropy'])
    assert np.all(np.isfinite(ot['vsave'])) and np.all(ot['vsave'] > 0)
    _check_grads(ot, ref, _rollout_names(case))


@pytest.mark.parametrize('case', gg.LONG_ROWS, ids=str)
def test_persistent_loop_second_round(case):
    """more column blocks than workgroups: the rules on the whole batch, and gX of the last two column blocks (a second
    block of their workgroups; the last one ragged) equals bitwise gX of a call on those points alone -- a workgroup's
    second block sees no state of its first"""
    M, D, Do, npts = case
    p, X, Wm, Wv, gX = _batch_adjoint(case)
    s = 16 * ((npts + 15) // 16 - 2)
    assert 16 < npts - s < 32
    _, gX_tail, _ = _abi_grads(M, D, Do, npts - s, p, X[s:], Wm[s:], Wv[s:], gc.KL_WEIGHT)
    assert np.array_equal(gX[s:], gX_tail), 'gX of the last column blocks depends on the blocks before them'


@pytest.mark.parametrize('name', gg.CHAIN_GROUP_ROWS)
def test_chain_groups_do_not_interact(name):
    """chains 0..15 of the N = 21 run equal an N = 16 run of the same chains bitwise, on the trajectory and on ga"""
    case = gg.rollout_case(gg.ROW_BY_NAME[name])
    M, D, Do, N, T, reverse, with_var = case
    p, h0, a, eps, var_add, W = rc.make_inputs(*case)

    def run(n):
        gp, _ = _model(p, M, D, Do)
        ad = _dev(a[:, :n]).requires_grad_()
        traj, ent = gp.rollout(_dev(h0[:n]), ad, _dev(eps[:, :n]), _dev(var_add) if with_var else None, reverse=reverse)
        ((_dev(W[:, :n]) * traj).sum() + rc.ENT_WEIGHT * ent).backward()
        return traj.detach(), ad.grad
    t21, g21 = run(N)
    t16, g16 = run(16)
    assert N > 16 and t21.shape == (T, N, Do) and g16.shape == (T, 16, D - Do) and D > Do
    assert torch.equal(t21[:, :16], t16) and torch.equal(g21[:, :16], g16)
