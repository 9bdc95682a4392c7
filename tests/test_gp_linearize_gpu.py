"""GPModel.linearize on the GPU: cbfssm_gp_linearize_f64 through cbfssm.hip.autograd.gp_linearize_eval and
cbfssm.model.gp_tf.GPModel.linearize / transition_jacobians, against reverse-mode autodiff of the CPU oracle per output
dimension (tests/gp_linearize_cases.py, reference (a)).  Rule for the Jacobians: every entry within 1e-6 of the largest entry
of its tensor (gp_autograd_cases.within_rule); fmean / fvar: rtol 1e-8, atol 1e-12 (tests/test_gp_autograd_gpu.py).

The two ill-conditioned cases run in the form the automatic switch picks and are judged by the same 1e-6 rule, fmean and fvar
included: the two CPU codings of fmean differ elementwise by 3e-8 and 5e-7 there, so rtol 1e-8 would be inside the
reference's own error.  Measured on an MI355X (err / largest entry; floor = the two CPU codings against each other, on
the same machine; the switch picks the two-triangular form for both, infinity-norm condition 3.1e8 and 1.4e9):
    (130, 3, 2, 33)  dmean 2.63e-10 = 1.1 x floor 2.43e-10   dvar 2.15e-10 = 0.3 x floor 7.31e-10
    (64, 2, 3, 33)   dmean 5.90e-09 = 1.4 x floor 4.22e-09   dvar 6.03e-09 = 0.9 x floor 6.73e-09"""
import numpy as np
import pytest
import torch

import gp_autograd_cases as gc
import gp_linearize_cases as lc
import gp_tile_grid as grid
from gp_autograd_cases import PARAMS, within_rule

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64, device=DEV)


def _model(p, M, D, Do, grad=(), q_full=False):
    """a gp_tf.GPModel carrying the case's parameters as leaves; `grad`: the names that require grad"""
    from cbfssm.model import gp_tf
    gp = gp_tf.GPModel(in_dim=D, out_dim=Do, num_points=M, gp_var=0.4, gp_len=1.0, zeta_mean=0.1, zeta_pos=1.0, zeta_var=0.01,
                       seed=0, device=DEV, q_full=q_full)
    if not q_full:
        gp.zeta_pos, gp.zeta_mean, gp.zeta_var_unc = _dev(p['zeta_pos']), _dev(p['zeta_mean']), _dev(p['zeta_var_unc'])
        gp.kern.variance_unc, gp.kern.lengthscales_unc = _dev(p['variance_unc']), _dev(p['lengthscales_unc'])
    leaves = dict(zip(PARAMS, gp.parameters()))
    for k in grad:
        leaves[k].requires_grad_()
    return gp


def _pack(p, M, D, Do, mode):
    """a prepared ops.GPPack with the form forced ('dense' / 'tri')"""
    from cbfssm.hip import ops
    pack = ops.GPPack(M, D, Do, torch.device(DEV), form_mode=mode)
    pt = {k: _dev(p[k]) for k in PARAMS}
    con = {k: (ops.tf_forward(pt[k]) if k.endswith('_unc') else pt[k]) for k in PARAMS}
    pack.prepare(con['zeta_pos'], con['lengthscales_unc'], con['variance_unc'], con['zeta_mean'], con['zeta_var_unc'])
    assert pack.gp_form() == mode
    return pack


def _check(case, out, tag, values_by_rule=False):
    """`values_by_rule`: fmean / fvar under the rule of the Jacobians instead of elementwise (the ill-conditioned cases, where
    the two CPU codings themselves differ elementwise by 3e-8 and 5e-7 on fmean: rtol 1e-8 is inside the reference's error)"""
    ref = lc.reference_autodiff(*case)
    fmean, fvar, dmean, dvar = [t.cpu().numpy() for t in out]
    assert dmean.shape == ref['dmean'].shape and dvar.shape == ref['dvar'].shape
    em = within_rule('%s %s dmean' % (case, tag), dmean, ref['dmean'])
    ev = within_rule('%s %s dvar' % (case, tag), dvar, ref['dvar'])
    if values_by_rule:
        within_rule('%s %s fmean' % (case, tag), fmean, ref['fmean'])
        within_rule('%s %s fvar' % (case, tag), fvar, ref['fvar'])
    else:
        np.testing.assert_allclose(fmean, ref['fmean'], rtol=1e-8, atol=1e-12)
        np.testing.assert_allclose(fvar, ref['fvar'], rtol=1e-8, atol=1e-12)
    return em, ev


def _linearize(case, **kw):
    M, D, Do, npts = case
    p, X, _, _ = gc.make_inputs(*case)
    return _model(p, M, D, Do).linearize(_dev(X), **kw)


@pytest.mark.parametrize('name', grid.ROW_IDS)
def test_every_compiled_leaf_against_the_oracle(name):
    """one small shape per compiled (tile height, DK) leaf, three column blocks with the last ragged, in the form the automatic
    switch picks and with the pack forced to dense and to two-triangular"""
    case = grid.predict_case(grid.ROW_BY_NAME[name])
    M, D, Do, npts = case
    from cbfssm.hip import autograd as ag
    _check(case, _linearize(case), 'auto')
    p, X, _, _ = gc.make_inputs(*case)
    for mode in ('dense', 'tri'):
        _check(case, ag.gp_linearize_eval(_pack(p, M, D, Do, mode), _dev(X)), mode)


@pytest.mark.parametrize('case', lc.EDGE_CASES, ids=str)
def test_edges_against_the_oracle(case):
    _check(case, _linearize(case), 'auto')


@pytest.mark.parametrize('case', lc.ILL_CASES, ids=str)
def test_ill_conditioned_in_the_form_the_switch_picks(case):
    M, D, Do, npts = case
    p, X, _, _ = gc.make_inputs(*case)
    gp = _model(p, M, D, Do)
    out = gp.linearize(_dev(X))
    a, b = lc.reference_autodiff(*case), lc.reference_closed_form(*case)
    fm, fv = lc.rel_err(b['dmean'], a['dmean']), lc.rel_err(b['dvar'], a['dvar'])
    em, ev = _check(case, out, gp._pack.gp_form(), values_by_rule=True)
    print('%s form %s cond(pack) %s: dmean %.2e = %.1f x floor %.2e, dvar %.2e = %.1f x floor %.2e'
          % (case, gp._pack.gp_form(), gp._pack.last_cond, em, em / fm, fm, ev, ev / fv, fv))


@pytest.mark.parametrize('case', [(100, 21, 14, 41), (113, 9, 1, 17)], ids=str)
def test_mean_only_is_bitwise_the_mean_of_the_full_call(case):
    fmean, fvar, dmean, dvar = _linearize(case)
    fmean2, fvar2, dmean2, dvar2 = _linearize(case, variance=False)
    assert dvar2 is None and dvar is not None
    assert torch.equal(dmean, dmean2) and torch.equal(fmean, fmean2) and torch.equal(fvar, fvar2)
    _check(case, (fmean2, fvar2, dmean2, dvar), 'mean only')


def test_grid_stride_more_column_blocks_than_workgroups():
    case = lc.LONG_CASE
    assert (case[3] + 15) // 16 > grid.max_workgroups(1)
    _check(case, _linearize(case), 'long')


@pytest.mark.parametrize('case', lc.LONG_CASES[1:], ids=str)
def test_grid_stride_second_trip_at_every_tile_height(case):
    """a few workgroups take a second column block, the last one ragged; the points of the last two column blocks give
    bitwise what a call on those points alone gives -- a second trip sees no state of the first"""
    M, D, Do, npts = case
    assert (npts + 15) // 16 > grid.max_workgroups(grid.leaf_key(M, D, Do)[0])
    out = _linearize(case)
    _check(case, out, 'long')
    s = 16 * ((npts + 15) // 16 - 2)
    p, X, _, _ = gc.make_inputs(*case)
    tail = _model(p, M, D, Do).linearize(_dev(X[s:]))
    for g, t in zip(out, tail):
        assert torch.equal(g[s:], t)


@pytest.mark.parametrize('M,D,Do', [(100, 21, 14), (200, 13, 7)])
def test_batch_independence_and_repeatability(M, D, Do):
    p, X, _, _ = gc.make_inputs(M, D, Do, 41)
    gp = _model(p, M, D, Do)
    Xd = _dev(X)
    full = gp.linearize(Xd)
    again = gp.linearize(Xd)
    head = gp.linearize(Xd[:16].contiguous())
    for a, b, c in zip(full, again, head):
        assert torch.equal(a, b)                          # two identical calls
        assert torch.equal(a[:16], c)                     # the first column block does not see the others


@pytest.mark.parametrize('case', [(100, 21, 14, 41), (200, 13, 7, 41)], ids=str)
def test_against_the_existing_input_adjoint(case):
    """sum_d Wm[n, d] dmean[n, d, :] + Wv[n, d] dvar[n, d, :] is Xnew.grad of sum(Wm o fmean + Wv o fvar) through
    GPModel.predict under grad (gp_predict_bwd_kernel): two kernels, one derivative"""
    M, D, Do, npts = case
    p, X, Wm, Wv = gc.make_inputs(*case)
    gp = _model(p, M, D, Do)
    Xd = _dev(X).requires_grad_()
    fmean, fvar = gp.predict(Xd)
    ((_dev(Wm) * fmean).sum() + (_dev(Wv) * fvar).sum()).backward()
    _, _, dmean, dvar = gp.linearize(Xd)
    mine = (_dev(Wm)[:, :, None] * dmean).sum(1) + (_dev(Wv)[:, :, None] * dvar).sum(1)
    within_rule('%s contracted Jacobians vs Xnew.grad' % (case,), mine.cpu().numpy(), Xd.grad.cpu().numpy())


def test_python_surface():
    M, D, Do = 30, 7, 5
    p, X, _, _ = gc.make_inputs(M, D, Do, 9)
    # no point: empty tensors of the right shapes, nothing launched
    gp = _model(p, M, D, Do)
    fmean, fvar, dmean, dvar = gp.linearize(torch.empty(0, D, dtype=torch.float64, device=DEV))
    assert fmean.shape == fvar.shape == (0, Do) and dmean.shape == dvar.shape == (0, Do, D)
    assert gp.linearize(torch.empty(0, D, dtype=torch.float64, device=DEV), variance=False)[3] is None
    # evaluation only, whatever the leaves and the inputs ask for
    gp = _model(p, M, D, Do, grad=PARAMS)
    out = gp.linearize(_dev(X).requires_grad_())
    assert all(not t.requires_grad and t.grad_fn is None for t in out)
    _check((M, D, Do, 9), out, 'leaves require grad')
    # full-covariance q(z): refused
    full = _model(p, M, D, Do, q_full=True)
    with pytest.raises(ValueError):
        full.linearize(_dev(X))
    with pytest.raises(ValueError):
        full.transition_jacobians(_dev(X[:, :Do]), _dev(X[:, Do:]))


def test_transition_jacobians():
    case = lc.VOLIRO_CASE
    M, D, Do, npts = case
    p, X, _, _ = gc.make_inputs(*case)
    A, B = _model(p, M, D, Do).transition_jacobians(_dev(X[:, :Do]), _dev(X[:, Do:]))
    Ar, Br = lc.transition_reference(*case)
    assert not A.requires_grad and not B.requires_grad
    within_rule('A', A.cpu().numpy(), Ar)
    within_rule('B', B.cpu().numpy(), Br)
    # the GP takes the state alone: a = None, B is empty
    case = (30, 5, 5, 7)
    p, X, _, _ = gc.make_inputs(*case)
    A, B = _model(p, 30, 5, 5).transition_jacobians(_dev(X))
    Ar, Br = lc.transition_reference(*case)
    assert B.shape == (7, 5, 0) == Br.shape
    within_rule('A (a = None)', A.cpu().numpy(), Ar)
