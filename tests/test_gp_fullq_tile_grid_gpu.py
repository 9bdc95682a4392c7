"""Every row of the GP tile grid on full-covariance q(z) (tests/gp_filter_fullq_grid.py), through the C ABI on NaN-prefilled
outputs: cbfssm_gp_fullq_predict_f64 and cbfssm_gp_fullq_bwd_f64 -> cbfssm_reduce_partials_f64 -> cbfssm_gp_fullq_wd_f64 ->
cbfssm_gp_tail_fullq_f64 -> cbfssm_gp_fullq_lbar_f64, in the dense and in the two-triangular form -- against reverse-mode
autodiff on the CPU (tests/gp_fullq_cases.py) -- and the host-side schedules of that path: the persistent column-block loop
of the adjoint and of the forward in its second round, the W_d sum in two and in three slices.
Rules (tests/test_gp_fullq_gpu.py): fmean / fvar rtol 1e-8, atol 1e-11; KL 1e-9 relative; every gradient tensor within 1e-6
of its largest entry, for the loss and for prior_kl alone; d/dq exactly zero above the diagonal, W_d exactly symmetric; two
calls are bitwise equal.  tests/test_gp_filter_fullq_grid_cpu.py proves that the rows reach every compiled leaf and that the
reference sits 100 times inside these rules.  Every comparison prints what it achieved."""
import ctypes as C

import numpy as np
import pytest
import torch

import gp_fullq_cases as fq
import gp_filter_fullq_grid as fg
from gp_fullq_cases import PARAMS, within_rule
from test_gp_fullq_gpu import DEV, _abi, _check_upper_zero, _dev

pytestmark = pytest.mark.gpu


def _value_rule(name, x, r):
    x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    assert x.shape == r.shape and np.all(np.isfinite(x)), name
    ratio = (np.abs(x - r) / (1e-11 + 1e-8 * np.abs(r))).max()
    print('%-34s max|ref| %.3e  |err| / (1e-11 + 1e-8 |ref|) %.2e' % (name, np.abs(r).max(), ratio))
    np.testing.assert_allclose(x, r, rtol=1e-8, atol=1e-11)


def _kl_rule(kl, r):
    err = abs(float(kl) - r) / abs(r)
    print('%-34s ref %.6e  rel err %.2e' % ('kl', r, err))
    assert float(kl) == pytest.approx(r, rel=1e-9)


def _grad_rules(g, gX, ref, prefix, key, zeros=()):
    if gX is not None:
        within_rule('gX', gX.cpu().numpy(), ref['g_X'])
    for k in PARAMS:
        if k in zeros:
            assert not np.any(ref[key + k]) and not np.any(g[k]), prefix + k + ' must be exactly 0'
        else:
            within_rule(prefix + k, g[k], ref[key + k].reshape(g[k].shape))


def _full_rules(case, form='dense'):
    """the C calls twice and once more for prior_kl alone: every rule on the whole batch; returns the inputs and the outputs"""
    M, D, Do, npts = case
    ref = fq.reference(*case)
    p, X, Wm, Wv = fq.make_inputs(*case)
    g, gX, fmean, fvar, kl, bits = _abi(M, D, Do, npts, p, X, Wm, Wv, fq.KL_WEIGHT, form=form)
    _, _, _, _, _, bits2 = _abi(M, D, Do, npts, p, X, Wm, Wv, fq.KL_WEIGHT, form=form)
    gk, _, _, _, _, _ = _abi(M, D, Do, npts, p, X, Wm, Wv, 1.0, data=False, form=form)
    assert gX.shape == (npts, D) and not torch.isnan(gX).any(), 'an entry of gX was never written'
    _value_rule('fmean', fmean, ref['fmean'])
    _value_rule('fvar', fvar, ref['fvar'])
    _kl_rule(kl, ref['kl'])
    _grad_rules(g, gX, ref, 'loss: ', 'g_')
    _grad_rules(gk, None, ref, 'prior_kl alone: ', 'k_', zeros=fg.kl_zero_names(M))
    _check_upper_zero(g['zeta_sqrt'], M)
    _check_upper_zero(gk['zeta_sqrt'], M)
    assert not torch.isnan(bits).any() and torch.equal(bits, bits2), 'two calls differ'
    return p, X, Wm, Wv, gX, fmean, fvar


@pytest.mark.parametrize('name', fg.ROW_IDS)
def test_full_q_dense_form(name):
    _full_rules(fg.fullq_case(fg.ROW_BY_NAME[name]))


@pytest.mark.parametrize('name', fg.ROW_IDS)
def test_full_q_two_triangular_form(name):
    """the forward in the reference's own order of the conditional, and the adjoint on the pack that form prepares"""
    M, D, Do, npts = case = fg.fullq_case(fg.ROW_BY_NAME[name])
    ref = fq.reference(*case)
    p, X, Wm, Wv = fq.make_inputs(*case)
    g, gX, fmean, fvar, kl, _ = _abi(M, D, Do, npts, p, X, Wm, Wv, fq.KL_WEIGHT, form='tri')
    _value_rule('tri fmean', fmean, ref['fmean'])
    _value_rule('tri fvar', fvar, ref['fvar'])
    _kl_rule(kl, ref['kl'])
    _grad_rules(g, gX, ref, 'tri loss: ', 'g_')
    _check_upper_zero(g['zeta_sqrt'], M)


def _tail(npts):
    s = 16 * ((npts + 15) // 16 - 2)
    assert 16 < npts - s < 32
    return s


@pytest.mark.parametrize('case', fg.FULLQ_BWD_LONG, ids=str)
def test_adjoint_persistent_loop_second_round(case):
    """more column blocks than workgroups: the rules on the whole batch, and gX, fmean, fvar of the last two column blocks (a
    second block of their workgroups; the last one ragged) equal bitwise those of a call on these points alone -- a
    workgroup's second block sees no state of its first"""
    M, D, Do, npts = case
    p, X, Wm, Wv, gX, fmean, fvar = _full_rules(case)
    s = _tail(npts)
    _, gX_t, fmean_t, fvar_t, _, _ = _abi(M, D, Do, npts - s, p, X[s:], Wm[s:], Wv[s:], fq.KL_WEIGHT)
    assert torch.equal(gX[s:], gX_t), 'gX of the last column blocks depends on the blocks before them'
    assert torch.equal(fmean[s:], fmean_t) and torch.equal(fvar[s:], fvar_t)


@pytest.mark.parametrize('case', fg.FULLQ_SLICE_ROWS, ids=str)
def test_w_sum_in_two_and_three_slices(case):
    _full_rules(case)


def _forward(M, D, Do, npts, p, X, form):
    """cbfssm_gp_fullq_prepare_f64 and cbfssm_gp_fullq_predict_f64 alone, on NaN-prefilled outputs"""
    from cbfssm.hip import lib as _l, ops
    from cbfssm.hip.ops import _ptr, _stream
    lib = _l.load()
    nan = float('nan')
    pack = ops.GPPack(M, D, Do, torch.device(DEV), form_mode=form)
    pt = {k: _dev(p[k]) for k in PARAMS}
    var, ls = ops.tf_forward(pt['variance_unc']), ops.tf_forward(pt['lengthscales_unc'])
    pack.prepare(pt['zeta_pos'], ls, var, pt['zeta_mean'], torch.zeros(M, Do, dtype=torch.float64, device=DEV))
    lay = pack.layout
    qpack = torch.full((lib.cbfssm_gp_fullq_pack_elems(C.byref(lay)),), nan, dtype=torch.float64, device=DEV)
    _l.check(lib.cbfssm_gp_fullq_prepare_f64(C.byref(lay), _ptr(pt['zeta_sqrt'].contiguous()), _ptr(qpack), _stream()), 'prepare')
    Xd = _dev(X)
    fmean = torch.full((npts, Do), nan, dtype=torch.float64, device=DEV)
    fvar = torch.full((npts, Do), nan, dtype=torch.float64, device=DEV)
    _l.check(lib.cbfssm_gp_fullq_predict_f64(C.byref(lay), _ptr(pack.buf), _ptr(qpack), _ptr(Xd), npts, _ptr(fmean), _ptr(fvar),
                                             _stream()), 'forward')
    return fmean, fvar


@pytest.mark.parametrize('form', ['dense', 'tri'])
@pytest.mark.parametrize('case', fg.FULLQ_FWD_LONG, ids=str)
def test_forward_persistent_loop_second_round(case, form):
    """more column blocks than four times the adjoint's workgroup cap: the value rules on the whole batch, twice the same
    bits, and the last two column blocks equal bitwise a call on these points alone"""
    M, D, Do, npts = case
    ref = fq.reference(*case)
    p, X, _, _ = fq.make_inputs(*case)
    fmean, fvar = _forward(M, D, Do, npts, p, X, form)
    fmean2, fvar2 = _forward(M, D, Do, npts, p, X, form)
    _value_rule('fmean', fmean, ref['fmean'])
    _value_rule('fvar', fvar, ref['fvar'])
    assert torch.equal(fmean, fmean2) and torch.equal(fvar, fvar2), 'two calls differ'
    s = _tail(npts)
    fmean_t, fvar_t = _forward(M, D, Do, npts - s, p, X[s:], form)
    assert torch.equal(fmean[s:], fmean_t) and torch.equal(fvar[s:], fvar_t), 'the last column blocks depend on the blocks before'
