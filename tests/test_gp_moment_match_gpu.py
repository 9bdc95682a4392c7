"""GPModel.moment_match on the GPU: cbfssm_gp_moment_match_f64 through cbfssm.hip.autograd.gp_moment_match_eval and
cbfssm.model.gp_tf.GPModel.moment_match / transition_moments, against the closed form in numpy (tests/gp_moment_match_cases.py,
reference (a), which tests/test_gp_moment_match_cpu.py pins to Gauss-Hermite quadrature through the oracle).

Rule: the project's for evaluation outputs (ekf, eks, linearize's values): every entry within 1e-8 of the largest entry of the
reference tensor -- for fmean, xcov, the diagonal of fcov, and separately for the strictly lower triangle of fcov against its
own largest entry, so that the small cross terms do not hide behind the variances.  Every check prints its figure; the
figures of one run on an MI355X are in profiles/gp_moment_match/parity.txt."""
import numpy as np
import pytest
import torch

import gp_autograd_cases as gc
import gp_moment_match_cases as mc
import gp_tile_grid as grid
from gp_autograd_cases import PARAMS, within_rule

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RULE = 1e-8


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


def _check(tag, out, ref):
    fmean, fcov, xcov, info = out
    fmean, fcov, info = fmean.cpu().numpy(), fcov.cpu().numpy(), info.cpu().numpy()
    assert info.dtype == np.int64 and not info.any(), (tag, info)
    assert fmean.shape == ref['fmean'].shape and fcov.shape == ref['fcov'].shape
    within_rule('%s fmean' % tag, fmean, ref['fmean'], RULE)
    within_rule('%s diag fcov' % tag, mc.diagonal(fcov), mc.diagonal(ref['fcov']), RULE)
    if fcov.shape[-1] > 1:
        within_rule('%s lower fcov' % tag, mc.lower(fcov), mc.lower(ref['fcov']), RULE)
    assert np.array_equal(fcov, np.transpose(fcov, (0, 2, 1))), '%s: fcov is not bitwise symmetric' % tag
    if xcov is not None:
        xcov = xcov.cpu().numpy()
        assert xcov.shape == ref['xcov'].shape
        if np.abs(ref['xcov']).max() > 0.0:
            within_rule('%s xcov' % tag, xcov, ref['xcov'], RULE)
        else:
            assert not xcov.any(), '%s: xcov is not exactly zero' % tag


def _run(case, kind='mixed', **kw):
    M, D, Do, npts = case
    p, mean, cov, _ = mc.make_beliefs(M, D, Do, npts, kind)
    return _model(p, M, D, Do).moment_match(_dev(mean), _dev(cov), **kw)


@pytest.mark.parametrize('name', grid.ROW_IDS)
def test_every_compiled_leaf_against_the_closed_form(name):
    """one small shape per compiled (tile height, DK) leaf, three point groups with the last ragged, rank-2, full-rank and
    block covariances in turn, in the form the automatic switch picks and with the pack forced to dense and to two-triangular"""
    _, M, D, Do = grid.ROW_BY_NAME[name]
    case = (M, D, Do, mc.N_POINTS)
    from cbfssm.hip import autograd as ag
    ref = mc.reference_closed_form(*case)
    _check('%s auto' % name, _run(case), ref)
    p, mean, cov, _ = mc.make_beliefs(*case)
    for mode in ('dense', 'tri'):
        _check('%s %s' % (name, mode), ag.gp_moment_match_eval(_pack(p, M, D, Do, mode), _dev(mean), _dev(cov)), ref)


@pytest.mark.parametrize('case', mc.EDGE_CASES + [mc.VOLIRO_CASE], ids=str)
def test_edges_against_the_closed_form(case):
    _check(str(case), _run(case), mc.reference_closed_form(*case))


def test_grid_stride_more_point_groups_than_workgroups():
    case = mc.LONG_CASE
    assert (case[3] + 15) // 16 > grid.max_workgroups(1)
    _check('long', _run(case), mc.reference_closed_form(*case))


@pytest.mark.parametrize('case', mc.LONG_CASES[1:], ids=str)
def test_grid_stride_second_trip_at_every_tile_height(case):
    """a few workgroups take a second point group, the last one ragged; the points of the last two groups give bitwise
    what a call on those points alone gives -- a second trip sees no state of the first"""
    M, D, Do, npts = case
    assert (npts + 15) // 16 > grid.max_workgroups(grid.leaf_key(M, D, Do)[0])
    out = _run(case)
    _check('long %s' % (case,), out, mc.reference_closed_form(*case))
    s = 16 * ((npts + 15) // 16 - 2)
    p, mean, cov, _ = mc.make_beliefs(*case)
    tail = _model(p, M, D, Do).moment_match(_dev(mean[s:]), _dev(cov[s:]))
    for g, t in zip(out, tail):
        assert torch.equal(g[s:], t)


@pytest.mark.parametrize('case', [(100, 21, 14, 19), (200, 13, 7, 19)], ids=str)
def test_zero_covariance_is_predict(case):
    """cov = 0 and cov = None: fmean and diag fcov are the GPU's own predict, the off-diagonal is that of (a), xcov is
    exactly zero; the two calls are bitwise the same"""
    M, D, Do, npts = case
    p, mean, cov, _ = mc.make_beliefs(M, D, Do, npts, 'zero')
    assert not cov.any()
    gp = _model(p, M, D, Do)
    zero = gp.moment_match(_dev(mean), _dev(cov))
    none = gp.moment_match(_dev(mean), None)
    for a, b in zip(zero, none):
        assert torch.equal(a, b)
    assert not zero[2].cpu().numpy().any() and not zero[3].cpu().numpy().any()
    fmean, fvar = gp.predict(_dev(mean))
    within_rule('%s fmean vs predict' % (case,), zero[0].cpu().numpy(), fmean.cpu().numpy(), RULE)
    within_rule('%s diag fcov vs predict' % (case,), mc.diagonal(zero[1].cpu().numpy()), fvar.cpu().numpy(), RULE)
    # off the diagonal the exact value is zero ((alpha.k)(k.alpha) - fmean fmean^T): the reference's own triangle is rounding
    # noise there, so the rule is applied to the whole tensor -- every entry within 1e-8 of the largest entry of fcov
    ref = mc.reference_closed_form(M, D, Do, npts, 'zero')
    fcov = zero[1].cpu().numpy()
    assert np.array_equal(fcov, np.transpose(fcov, (0, 2, 1)))
    within_rule('%s fcov vs (a)' % (case,), fcov, ref['fcov'], RULE)
    assert np.abs(mc.lower(fcov)).max() < RULE * np.abs(ref['fcov']).max()


def test_wide_belief():
    """eigenvalues of the covariance around 1e4 squared lengthscales: finite, within the rule, fmean -> 0, diag fcov -> v"""
    case = mc.WIDE_CASE
    out = _run(case, 'wide')
    ref = mc.reference_closed_form(*case, 'wide')
    _check('wide', out, ref)
    v = float(mc.softplus(gc.make_inputs(*case)[0]['variance_unc'])[0])
    assert np.abs(out[0].cpu().numpy()).max() < 1e-8
    assert np.abs(mc.diagonal(out[1].cpu().numpy()) - v).max() < 1e-8 * v


def test_rank_one_covariance():
    case = mc.RANK1_CASE
    _check('rank one', _run(case, 'rank1'), mc.reference_closed_form(*case, 'rank1'))


@pytest.mark.parametrize('case', [(100, 21, 14, 37), (113, 9, 1, 17)], ids=str)
def test_without_the_cross_covariance_is_bitwise_the_full_call(case):
    fmean, fcov, xcov, info = _run(case)
    fmean2, fcov2, xcov2, info2 = _run(case, cross=False)
    assert xcov2 is None and xcov is not None
    assert torch.equal(fmean, fmean2) and torch.equal(fcov, fcov2) and torch.equal(info, info2)


def test_an_indefinite_covariance_is_flagged_and_stays_alone():
    M, D, Do, npts = 100, 21, 14, 37
    p, mean, cov, _ = mc.make_beliefs(M, D, Do, npts)
    gp = _model(p, M, D, Do)
    good = gp.moment_match(_dev(mean), _dev(cov))
    bad_cov = cov.copy()
    bad_cov[20] = -3.0 * np.eye(D) * mc.softplus(p['lengthscales_unc']) ** 2         # I + S~ = -2 I: the first pivot fails
    bad = gp.moment_match(_dev(mean), _dev(bad_cov))
    info = bad[3].cpu().numpy()
    assert info[20] != 0 and not np.delete(info, 20).any()
    keep = torch.tensor(np.delete(np.arange(npts), 20), device=DEV)
    for a, b in zip(good[:3], bad[:3]):
        assert torch.isnan(b[20]).all()
        assert torch.equal(a[keep], b[keep])
    # the second factor alone: -0.75 I has I + S~ = I / 4 positive and I / 2 + S~ = -I / 4 not
    bad_cov[20] = -0.75 * np.eye(D) * mc.softplus(p['lengthscales_unc']) ** 2
    info = gp.moment_match(_dev(mean), _dev(bad_cov))[3].cpu().numpy()
    assert info[20] == 2 and not np.delete(info, 20).any()


@pytest.mark.parametrize('name', grid.CHAIN_GROUP_ROWS)
def test_repeatability_and_point_group_independence(name):
    _, M, D, Do = grid.ROW_BY_NAME[name]
    p, mean, cov, _ = mc.make_beliefs(M, D, Do, mc.N_POINTS)
    gp = _model(p, M, D, Do)
    full = gp.moment_match(_dev(mean), _dev(cov))
    again = gp.moment_match(_dev(mean), _dev(cov))
    head = gp.moment_match(_dev(mean[:16]), _dev(cov[:16]))
    for a, b, c in zip(full, again, head):
        assert torch.equal(a, b)                          # two identical calls
        assert torch.equal(a[:16], c)                     # the first point group does not see the others


@pytest.mark.parametrize('case', [(100, 21, 14, 37), (300, 21, 7, 19), (20, 19, 6, 37)], ids=str)
def test_output_covariance_is_symmetric_and_positive(case):
    fcov = _run(case)[1].cpu().numpy()
    assert np.array_equal(fcov, np.transpose(fcov, (0, 2, 1)))
    lam = np.linalg.eigvalsh(fcov)
    print('%s smallest eigenvalue / largest entry: %.2e' % (case, (lam.min(axis=1) / np.abs(fcov).max(axis=(1, 2))).min()))
    assert (lam.min(axis=1) >= -1e-12 * np.abs(fcov).max(axis=(1, 2))).all()


@pytest.mark.parametrize('case', mc.TRANSITION_CASES, ids=str)
def test_transition_moments(case):
    M, D, Do, npts = case
    p, mean, cov, _ = mc.make_beliefs(M, D, Do, npts, 'transition')
    gp = _model(p, M, D, Do)
    h, P = _dev(mean[:, :Do]), _dev(cov[:, :Do, :Do])
    a = _dev(mean[:, Do:]) if D > Do else None
    mn, Pn, cross, info = gp.transition_moments(h, P, a)
    mr, Pr, cr = mc.transition_reference(*case)
    assert not info.cpu().numpy().any() and not mn.requires_grad
    within_rule('%s m+' % (case,), mn.cpu().numpy(), mr, RULE)
    within_rule('%s P+' % (case,), Pn.cpu().numpy(), Pr, RULE)
    within_rule('%s cross' % (case,), cross.cpu().numpy(), cr, RULE)
    assert torch.equal(Pn, Pn.transpose(1, 2))


def test_python_surface():
    M, D, Do = 30, 7, 5
    p, mean, cov, _ = mc.make_beliefs(M, D, Do, 9)
    # no point: empty tensors of the right shapes, nothing launched
    gp = _model(p, M, D, Do)
    e = torch.empty(0, D, dtype=torch.float64, device=DEV)
    fmean, fcov, xcov, info = gp.moment_match(e, torch.empty(0, D, D, dtype=torch.float64, device=DEV))
    assert fmean.shape == (0, Do) and fcov.shape == (0, Do, Do) and xcov.shape == (0, Do, D)
    assert info.shape == (0,) and info.dtype == torch.int64
    assert gp.moment_match(e, None, cross=False)[2] is None
    # evaluation only, whatever the leaves and the inputs ask for
    gp = _model(p, M, D, Do, grad=PARAMS)
    out = gp.moment_match(_dev(mean).requires_grad_(), _dev(cov).requires_grad_())
    assert all(not t.requires_grad and t.grad_fn is None for t in out)
    _check('leaves require grad', out, mc.reference_closed_form(M, D, Do, 9))
    # full-covariance q(z): refused
    full = _model(p, M, D, Do, q_full=True)
    with pytest.raises(ValueError):
        full.moment_match(_dev(mean), _dev(cov))
    with pytest.raises(ValueError):
        full.transition_moments(_dev(mean[:, :Do]), _dev(cov[:, :Do, :Do]), _dev(mean[:, Do:]))
    # a GP whose input is narrower than its output has no recurrence
    p2, mean2, cov2, _ = mc.make_beliefs(12, 2, 3, 4)
    with pytest.raises(ValueError):
        _model(p2, 12, 2, 3).transition_moments(_dev(np.zeros((4, 3))), _dev(np.zeros((4, 3, 3))))
