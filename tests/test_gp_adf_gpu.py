"""GPModel.adf and GPModel.ads on the GPU: cbfssm_gp_adf_f64 / cbfssm_gp_ads_f64 through cbfssm.hip.autograd and
cbfssm.model.gp_tf.GPModel, against reference (b) of tests/gp_adf_cases.py (gp_moment_match_cases.closed_form per step and
the sequential scalar updates) and the numpy RTS sweep over it.  Rule: every entry of means, covs, loglik, pmeans, pcovs and
cross within 1e-8 of the largest entry of the reference tensor; the strictly lower triangle of covs separately against its
own largest entry where Do > 1; a reference log-likelihood of exactly zero must be met exactly.  Every check prints its
figure.

The cross-checks on the device compare two evaluations of the same closed form by two kernels: one step against
GPModel.transition_moments to 1e-10, a Python loop of transition_moments plus tensor-library updates against one adf call
to 1e-9, the S = 0 first step against predict to 1e-12.

Measured on an MI355X: profiles/gp_adf/parity.txt."""
import numpy as np
import pytest
import torch

import gp_adf_cases as ac
import gp_tile_grid as grid
from gp_autograd_cases import PARAMS
from test_gp_ekf_gpu import _dev, _model, _pack, _args

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RULE = 1e-8


def _adf(c, **over):
    M, D, Do = c[:3]
    args, cond = _args(c, **over)
    return _model(ac.make_inputs(c)['p'], M, D, Do).adf(*args, cond=cond)


def _ads(c, lag_one, **over):
    M, D, Do = c[:3]
    args, cond = _args(c, **over)
    return _model(ac.make_inputs(c)['p'], M, D, Do).ads(*args, cond=cond, lag_one=lag_one)


def _figure(c, tag, k, g, r, rule):
    assert g.shape == r.shape, (k, g.shape, r.shape)
    assert np.all(np.isfinite(g)), (c, tag, k)
    scale = np.abs(r).max()
    if scale == 0.0:
        assert np.all(g == 0.0), (c, tag, k)
        return 0.0
    err = float(np.abs(g - r).max() / scale)
    print('%s %-5s %-9s max|ref| %.3e  err/max %.2e' % (c, tag, k, scale, err))
    assert err < rule, (c, tag, k, err)
    return err


def _check(c, out, tag, ref=None, rule=RULE):
    ref = ac.reference_sequential(c) if ref is None else ref
    for k in ac.KEYS:
        _figure(c, tag, k, getattr(out, k).cpu().numpy(), ref[k], rule)
    if c[2] > 1:
        _figure(c, tag, 'covs.low', ac.mc.lower(out.covs.cpu().numpy()), ac.mc.lower(ref['covs']), rule)
    assert out.info.dtype == torch.int64 and not out.info.any(), (c, tag)


def _symmetric_psd(out):
    for covs in (out.covs, out.pcovs):
        assert torch.equal(covs, covs.transpose(2, 3))                   # bitwise symmetric
        assert float(torch.linalg.eigvalsh(covs.cpu()).min()) >= -1e-12 * float(covs.abs().max())


# ---- every compiled leaf
@pytest.mark.parametrize('name', [r[0] for r in ac.GRID_ROWS])
def test_every_compiled_leaf_against_the_closed_form(name):
    """one small shape per compiled (tile height, DK) leaf, two chain groups with the second ragged, a random mask with NaN in
    y, in the form the automatic switch picks and with the pack forced to dense and to two-triangular"""
    c = ac.ec.grid_case(grid.ROW_BY_NAME[name])
    M, D, Do = c[:3]
    from cbfssm.hip import autograd as ag
    out = _adf(c)
    _check(c, out, 'auto')
    _symmetric_psd(out)
    args, cond = _args(c)
    p = ac.make_inputs(c)['p']
    for mode in ('dense', 'tri'):
        _check(c, ag.gp_adf_eval(_pack(p, M, D, Do, mode), *args, cond=cond), mode)


# ---- masks and edges
@pytest.mark.parametrize('c', ac.MASK_CASES + ac.EDGE_CASES, ids=str)
def test_masks_and_edges_against_the_closed_form(c):
    out = _adf(c)
    _check(c, out, 'auto')
    _symmetric_psd(out)


# ---- cross-checks on the device
def _cross(name, g, r, rule):
    err = float((g - r).abs().max() / r.abs().max())
    print('%-52s max|ref| %.3e  err/max %.2e' % (name, float(r.abs().max()), err))
    assert err <= rule, (name, err)


def test_one_free_step_is_transition_moments():
    c = ac.case(100, 21, 14, T=1, mask='zeros')
    M, D, Do = c[:3]
    (m0, P0, a, y, var_x, var_y), cond = _args(c)
    gp = _model(ac.make_inputs(c)['p'], M, D, Do)
    out = gp.adf(m0, P0, a, y, var_x, var_y, cond=cond)
    mp, Pp, cross, info = gp.transition_moments(m0, P0, a[0])
    assert not info.any()
    _cross('pmeans[0] = m+', out.pmeans[0], mp, 1e-10)
    _cross('pcovs[0] = P+ + diag(var_x)', out.pcovs[0], Pp + torch.diag_embed(var_x.expand(c[3], Do)), 1e-10)
    _cross('cross[0] = (P + Cov(h, f))^T', out.cross[0], cross.transpose(1, 2), 1e-10)
    assert torch.equal(out.means, out.pmeans) and torch.equal(out.covs, out.pcovs)
    assert torch.equal(out.loglik, torch.zeros_like(out.loglik))


def loop_of_transition_moments(gp, m0, P0, a, y, var_x, var_y, cond):
    """the per-step loop a caller writes without adf: transition_moments plus the scalar updates in the tensor library"""
    T, N, Dy = y.shape
    Do = m0.shape[1]
    m, P = m0.clone(), (P0.clone() if P0 is not None else torch.zeros(N, Do, Do, dtype=torch.float64, device=m0.device))
    ll = torch.zeros(N, dtype=torch.float64, device=m0.device)
    means, covs = [], []
    for t in range(T):
        m, P, _, _ = gp.transition_moments(m, P, None if a is None else a[t])
        if var_x is not None:
            P = P + torch.diag_embed(var_x.expand(N, Do))
        on = torch.ones(N, dtype=torch.bool, device=m0.device) if cond is None else cond[t] != 0
        for j in range(Dy):
            s = P[:, j, j] + var_y[j]
            dl = y[t, :, j] - m[:, j]
            g = P[:, :, j] / s[:, None]
            m = torch.where(on[:, None], m + g * dl[:, None], m)
            P = torch.where(on[:, None, None], P - s[:, None, None] * g[:, :, None] * g[:, None, :], P)
            ll = torch.where(on, ll - 0.5 * (torch.log(2.0 * np.pi * s) + dl * dl / s), ll)
        means.append(m)
        covs.append(P)
    return torch.stack(means), torch.stack(covs), ll


def test_a_loop_of_transition_moments_is_one_call():
    c = ac.case(100, 21, 14)
    M, D, Do = c[:3]
    (m0, P0, a, y, var_x, var_y), cond = _args(c)
    gp = _model(ac.make_inputs(c)['p'], M, D, Do)
    out = gp.adf(m0, P0, a, y, var_x, var_y, cond=cond)
    means, covs, ll = loop_of_transition_moments(gp, m0, P0, a, y, var_x, var_y, cond)
    _cross('means', out.means, means, 1e-9)
    _cross('covs', out.covs, covs, 1e-9)
    _cross('loglik', out.loglik, ll, 1e-9)


def test_the_first_step_from_a_point_belief_is_predict():
    c = ac.case(100, 21, 14, mask='zeros')
    M, D, Do = c[:3]
    (m0, _, a, y, var_x, var_y), cond = _args(c)
    gp = _model(ac.make_inputs(c)['p'], M, D, Do)
    out = gp.adf(m0, None, a, y, None, var_y, cond=cond)
    fmean, fvar = gp.predict(torch.cat([m0, a[0]], 1))
    _cross('pmeans[0] = m0 + fmean', out.pmeans[0], m0 + fmean, 1e-12)
    _cross('pcovs[0] = diag(fvar)', out.pcovs[0], torch.diag_embed(fvar), 1e-12)
    assert torch.equal(out.cross[0], torch.zeros_like(out.cross[0]))


# ---- properties
@pytest.mark.parametrize('c', [ac.case(100, 21, 14), ac.case(200, 13, 7)], ids=str)
def test_two_calls_are_bitwise_equal(c):
    for x, z in zip(_adf(c), _adf(c)):
        assert torch.equal(x, z)


@pytest.mark.parametrize('M,D,Do', ac.CHAIN_GROUP_SHAPES)
def test_the_first_chain_group_does_not_see_the_second(M, D, Do):
    c = ac.case(M, D, Do)
    i = ac.make_inputs(c)
    head = {k: (None if i[k] is None else np.ascontiguousarray(i[k][:, :16])) for k in ('a', 'y', 'cond')}
    head.update(m0=i['m0'][:16].copy(), P0=i['P0'][:16].copy())
    full, part = _adf(c), _adf(c, **head)
    assert part.means.shape[1] == 16
    for k in ('means', 'covs', 'pmeans', 'pcovs', 'cross'):
        assert torch.equal(getattr(full, k)[:, :16], getattr(part, k)), k
    assert torch.equal(full.loglik[:16], part.loglik) and torch.equal(full.info[:16], part.info)


def test_nothing_conditioned_reads_no_observation():
    c = ac.case(30, 7, 5, mask='zeros')
    i = ac.make_inputs(c)
    out = _adf(c)
    nan = _adf(c, y=np.full_like(i['y'], np.nan))
    assert torch.equal(out.loglik, torch.zeros_like(out.loglik))
    for x, z in zip(out, nan):
        assert torch.isfinite(z).all() and torch.equal(x, z)


def test_unobserved_entries_reach_no_output():
    """the NaNs of y where cond = 0 replaced by other values: no output bit changes"""
    c = ac.case(100, 12, 9)
    i = ac.make_inputs(c)
    assert np.isnan(i['y']).any()
    for x, z in zip(_adf(c), _adf(c, y=np.where(np.isnan(i['y']), 123.456, i['y']))):
        assert torch.equal(x, z)


# ---- info
def test_a_failed_factorisation_is_flagged_and_stays_in_its_chain():
    c, n = ac.FAIL_CASE, ac.FAIL_CHAIN
    good, bad = _adf(c), _adf(c, P0=ac.fail_P0())
    expect = torch.zeros(c[3], dtype=torch.int64, device=DEV)
    expect[n] = 1
    assert torch.equal(bad.info, expect) and not good.info.any()
    keep = [k for k in range(c[3]) if k != n]
    for k in ('means', 'covs', 'pmeans', 'pcovs', 'cross'):
        g, b = getattr(good, k), getattr(bad, k)
        assert torch.isnan(b[:, n]).all(), k
        assert torch.equal(g[:, keep], b[:, keep]), k
    assert torch.isnan(bad.loglik[n]) and torch.equal(good.loglik[keep], bad.loglik[keep])
    _check(c, good, 'good')
    # the smoother: the forward pass's info, NaN throughout for that chain, the others bitwise
    sg, sb = _ads(c, True), _ads(c, True, P0=ac.fail_P0())
    assert torch.equal(sb.info, expect) and not sg.info.any()
    idx = torch.tensor(keep, device=DEV)
    for k in ('smeans', 'scovs', 'init_mean', 'init_cov', 'lag_one'):
        g, b = getattr(sg, k), getattr(sb, k)
        ax = 0 if k.startswith('init') else 1                           # the chain axis
        assert torch.isnan(b.select(ax, n)).all(), k
        assert torch.equal(g.index_select(ax, idx), b.index_select(ax, idx)), k


# ---- the smoother
@pytest.mark.parametrize('c', ac.ADS_CASES, ids=str)
def test_ads_against_the_rts_sweep(c):
    ref = ac.reference_rts(c)
    fwd = _adf(c)
    for lag_one in (False, True):
        out = _ads(c, lag_one)
        for k in ('means', 'covs', 'loglik', 'pmeans', 'pcovs'):
            assert torch.equal(getattr(out, k), getattr(fwd, k)), k       # bitwise adf's
        for k in ('smeans', 'scovs', 'init_mean', 'init_cov') + (('lag_one',) if lag_one else ()):
            _figure(c, 'ads', k, getattr(out, k).cpu().numpy(), ref[k], RULE)
        assert (out.lag_one is None) == (not lag_one)
        assert torch.equal(out.scovs, out.scovs.transpose(2, 3)) and torch.equal(out.init_cov, out.init_cov.transpose(1, 2))
        assert out.info.dtype == torch.int64 and not out.info.any()


def test_ads_with_nothing_conditioned_is_the_filter():
    c = ac.case(30, 7, 5, mask='zeros')
    out = _ads(c, False)
    _cross('smeans = means', out.smeans, out.means, 1e-10)
    _cross('scovs = covs', out.scovs, out.covs, 1e-10)
    i = ac.make_inputs(c)
    _cross('init_mean = m0', out.init_mean, _dev(i['m0']), 1e-10)
    _cross('init_cov = P0', out.init_cov, _dev(i['P0']), 1e-10)


# ---- surface
def test_python_surface():
    c = ac.case(30, 7, 5)
    M, D, Do, N, T, Dy = c[:6]
    p = ac.make_inputs(c)['p']
    (m0, P0, a, y, var_x, var_y), cond = _args(c)
    gp = _model(p, M, D, Do)
    # no chain, no step: empty tensors of the right shapes, zeros for loglik and info
    for call in (gp.adf, gp.ads):
        out = call(m0[:0], P0[:0], a[:, :0], y[:, :0], var_x, var_y, cond=cond[:, :0])
        assert out.means.shape == (T, 0, Do) and out.covs.shape == (T, 0, Do, Do) and out.loglik.shape == (0,)
        assert out.pmeans.shape == (T, 0, Do) and out.pcovs.shape == (T, 0, Do, Do) and out.info.shape == (0,)
        out = call(m0, P0, a[:0], y[:0], var_x, var_y, cond=cond[:0])
        assert out.means.shape == (0, N, Do) and out.covs.shape == (0, N, Do, Do) and out.pcovs.shape == (0, N, Do, Do)
        assert torch.equal(out.loglik, torch.zeros(N, dtype=torch.float64, device=DEV))
        assert torch.equal(out.info, torch.zeros(N, dtype=torch.int64, device=DEV))
    assert gp.adf(m0, P0, a[:0], y[:0], var_x, var_y, cond=cond[:0]).cross.shape == (0, N, Do, Do)
    out = gp.ads(m0, P0, a[:0], y[:0], var_x, var_y, cond=cond[:0], lag_one=True)
    assert out.smeans.shape == (0, N, Do) and out.init_cov.shape == (N, Do, Do) and out.lag_one.shape == (0, N, Do, Do)
    # evaluation only, whatever the leaves and the inputs ask for
    gp = _model(p, M, D, Do, grad=PARAMS)
    req = lambda t: t.clone().requires_grad_()
    out = gp.adf(req(m0), req(P0), req(a), y, req(var_x), req(var_y), cond=cond)
    assert all(not t.requires_grad and t.grad_fn is None for t in out)
    _check(c, out, 'leaves require grad')
    out = gp.ads(req(m0), req(P0), req(a), y, req(var_x), req(var_y), cond=cond, lag_one=True)
    assert all(not t.requires_grad and t.grad_fn is None for t in out)
    # full-covariance q(z): refused; fewer inputs than outputs: refused
    for call in ('adf', 'ads'):
        with pytest.raises(ValueError):
            getattr(_model(p, M, D, Do, q_full=True), call)(m0, P0, a, y, var_x, var_y, cond=cond)
    Mr, Dr, Dor = ac.ec.ILL_REFUSED
    import gp_autograd_cases as gc
    pr = gc.make_inputs(Mr, Dr, Dor, 1)[0]
    z = torch.zeros
    for call in ('adf', 'ads'):
        with pytest.raises(ValueError):
            getattr(_model(pr, Mr, Dr, Dor), call)(z(3, Dor, device=DEV), None, None, z(2, 3, 1, device=DEV), None,
                                                   z(1, device=DEV) + 0.1)
