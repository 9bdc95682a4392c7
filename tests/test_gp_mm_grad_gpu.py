"""The input gradients of GPModel.moment_match on the GPU: cbfssm_gp_moment_match_bwd_f64 through
cbfssm.hip.autograd.gp_moment_match and GPModel.moment_match / transition_moments(..., input_grads=True), against torch
autograd through the Gram coding of the closed form on the CPU (tests/gp_mm_grad_cases.py, reference (a), which
tests/test_gp_mm_grad_cpu.py pins to a second coding and to finite differences of the numpy closed form).

Rule: the project's for gradients -- gp_autograd_cases.within_rule at 1e-6 of the largest entry of the reference tensor.
Every check prints its figure; the figures of one run on an MI355X are in profiles/gp_moment_match_grad/parity.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

import gp_autograd_cases as gc
import gp_mm_grad_cases as gg
import gp_moment_match_cases as mc
import gp_tile_grid as grid
from gp_autograd_cases import PARAMS, within_rule

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RULE = gg.GPU_RULE


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


def _grads(fn, mean, cov, weights, variant='all', cross=True):
    """(outputs, g_mean, g_cov) of the loss of gp_mm_grad_cases through fn(mean, cov) -> (fmean, fcov, xcov, info)"""
    mt = _dev(mean).requires_grad_()
    ct = _dev(cov).requires_grad_() if cov is not None else None
    out = fn(mt, ct)
    assert out[3].grad_fn is None and not out[3].requires_grad
    assert all(t.grad_fn is not None for t in out[:3] if t is not None)
    gg.loss_of(out[:3], weights, variant).backward()
    return out, mt.grad, (ct.grad if ct is not None else None)


def _check(tag, got, ref, cov=True):
    _, gm, gcov = got
    within_rule('%s g_mean' % tag, gm.cpu().numpy(), ref['g_mean'], RULE)
    if cov:
        g = gcov.cpu().numpy()
        within_rule('%s g_cov' % tag, g, ref['g_cov'], RULE)
        iu = np.triu_indices(g.shape[-1], 1)
        assert not g[:, iu[0], iu[1]].any(), '%s: g_cov is not exactly zero above the diagonal' % tag


def _case_grads(case, kind='mixed', variant='all', fn=None, cross=True):
    M, D, Do, npts = case
    p, mean, cov, _ = mc.make_beliefs(M, D, Do, npts, kind)
    if fn is None:
        gp = _model(p, M, D, Do)
        fn = lambda m, c: gp.moment_match(m, c, cross=cross, input_grads=True)     # noqa: E731
    return _grads(fn, mean, cov, gg.make_weights(M, D, Do, npts), variant)


@pytest.mark.parametrize('name', grid.ROW_IDS)
def test_every_compiled_leaf(name):
    """one small shape per compiled (tile height, DK) leaf, three point groups with the last ragged, rank-2, full-rank and
    block beliefs in turn, in the automatic form and with the pack forced dense and two-triangular"""
    from cbfssm.hip import autograd as ag
    _, M, D, Do = grid.ROW_BY_NAME[name]
    case = (M, D, Do, mc.N_POINTS)
    ref = gg.reference(*case)
    _check('%s auto' % name, _case_grads(case), ref)
    p = mc.make_beliefs(*case)[0]
    for mode in ('dense', 'tri'):
        pack = _pack(p, M, D, Do, mode)
        _check('%s %s' % (name, mode), _case_grads(case, fn=lambda m, c: ag.gp_moment_match(pack, m, c)), ref)


@pytest.mark.parametrize('case', mc.EDGE_CASES, ids=str)
def test_edges(case):
    _check(str(case), _case_grads(case), gg.reference(*case))


@pytest.mark.parametrize('case', mc.LONG_CASES, ids=str)
def test_second_trip_of_the_persistent_loop(case):
    """more point groups than workgroups at every tile height: period-37 beliefs and weights"""
    M, D, Do, npts = case
    assert (npts + 15) // 16 > grid.max_workgroups(grid.leaf_key(M, D, Do)[0])
    _check('long %s' % (case,), _case_grads(case), gg.reference(*case))


@pytest.mark.parametrize('kind,case', [('zero', (100, 21, 14, 19)), ('rank1', mc.RANK1_CASE), ('block', (130, 21, 14, 19))],
                         ids=['zero', 'rank1', 'block'])
def test_belief_kinds(kind, case):
    """cov of zeros is an ordinary input (its gradient is not zero); rank one; block"""
    got = _case_grads(case, kind)
    ref = gg.reference(*case, kind)
    _check('%s %s' % (kind, case), got, ref)
    assert np.abs(got[2].cpu().numpy()).max() > 0.0


def test_wide_belief():
    """eigenvalues of the covariance around 1e4 squared lengthscales: the reference gradients are 3e-14 and 6e-18 in size,
    so they are asserted finite and below 1e-9 in magnitude, not by the relative rule"""
    _, gm, gcov = _case_grads(mc.WIDE_CASE, 'wide')
    ref = gg.reference(*mc.WIDE_CASE, 'wide')
    gm, gcov = gm.cpu().numpy(), gcov.cpu().numpy()
    print('wide: |g_mean| %.2e (reference %.2e), |g_cov| %.2e (reference %.2e)'
          % (np.abs(gm).max(), np.abs(ref['g_mean']).max(), np.abs(gcov).max(), np.abs(ref['g_cov']).max()))
    assert np.isfinite(gm).all() and np.isfinite(gcov).all()
    assert np.abs(gm).max() < 1e-9 and np.abs(gcov).max() < 1e-9


@pytest.mark.parametrize('variant', ['fmean', 'fcov', 'xcov'])
@pytest.mark.parametrize('case', [(100, 21, 14, 19), (180, 6, 2, 19)], ids=str)
def test_partial_losses_pass_null_cotangents(case, variant):
    _check('%s %s' % (variant, case), _case_grads(case, variant=variant), gg.reference(*case, 'mixed', variant))


@pytest.mark.parametrize('case', [(100, 21, 14, 19), (113, 9, 1, 17)], ids=str)
def test_without_the_cross_covariance(case):
    got = _case_grads(case, variant='nocross', cross=False)
    assert got[0][2] is None
    _check('nocross %s' % (case,), got, gg.reference(*case, 'mixed', 'nocross'))


def test_symmetric_and_antisymmetric_weights_of_fcov():
    """a symmetric Wc gives the reference's answer; an antisymmetric one contributes nothing (fcov is symmetric)"""
    case = (100, 21, 14, 19)
    M, D, Do, npts = case
    p, mean, cov, _ = mc.make_beliefs(*case)
    Wf, Wc, Wx = gg.make_weights(*case)
    gp = _model(p, M, D, Do)
    fn = lambda m, c: gp.moment_match(m, c, input_grads=True)     # noqa: E731
    sym, anti = 0.5 * (Wc + np.transpose(Wc, (0, 2, 1))), 0.5 * (Wc - np.transpose(Wc, (0, 2, 1)))
    ref = gg.evaluate(p, mean, cov, (Wf, sym, Wx), 'fcov')
    _check('symmetric Wc', _grads(fn, mean, cov, (Wf, sym, Wx), 'fcov'), ref)
    _, gm, gcov = _grads(fn, mean, cov, (Wf, anti, Wx), 'fcov')
    scale = max(np.abs(ref['g_mean']).max(), np.abs(ref['g_cov']).max())
    print('antisymmetric Wc: |g_mean| %.2e |g_cov| %.2e of %.2e' % (gm.abs().max(), gcov.abs().max(), scale))
    assert gm.abs().max() < RULE * scale and gcov.abs().max() < RULE * scale
    # and with the other two results in the loss the antisymmetric part changes nothing beyond rounding
    ref_all = gg.evaluate(p, mean, cov, (Wf, sym, Wx), 'all')
    _check('Wf, antisymmetric + symmetric Wc, Wx', _grads(fn, mean, cov, (Wf, Wc, Wx), 'all'), ref_all)


@pytest.mark.parametrize('case', [(100, 21, 14, 19), (200, 13, 7, 19)], ids=str)
def test_without_a_covariance_the_gradient_is_that_of_predict(case):
    """cov=None: g_mean under Wf and a diagonal Wc equals gp_predict's g_X for gmean = Wf, gvar = diag Wc (a device
    cross-check), and under Wf alone einsum(Wf, linearize(...).dmean); both also against (a)"""
    M, D, Do, npts = case
    p, mean, _, _ = mc.make_beliefs(M, D, Do, npts, 'zero')
    Wf, Wc, Wx = gg.make_weights(*case)
    Wd = Wc * np.eye(Do)[None]
    gp = _model(p, M, D, Do)
    fn = lambda m, c: gp.moment_match(m, None, input_grads=True)     # noqa: E731
    out, gm, gcov = _grads(fn, mean, None, (Wf, Wd, Wx), 'nocross')
    assert gcov is None
    within_rule('%s cov=None vs (a)' % (case,), gm.cpu().numpy(), gg.evaluate(p, mean, None, (Wf, Wd, Wx), 'nocross')['g_mean'], RULE)
    X = _dev(mean).requires_grad_()
    fmean, fvar = gp.predict(X)
    ((_dev(Wf) * fmean).sum() + (_dev(np.einsum('ndd->nd', Wc)) * fvar).sum()).backward()
    within_rule('%s cov=None vs gp_predict g_X' % (case,), gm.cpu().numpy(), X.grad.cpu().numpy(), RULE)
    _, gm1, _ = _grads(fn, mean, None, (Wf, Wd, Wx), 'fmean')
    dmean = gp.linearize(_dev(mean), variance=False)[2]
    lin = torch.einsum('nd,ndi->ni', _dev(Wf), dmean)
    within_rule('%s cov=None vs linearize' % (case,), gm1.cpu().numpy(), lin.cpu().numpy(), RULE)


@pytest.mark.parametrize('name', grid.CHAIN_GROUP_ROWS)
def test_bitwise_properties(name):
    """forward values under grad equal the evaluation call; two backward calls are equal; points 0..15 of a 37-point call
    equal the same points of a 16-point call; g_cov above the diagonal is exactly 0.0"""
    _, M, D, Do = grid.ROW_BY_NAME[name]
    case = (M, D, Do, mc.N_POINTS)
    p, mean, cov, _ = mc.make_beliefs(*case)
    W = gg.make_weights(*case)
    gp = _model(p, M, D, Do)
    fn = lambda m, c: gp.moment_match(m, c, input_grads=True)     # noqa: E731
    out, gm, gcov = _grads(fn, mean, cov, W)
    for a, b in zip(out, gp.moment_match(_dev(mean), _dev(cov))):
        assert torch.equal(a.detach(), b)
    _, gm2, gcov2 = _grads(fn, mean, cov, W)
    assert torch.equal(gm, gm2) and torch.equal(gcov, gcov2)
    _, gmh, gcovh = _grads(fn, mean[:16], cov[:16], tuple(w[:16] for w in W))
    assert torch.equal(gm[:16], gmh) and torch.equal(gcov[:16], gcovh)
    assert torch.equal(torch.triu(gcov, 1), torch.zeros_like(gcov))
    assert not torch.signbit(torch.triu(gcov, 1)).any()


@pytest.mark.parametrize('case', [(100, 21, 14, 37), (180, 6, 2, 37)], ids=str)
def test_poisoned_buffers_through_the_c_abi(case):
    """gmean, gcov and work pre-filled with NaN: the results are those of the autograd path, bitwise"""
    from cbfssm.hip import lib as hl
    from cbfssm.hip.ops import _ptr, _stream
    M, D, Do, npts = case
    p, mean, cov, _ = mc.make_beliefs(*case)
    W = gg.make_weights(*case)
    pack = _pack(p, M, D, Do, 'dense')
    from cbfssm.hip import autograd as ag
    _, gm, gcov = _grads(lambda m, c: ag.gp_moment_match(pack, m, c), mean, cov, W)
    lib, lay = hl.load(), pack.layout
    nwork = int(lib.cbfssm_gp_moment_match_bwd_work_elems(C.byref(lay)))
    nan = float('nan')
    work = torch.full((nwork,), nan, dtype=torch.float64, device=DEV)
    gm2, gcov2 = torch.full((npts, D), nan, dtype=torch.float64, device=DEV), torch.full((npts, D, D), nan, dtype=torch.float64, device=DEV)
    info = torch.full((npts,), nan, dtype=torch.float64, device=DEV)
    m, c, (wf, wc, wx) = _dev(mean), _dev(cov), (_dev(w) for w in W)
    hl.check(lib.cbfssm_gp_moment_match_bwd_f64(C.byref(lay), _ptr(pack.buf), _ptr(m), _ptr(c), npts, _ptr(wf), _ptr(wc), _ptr(wx),
                                                _ptr(gm2), _ptr(gcov2), _ptr(info), _ptr(work), _stream()), 'bwd')
    assert torch.equal(gm, gm2) and torch.equal(gcov, gcov2) and not info.cpu().numpy().any()


def test_an_indefinite_covariance_is_flagged_and_stays_alone():
    M, D, Do, npts = 100, 21, 14, 19
    p, mean, cov, _ = mc.make_beliefs(M, D, Do, npts)
    W = gg.make_weights(M, D, Do, npts)
    gp = _model(p, M, D, Do)
    fn = lambda m, c: gp.moment_match(m, c, input_grads=True)     # noqa: E731
    _, gm, gcov = _grads(fn, mean, cov, W)
    bad_cov = cov.copy()
    bad_cov[7] = -3.0 * np.eye(D) * mc.softplus(p['lengthscales_unc']) ** 2          # I + S~ = -2 I: the first pivot fails
    mt, ct = _dev(mean).requires_grad_(), _dev(bad_cov).requires_grad_()
    out = fn(mt, ct)
    info = out[3].cpu().numpy()
    assert info[7] != 0 and not np.delete(info, 7).any()
    keep = torch.tensor(np.delete(np.arange(npts), 7), device=DEV)
    # the loss over the well-formed points only: the NaN results of point 7 are not in it, its cotangents are zero
    Wk = tuple(_dev(w)[keep] for w in W)
    gg.loss_of(tuple(t[keep] for t in out[:3]), Wk).backward()
    assert torch.isnan(mt.grad[7]).all() and torch.isnan(ct.grad[7]).all()
    assert torch.equal(mt.grad[keep], gm[keep]) and torch.equal(ct.grad[keep], gcov[keep])


def test_python_surface():
    M, D, Do = 30, 7, 5
    p, mean, cov, _ = mc.make_beliefs(M, D, Do, 9)
    W = gg.make_weights(M, D, Do, 9)
    # the default keyword still gives no grad_fn
    gp = _model(p, M, D, Do, grad=PARAMS)
    out = gp.moment_match(_dev(mean).requires_grad_(), _dev(cov).requires_grad_())
    assert all(not t.requires_grad and t.grad_fn is None for t in out)
    # input_grads=True without a gradient request is the evaluation call
    out = gp.moment_match(_dev(mean), _dev(cov), input_grads=True)
    assert all(t.grad_fn is None for t in out)
    with torch.no_grad():
        out = gp.moment_match(_dev(mean).requires_grad_(), _dev(cov), input_grads=True)
    assert all(t.grad_fn is None for t in out)
    # the model is a constant of the call: leaves that require grad end with .grad None, and are not connected
    mt, ct = _dev(mean).requires_grad_(), _dev(cov).requires_grad_()
    out = gp.moment_match(mt, ct, input_grads=True)
    loss = gg.loss_of(out[:3], W)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(loss, gp.parameters()[0], retain_graph=True)
    loss.backward()
    assert all(leaf.grad is None for leaf in gp.parameters()) and mt.grad is not None and ct.grad is not None
    # once differentiable, and the graph is freed: a second backward raises
    with pytest.raises(RuntimeError):
        loss.backward()
    # only one of the two inputs asks
    mt = _dev(mean).requires_grad_()
    out = gp.moment_match(mt, _dev(cov), input_grads=True)
    gg.loss_of(out[:3], W).backward()
    within_rule('mean alone', mt.grad.cpu().numpy(), gg.reference(M, D, Do, 9)['g_mean'], RULE)
    # full-covariance q(z): refused
    full = _model(p, M, D, Do, q_full=True)
    with pytest.raises(ValueError):
        full.moment_match(_dev(mean).requires_grad_(), _dev(cov), input_grads=True)
    with pytest.raises(ValueError):
        full.transition_moments(_dev(mean[:, :Do]), _dev(cov[:, :Do, :Do]), _dev(mean[:, Do:]), input_grads=True)
    # no point: empty results with a grad_fn, empty gradients, nothing launched
    gp = _model(p, M, D, Do)
    e, ec = torch.empty(0, D, dtype=torch.float64, device=DEV, requires_grad=True), torch.empty(0, D, D, dtype=torch.float64, device=DEV)
    fmean, fcov, xcov, info = gp.moment_match(e, ec, input_grads=True)
    assert fmean.shape == (0, Do) and fcov.shape == (0, Do, Do) and xcov.shape == (0, Do, D) and info.shape == (0,)
    (fmean.sum() + fcov.sum() + xcov.sum()).backward()
    assert e.grad.shape == (0, D)


def test_the_gradient_is_that_of_the_model_the_forward_saw():
    """an in-place change of a leaf and a predict in between (which prepares the pack again) do not reach the gradient"""
    M, D, Do, npts = 30, 7, 5, 9
    p, mean, cov, _ = mc.make_beliefs(M, D, Do, npts)
    W = gg.make_weights(M, D, Do, npts)
    gp = _model(p, M, D, Do)
    mt, ct = _dev(mean).requires_grad_(), _dev(cov).requires_grad_()
    out = gp.moment_match(mt, ct, input_grads=True)
    with torch.no_grad():
        gp.zeta_mean.mul_(1.7)
        gp.kern.lengthscales_unc.add_(0.3)
    gp.predict(_dev(mean))
    gg.loss_of(out[:3], W).backward()
    _check('model of the forward', (out, mt.grad, ct.grad), gg.reference(M, D, Do, npts))


def _transition_reference(p, h, P, a, fn_loss, D, Do):
    """the tensor-library steps of GPModel.transition_moments over reference (a), on the CPU"""
    c = gg.model_constants(p)
    Pl = torch.tril(P)
    Ps = Pl + torch.tril(P, -1).transpose(1, 2)
    if D == Do:
        X, S = h, Pl
    else:
        X = torch.cat([h, a], dim=1)
        S = torch.zeros(h.shape[0], D, D, dtype=torch.float64)
        S[:, :Do, :Do] = Pl
    fmean, fcov, xcov = gg.gram_moments(c, X, S)
    Cm = xcov[:, :, :Do].transpose(1, 2)
    low = torch.tril(Ps + Cm + Cm.transpose(1, 2) + fcov)
    return h + fmean, low + torch.tril(low, -1).transpose(1, 2), Ps + Cm


@pytest.mark.parametrize('case', mc.TRANSITION_CASES, ids=str)
def test_transition_moments(case):
    M, D, Do, npts = case
    p, mean, cov, _ = mc.make_beliefs(M, D, Do, npts, 'transition')
    rng = np.random.default_rng(5)
    Wm, WP, Wc = rng.standard_normal((npts, Do)), rng.standard_normal((npts, Do, Do)), rng.standard_normal((npts, Do, Do))
    res = {}
    for where in ('cpu', DEV):
        t = lambda x: torch.tensor(np.asarray(x), dtype=torch.float64, device=where).requires_grad_()     # noqa: E731
        h, P = t(mean[:, :Do]), t(cov[:, :Do, :Do])
        a = t(mean[:, Do:]) if D > Do else None
        if where == 'cpu':
            mn, Pn, cr = _transition_reference(p, h, P, a, None, D, Do)
        else:
            mn, Pn, cr, info = _model(p, M, D, Do).transition_moments(h, P, a, input_grads=True)
            assert not info.cpu().numpy().any() and mn.grad_fn is not None
        w = lambda x: torch.tensor(x, dtype=torch.float64, device=where)     # noqa: E731
        ((w(Wm) * mn).sum() + (w(WP) * Pn).sum() + (w(Wc) * cr).sum()).backward()
        res[where] = [x.grad.cpu().numpy() for x in (h, P, a) if x is not None]
    for name, g, r in zip(('g_h', 'g_P', 'g_a'), res[DEV], res['cpu']):
        within_rule('%s %s' % (case, name), g, r, RULE)


def test_three_step_chain_of_beliefs():
    """the PILCO use: h, P -> transition_moments -> ... three times with var_x added by the caller, and the gradient of a
    quadratic cost of the last belief with respect to h0, P0 and a[0..2]"""
    M, D, Do, N, T = 30, 7, 5, 5, 3
    p, mean, cov, _ = mc.make_beliefs(M, D, Do, N, 'transition')
    rng = np.random.default_rng(11)
    a_np = mean[:, Do:][None] + 0.1 * rng.standard_normal((T, N, D - Do))
    var_x = 0.01 + 0.01 * np.arange(Do)
    Wq = rng.standard_normal((Do, Do))
    Wq = Wq @ Wq.T
    target = rng.standard_normal(Do)
    res = {}
    for where in ('cpu', DEV):
        t = lambda x: torch.tensor(np.asarray(x), dtype=torch.float64, device=where)     # noqa: E731
        h0, P0, a = t(mean[:, :Do]).requires_grad_(), t(cov[:, :Do, :Do]).requires_grad_(), t(a_np).requires_grad_()
        gp = _model(p, M, D, Do) if where != 'cpu' else None
        h, P = h0, P0
        for s in range(T):
            if where == 'cpu':
                h, P, _ = _transition_reference(p, h, P, a[s], None, D, Do)
            else:
                h, P, _, info = gp.transition_moments(h, P, a[s], input_grads=True)
                assert not info.cpu().numpy().any()
            P = P + torch.diag(t(var_x))
        e = h - t(target)
        cost = (torch.einsum('ni,ij,nj->n', e, t(Wq), e) + torch.einsum('ij,nij->n', t(Wq), P)).sum()    # E[(x - t)^T Wq (x - t)]
        cost.backward()
        res[where] = [cost.item()] + [x.grad.cpu().numpy() for x in (h0, P0, a)]
    print('chain cost: %.15g (reference %.15g)' % (res[DEV][0], res['cpu'][0]))
    assert abs(res[DEV][0] - res['cpu'][0]) <= 1e-8 * abs(res['cpu'][0])
    for name, g, r in zip(('g_h0', 'g_P0', 'g_a'), res[DEV][1:], res['cpu'][1:]):
        within_rule('chain %s' % name, g, r, RULE)
