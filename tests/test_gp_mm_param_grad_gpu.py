"""The leaf gradients of GPModel.moment_match on the GPU: cbfssm_gp_moment_match_params_bwd_f64 and the unchanged tail through
cbfssm.hip.autograd.gp_moment_match_params and GPModel.moment_match / transition_moments(..., differentiable=True), against
torch autograd FROM THE FIVE UNCONSTRAINED LEAVES through the Gram coding of the closed form on the CPU
(tests/gp_mm_param_grad_cases.py, reference (a), which tests/test_gp_mm_param_grad_cpu.py pins to a second coding, to the
numpy adjoint and to finite differences).

Rule: the project's for gradients -- gp_autograd_cases.within_rule at 1e-6 of the largest entry of the reference tensor, per
gradient tensor: the five leaves, `mean` and `cov`.  One exception, with its reason: fmean and xcov do not depend on the
signal variance but for the jitter (alpha ~ 1 / v, q ~ v), so under a loss of fmean or xcov alone the reference's variance
gradient is 1e-8 in size -- the difference of two terms (through K_mm, and the direct one) that are each of the size of
the variance gradient of the full loss.  Rounding is relative to those terms, so that entry is held to 1e-6 of the full
loss's variance gradient.  Every check prints its figure; the figures of one run on an MI355X are in
profiles/gp_moment_match_param_grad/parity.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

import gp_autograd_cases as gc
import gp_mm_grad_cases as gg
import gp_mm_param_grad_cases as pc
import gp_moment_match_cases as mc
import gp_surface_poison as gsp
import gp_tile_grid as grid
from gp_autograd_cases import PARAMS, within_rule
from test_gp_mm_grad_gpu import _dev, _model, _pack

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RULE = pc.GPU_RULE
FORM_ROWS = ['nb1_mid_dk6', 'nb2_first_dk4', 'nb4_mid_dk4', 'nb7_kt3_dk6', 'nb10_first_dk2', 'nb13_fill_dk6', 'nb16_mid_dk4',
             'nb20_mid_dk6']


def _grads(fn, leaves, mean, cov, weights, variant='all', want=('leaves', 'mean', 'cov')):
    """(outputs, {name: gradient}) of the loss of gp_mm_grad_cases through fn(mean, cov) -> (fmean, fcov, xcov, info)"""
    for t in leaves:
        t.grad = None
        t.requires_grad_('leaves' in want)
    mt = _dev(mean).requires_grad_('mean' in want)
    ct = _dev(cov).requires_grad_('cov' in want) if cov is not None else None
    out = fn(mt, ct)
    assert out[3].grad_fn is None and not out[3].requires_grad
    assert all(t.grad_fn is not None for t in out[:3] if t is not None)
    gg.loss_of(out[:3], weights, variant).backward()
    g = {'g_' + k: t.grad for k, t in zip(PARAMS, leaves)}
    g['g_mean'], g['g_cov'] = mt.grad, (ct.grad if ct is not None else None)
    return out, g


def _check(tag, g, ref, names=None, var_scale=None):
    worst = 0.0
    for k in names or (['g_' + n for n in PARAMS] + ['g_mean'] + (['g_cov'] if ref.get('g_cov') is not None else [])):
        got = g[k].cpu().numpy().reshape(np.shape(ref[k]))
        if k == 'g_variance_unc' and var_scale is not None:
            err = np.abs(got - ref[k]).max() / var_scale
            print('%-34s held to the full loss: err/scale %.2e' % ('%s %s' % (tag, k), err))
            assert np.isfinite(got).all() and err < RULE, (tag, k, err)
        elif not np.any(ref[k]):                      # (a tensor the loss does not reach: exactly zero, not small)
            assert not got.any(), (tag, k, 'the reference is exactly zero')
            err = 0.0
        else:
            err = within_rule('%s %s' % (tag, k), got, ref[k], RULE)
        worst = max(worst, err)
    if g.get('g_cov') is not None:
        gcov = g['g_cov'].cpu().numpy()
        iu = np.triu_indices(gcov.shape[-1], 1)
        assert not gcov[:, iu[0], iu[1]].any(), '%s: g_cov is not exactly zero above the diagonal' % tag
    return worst


def _case(case, kind='mixed', variant='all', cross=True, pack_mode=None, want=('leaves', 'mean', 'cov')):
    from cbfssm.hip import autograd as ag
    M, D, Do, npts = case
    p, mean, cov, weights = pc.case_inputs(M, D, Do, npts, kind)
    gp = _model(p, M, D, Do)
    leaves = gp.parameters()
    if pack_mode is None:
        fn = lambda m, c: gp.moment_match(m, c, cross=cross, differentiable=True)     # noqa: E731
    else:
        from cbfssm.hip import ops
        pack = ops.GPPack(M, D, Do, torch.device(DEV), form_mode=pack_mode)
        fn = lambda m, c: ag.gp_moment_match_params(pack, m, c, *leaves, cross=cross)     # noqa: E731
    return _grads(fn, leaves, mean, cov, weights, variant, want)


@pytest.mark.parametrize('name', grid.ROW_IDS)
def test_every_grid_row(name):
    """one small shape per (tile height, DK) leaf of the layouts, three belief kinds in turn, the automatic form"""
    _, M, D, Do = grid.ROW_BY_NAME[name]
    case = (M, D, Do, mc.N_POINTS)
    _check(name, _case(case)[1], pc.reference(*case))


@pytest.mark.parametrize('mode', ['dense', 'tri'])
@pytest.mark.parametrize('name', FORM_ROWS)
def test_both_pack_forms(name, mode):
    _, M, D, Do = grid.ROW_BY_NAME[name]
    case = (M, D, Do, mc.N_POINTS)
    _check('%s %s' % (name, mode), _case(case, pack_mode=mode)[1], pc.reference(*case))


def test_the_form_rows_cover_every_tile_height():
    assert sorted(grid.leaf_key(*grid.ROW_BY_NAME[n][1:])[0] for n in FORM_ROWS) == grid.dispatch_heights()


@pytest.mark.parametrize('shape', pc.M_EDGES + pc.SHAPE_EDGES, ids=str)
def test_edges_of_the_shape(shape):
    """M = 1, 15, 16, 17, 112, 113 (the slab / stash switch of the tail), 257; ragged D; Do = 1"""
    case = shape + (17,)
    _check(str(case), _case(case)[1], pc.reference(*case))


@pytest.mark.parametrize('npts', [1, 16, 17, 33])
def test_numbers_of_points(npts):
    case = (30, 7, 5, npts)
    _check(str(case), _case(case)[1], pc.reference(*case))


@pytest.mark.parametrize('case', mc.LONG_CASES, ids=str)
def test_more_points_than_the_persistent_caps(case):
    """beyond the workgroup cap of the input adjoint at every tile height and of the point pass here (512): the second trip.
    Period-37 beliefs and weights; the reference weighs each distinct belief by its count"""
    M, D, Do, npts = case
    assert (npts + 15) // 16 > grid.max_workgroups(grid.leaf_key(M, D, Do)[0]) and npts > 512
    _check('long %s' % (case,), _case(case)[1], pc.reference(*case))


@pytest.mark.parametrize('kind,case', [('rank1', (100, 21, 14, 19)), ('rank2', (50, 9, 2, 19)), ('full', (30, 7, 5, 19)),
                                       ('block', (130, 21, 14, 19))], ids=['rank1', 'rank2', 'full', 'block'])
def test_belief_kinds(kind, case):
    _check('%s %s' % (kind, case), _case(case, kind)[1], pc.reference(*case, kind))


@pytest.mark.parametrize('case', [(100, 21, 14, 19), (200, 13, 7, 19)], ids=str)
def test_without_a_covariance_the_leaf_gradients_are_those_of_predict(case):
    """cov=None under Wf and a diagonal Wc: the leaf gradients equal gp_predict's for gmean = Wf, gvar = diag Wc (a device
    cross-check of two different kernels), and reference (a)"""
    M, D, Do, npts = case
    p, mean, _, _ = mc.make_beliefs(M, D, Do, npts, 'zero')
    Wf, Wc, Wx = gg.make_weights(*case)
    Wd = Wc * np.eye(Do)[None]
    gp = _model(p, M, D, Do)
    leaves = gp.parameters()
    fn = lambda m, c: gp.moment_match(m, None, differentiable=True)     # noqa: E731
    out, g = _grads(fn, leaves, mean, None, (Wf, Wd, Wx), 'nocross')
    assert g['g_cov'] is None
    ref = pc.evaluate(p, mean, None, (Wf, Wd, Wx), 'nocross')
    _check('%s cov=None vs (a)' % (case,), g, ref)
    for t in leaves:
        t.grad = None
    X = _dev(mean).requires_grad_()
    fmean, fvar = gp.predict(X)
    ((_dev(Wf) * fmean).sum() + (_dev(np.einsum('ndd->nd', Wc)) * fvar).sum()).backward()
    for k, t in zip(PARAMS, leaves):
        within_rule('%s cov=None vs gp_predict g_%s' % (case, k), g['g_' + k].cpu().numpy(), t.grad.cpu().numpy(), RULE)
    within_rule('%s cov=None vs gp_predict g_X' % (case,), g['g_mean'].cpu().numpy(), X.grad.cpu().numpy(), RULE)


@pytest.mark.parametrize('variant', ['fmean', 'fcov', 'xcov'])
@pytest.mark.parametrize('case', [(100, 21, 14, 19), (180, 6, 2, 19)], ids=str)
def test_partial_losses_pass_null_cotangents(case, variant):
    ref = pc.reference(*case, 'mixed', variant)
    scale = np.abs(pc.reference(*case)['g_variance_unc']).max() if variant in ('fmean', 'xcov') else None
    _check('%s %s' % (variant, case), _case(case, variant=variant)[1], ref, var_scale=scale)


@pytest.mark.parametrize('case', [(100, 21, 14, 19), (113, 9, 1, 17)], ids=str)
def test_without_the_cross_covariance(case):
    out, g = _case(case, variant='nocross', cross=False)
    assert out[2] is None
    _check('nocross %s' % (case,), g, pc.reference(*case, 'mixed', 'nocross'))


@pytest.mark.parametrize('case', [(100, 21, 14, 19), (130, 6, 4, 19)], ids=str)
def test_only_the_leaves_or_only_the_mean(case):
    """only the leaves require grad: their gradients are the full call's, bitwise; only `mean` does: bitwise the gradient
    of input_grads=True"""
    M, D, Do, npts = case
    ref = pc.reference(*case)
    out, g = _case(case)
    _, gl = _case(case, want=('leaves',))
    assert gl['g_mean'] is None and gl['g_cov'] is None
    for k in PARAMS:
        assert torch.equal(g['g_' + k], gl['g_' + k]), k
    _check('leaves alone %s' % (case,), gl, ref, names=['g_' + n for n in PARAMS])
    _, gm = _case(case, want=('mean',))
    assert all(gm['g_' + k] is None for k in PARAMS) and gm['g_cov'] is None
    p, mean, cov, W = pc.case_inputs(*case)
    gp = _model(p, M, D, Do)
    mt = _dev(mean).requires_grad_()
    gg.loss_of(gp.moment_match(mt, _dev(cov), input_grads=True)[:3], W).backward()
    assert torch.equal(gm['g_mean'], mt.grad)


@pytest.mark.parametrize('name', ['nb13_mid_dk2', 'nb7_kt1_dk4'])
def test_bitwise_properties(name):
    """forward values under grad equal the evaluation call on that pack; two backward calls are equal"""
    _, M, D, Do = grid.ROW_BY_NAME[name]
    case = (M, D, Do, mc.N_POINTS)
    p, mean, cov, W = pc.case_inputs(*case)
    out, g = _case(case)
    gp = _model(p, M, D, Do)
    for a, b in zip(out, gp.moment_match(_dev(mean), _dev(cov))):
        assert torch.equal(a.detach(), b)
    _, g2 = _case(case)
    for k in g:
        assert torch.equal(g[k], g2[k]), k


def test_the_gradient_is_that_of_the_model_the_forward_saw():
    """the pack prepared again with other parameters between forward and backward does not reach the gradient"""
    M, D, Do, npts = 30, 7, 5, 9
    p, mean, cov, W = pc.case_inputs(M, D, Do, npts)
    gp = _model(p, M, D, Do, grad=PARAMS)
    mt, ct = _dev(mean).requires_grad_(), _dev(cov).requires_grad_()
    out = gp.moment_match(mt, ct, differentiable=True)
    with torch.no_grad():
        gp.zeta_mean.mul_(1.7)
        gp.kern.lengthscales_unc.add_(0.3)
        gp.predict(_dev(mean))
    gg.loss_of(out[:3], W).backward()
    g = {'g_' + k: t.grad for k, t in zip(PARAMS, gp.parameters())}
    g['g_mean'], g['g_cov'] = mt.grad, ct.grad
    _check('model of the forward', g, pc.reference(M, D, Do, npts))


@pytest.mark.parametrize('word', gsp.ORDER)
@pytest.mark.parametrize('case', [(100, 21, 14, 37), (180, 6, 2, 37)], ids=str)
def test_poisoned_allocations_and_pack(case, word):
    """whatever torch.empty hands out carries the poison word before the call and before backward(), and the pack is
    poisoned before the call: the gradients are those of a clean run, bitwise"""
    M, D, Do, npts = case
    p, mean, cov, W = pc.case_inputs(*case)
    _, clean = _case(case)
    gp = _model(p, M, D, Do, grad=PARAMS)
    mt, ct = _dev(mean).requires_grad_(), _dev(cov).requires_grad_()
    gsp.poison_pack(gp, gsp.WORDS[word])
    with gsp.poisoned_allocations(gsp.WORDS[word]):
        out = gp.moment_match(mt, ct, differentiable=True)
        loss = gg.loss_of(out[:3], W)
    with gsp.poisoned_allocations(gsp.WORDS[word]):
        loss.backward()
    got = {'g_' + k: t.grad for k, t in zip(PARAMS, gp.parameters())}
    got['g_mean'], got['g_cov'] = mt.grad, ct.grad
    for k in clean:
        assert torch.equal(clean[k], got[k]), (word, k)


def test_an_indefinite_covariance_makes_every_leaf_gradient_nan_and_leaves_the_other_points_alone():
    M, D, Do, npts = 100, 21, 14, 19
    p, mean, cov, W = pc.case_inputs(M, D, Do, npts)
    keep_np = np.delete(np.arange(npts), 7)
    keep = torch.tensor(keep_np, device=DEV)
    bad_cov = cov.copy()
    bad_cov[7] = -3.0 * np.eye(D) * mc.softplus(p['lengthscales_unc']) ** 2          # I + S~ = -2 I: the first pivot fails
    gp = _model(p, M, D, Do, grad=PARAMS)
    mt, ct = _dev(mean).requires_grad_(), _dev(bad_cov).requires_grad_()
    out = gp.moment_match(mt, ct, differentiable=True)
    info = out[3].cpu().numpy()
    assert info[7] != 0 and not np.delete(info, 7).any()
    Wk = tuple(_dev(w)[keep] for w in W)
    gg.loss_of(tuple(t[keep] for t in out[:3]), Wk).backward()
    for k, t in zip(PARAMS, gp.parameters()):
        assert torch.isnan(t.grad).all(), k
    assert torch.isnan(mt.grad[7]).all() and torch.isnan(ct.grad[7]).all()
    # the same call without that point is finite, and the other points' rows are its rows
    gp2 = _model(p, M, D, Do, grad=PARAMS)
    m2, c2 = _dev(mean[keep_np]).requires_grad_(), _dev(cov[keep_np]).requires_grad_()
    out2 = gp2.moment_match(m2, c2, differentiable=True)
    gg.loss_of(out2[:3], Wk).backward()
    assert all(torch.isfinite(t.grad).all() for t in gp2.parameters())
    assert torch.equal(mt.grad[keep], m2.grad) and torch.equal(ct.grad[keep], c2.grad)
    ref = pc.evaluate(p, mean[keep_np], cov[keep_np], tuple(w[keep_np] for w in W))
    g = {'g_' + k: t.grad for k, t in zip(PARAMS, gp2.parameters())}
    g['g_mean'], g['g_cov'] = m2.grad, c2.grad
    _check('without the flagged point', g, ref)


def test_python_surface():
    M, D, Do = 30, 7, 5
    p, mean, cov, W = pc.case_inputs(M, D, Do, 9)
    gp = _model(p, M, D, Do, grad=PARAMS)
    # nothing requires grad, or grad is disabled: the evaluation call
    plain = _model(p, M, D, Do)
    assert all(t.grad_fn is None for t in plain.moment_match(_dev(mean), _dev(cov), differentiable=True))
    with torch.no_grad():
        assert all(t.grad_fn is None for t in gp.moment_match(_dev(mean), _dev(cov), differentiable=True))
    # differentiable=False keeps the contract of input_grads: the leaves stay unconnected
    mt = _dev(mean).requires_grad_()
    out = gp.moment_match(mt, _dev(cov), input_grads=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(gg.loss_of(out[:3], W), gp.parameters()[0])
    # differentiable=True takes precedence over input_grads; info never carries a grad_fn; once differentiable
    out = gp.moment_match(_dev(mean), _dev(cov), input_grads=True, differentiable=True)
    assert all(t.grad_fn is not None for t in out[:3]) and out[3].grad_fn is None and out[3].dtype == torch.int64
    loss = gg.loss_of(out[:3], W)
    loss.backward()
    assert all(t.grad is not None for t in gp.parameters())
    with pytest.raises(RuntimeError):
        loss.backward()
    # full-covariance q(z): refused
    full = _model(p, M, D, Do, q_full=True)
    with pytest.raises(ValueError):
        full.moment_match(_dev(mean), _dev(cov), differentiable=True)
    with pytest.raises(ValueError):
        full.transition_moments(_dev(mean[:, :Do]), _dev(cov[:, :Do, :Do]), _dev(mean[:, Do:]), differentiable=True)
    # no point: nothing is prepared or launched, the leaf gradients are zeros
    gp = _model(p, M, D, Do, grad=PARAMS)
    buf = gp._pack.buf.clone()
    e, ec = torch.zeros(0, D, dtype=torch.float64, device=DEV), torch.zeros(0, D, D, dtype=torch.float64, device=DEV)
    fmean, fcov, xcov, info = gp.moment_match(e, ec, differentiable=True)
    assert fmean.shape == (0, Do) and fcov.shape == (0, Do, Do) and xcov.shape == (0, Do, D) and info.shape == (0,)
    (fmean.sum() + fcov.sum() + xcov.sum()).backward()
    assert torch.equal(gp._pack.buf.view(torch.int64), buf.view(torch.int64)), 'the pack was prepared without a point'
    for t in gp.parameters():
        assert t.grad is not None and not t.grad.any()


def _adf_loop(step, h, P, a, y, var_x, var_y, Dy):
    """three steps of GP-ADF with tensor-library Kalman updates on the first Dy state dimensions; returns -loglik"""
    ll = 0.0
    eye = torch.eye(h.shape[1], dtype=torch.float64, device=h.device)
    for t in range(a.shape[0]):
        h, P = step(h, P, a[t])
        P = P + torch.diag(var_x)
        Hm = eye[:Dy]
        S = Hm @ P @ Hm.T + torch.diag(var_y)
        delta = y[t] - h[:, :Dy]
        Kg = torch.linalg.solve(S, Hm @ P).transpose(1, 2)                           # P H^T S^-1
        ll = ll - 0.5 * (torch.einsum('ni,ni->n', delta, torch.linalg.solve(S, delta)) + torch.logdet(S)
                         + Dy * np.log(2.0 * np.pi)).sum()
        h = h + torch.einsum('nij,nj->ni', Kg, delta)
        P = P - Kg @ S @ Kg.transpose(1, 2)
        P = 0.5 * (P + P.transpose(1, 2))
    return -ll


def _adf_problem():
    M, D, Do, N, T, Dy = 30, 7, 5, 6, 3, 2
    p, mean, cov, _ = mc.make_beliefs(M, D, Do, N, 'transition')
    rng = np.random.default_rng(21)
    a = mean[:, Do:][None] + 0.1 * rng.standard_normal((T, N, D - Do))
    y = mean[:, :Dy][None] + 0.3 * rng.standard_normal((T, N, Dy))
    return (M, D, Do, N, T, Dy), p, mean[:, :Do], cov[:, :Do, :Do], a, y, 0.01 + 0.01 * np.arange(Do), 0.05 + 0.01 * np.arange(Dy)


def _reference_step(leaves, D, Do):
    def step(h, P, a):
        Pl = torch.tril(P)
        Ps = Pl + torch.tril(P, -1).transpose(1, 2)
        S = torch.zeros(h.shape[0], D, D, dtype=torch.float64)
        S[:, :Do, :Do] = Pl
        fmean, fcov, xcov = pc.moments_t(leaves, torch.cat([h, a], dim=1), S)
        Cm = xcov[:, :, :Do].transpose(1, 2)
        low = torch.tril(Ps + Cm + Cm.transpose(1, 2) + fcov)
        return h + fmean, low + torch.tril(low, -1).transpose(1, 2)
    return step


def test_three_step_adf_loop_trains_the_model():
    """transition_moments(differentiable=True) in a three-step ADF loop: the leaf gradients of -loglik against the same loop
    over reference (a); then twenty Adam steps on the leaves lower that loss"""
    (M, D, Do, N, T, Dy), p, h0, P0, a, y, var_x, var_y = _adf_problem()
    leaves = pc.leaf_tensors(p)
    c = lambda x: torch.tensor(np.asarray(x), dtype=torch.float64)     # noqa: E731
    ref_loss = _adf_loop(_reference_step(leaves, D, Do), c(h0), c(P0), c(a), c(y), c(var_x), c(var_y), Dy)
    ref_loss.backward()
    gp = _model(p, M, D, Do, grad=PARAMS)

    def loss_fn():
        def step(h, P, at):
            mn, Pn, _, info = gp.transition_moments(h, P, at, differentiable=True)
            return mn, Pn
        return _adf_loop(step, _dev(h0), _dev(P0), _dev(a), _dev(y), _dev(var_x), _dev(var_y), Dy)
    loss = loss_fn()
    print('adf loop -loglik: %.15g (reference %.15g)' % (loss.item(), ref_loss.item()))
    assert abs(loss.item() - ref_loss.item()) <= 1e-8 * abs(ref_loss.item())
    loss.backward()
    for k, t, r in zip(PARAMS, gp.parameters(), leaves):
        within_rule('adf loop g_%s' % k, t.grad.cpu().numpy(), r.grad.numpy(), RULE)
    opt = torch.optim.Adam(gp.parameters(), lr=0.02)
    first = loss.item()
    for _ in range(20):
        opt.zero_grad()
        loss = loss_fn()
        loss.backward()
        opt.step()
    last = loss_fn().item()
    print('twenty Adam steps: %.6f -> %.6f' % (first, last))
    assert np.isfinite(last) and last < first


def test_through_the_c_abi_with_poisoned_buffers():
    """the entry point alone on NaN-filled work, slab and dense image: two calls are bitwise identical, rows and columns
    beyond M of every image are exactly zero"""
    from cbfssm.hip import lib as hl
    from cbfssm.hip.ops import _ptr, _stream
    from cbfssm.hip import autograd as ag
    for case in [(100, 21, 14, 37), (130, 6, 4, 37)]:
        M, D, Do, npts = case
        p, mean, cov, W = pc.case_inputs(*case)
        pack = _pack(p, M, D, Do, 'dense')
        lib, lay = hl.load(), pack.layout
        params = [_dev(p[k]) for k in PARAMS]
        pflat, cflat = ag._gp_flat(params)
        m, c, (wf, wc, wx) = _dev(mean), _dev(cov), (_dev(w) for w in W)
        fmean, fcov, xcov, info = ag.gp_moment_match_eval(pack, m, c)
        nan = float('nan')
        full = lambda *s: torch.full(s, nan, dtype=torch.float64, device=DEV)     # noqa: E731
        gm, gcv = full(npts, D), full(npts, D, D)
        hl.check(lib.cbfssm_gp_moment_match_bwd_f64(C.byref(lay), _ptr(pack.buf), _ptr(m), _ptr(c), npts, _ptr(wf), _ptr(wc),
                                                    _ptr(wx), _ptr(gm), _ptr(gcv), None,
                                                    _ptr(full(int(lib.cbfssm_gp_moment_match_bwd_work_elems(C.byref(lay))))),
                                                    _stream()), 'bwd')
        nwork = int(lib.cbfssm_gp_moment_match_params_bwd_work_elems(C.byref(lay), npts))
        res = []
        for _ in range(2):
            red, dense = full(lay.rev_slab), (full(M * M) if lay.rev_stash else None)
            hl.check(lib.cbfssm_gp_moment_match_params_bwd_f64(C.byref(lay), _ptr(pack.buf), _ptr(cflat), _ptr(m), _ptr(c), npts,
                                                               _ptr(wf), _ptr(wc), _ptr(wx), _ptr(gm), _ptr(gcv), _ptr(xcov),
                                                               _ptr(red), _ptr(dense), _ptr(full(nwork)), _stream()), 'params bwd')
            res.append((red, dense))
        assert torch.equal(res[0][0], res[1][0]) and torch.isfinite(res[0][0]).all()
        if lay.rev_stash:
            assert torch.equal(res[0][1], res[1][1]) and torch.isfinite(res[0][1]).all()
        # the images: [rb][cb][4][64], row = 16 rb + (lane >> 4) + 4 r, col = 16 cb + (lane & 15)
        red = res[0][0].cpu().numpy()
        NB, JB = lay.NBLK, lay.JB
        lane = np.arange(64)
        rows = lambda nrb, ncb: (16 * np.arange(nrb)[:, None, None, None] + 4 * np.arange(4)[None, None, :, None]     # noqa: E731
                                 + (lane >> 4)[None, None, None, :]) + np.zeros((nrb, ncb, 4, 64), int)
        cols = lambda nrb, ncb: (16 * np.arange(ncb)[None, :, None, None] + (lane & 15)[None, None, None, :]     # noqa: E731
                                 + np.zeros((nrb, ncb, 4, 64), int))
        o = 0
        for ncb, width in ((1, Do), (1, Do)) + (() if lay.rev_stash else ((NB, M),)) + ((JB, D),):
            img = red[o:o + NB * ncb * 256].reshape(NB, ncb, 4, 64)
            outside = (rows(NB, ncb) >= M) | (cols(NB, ncb) >= width)
            assert not img[outside].any() and img[~outside].any()
            o += NB * ncb * 256
        small = red[o:]
        assert small.shape == (192,) and not small[:32].any() and not small[32 + D:96].any() and not small[98:].any()
