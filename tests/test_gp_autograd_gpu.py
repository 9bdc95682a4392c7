"""Differentiable GPModel on the GPU: cbfssm_gp_predict_bwd_f64 -> cbfssm_reduce_partials_f64 -> cbfssm_gp_tail_f64 through
the C ABI and through cbfssm.hip.autograd / cbfssm.model.gp_tf.GPModel, against reverse-mode autodiff of the CPU oracle
(tests/gp_autograd_cases.py).  Rule for gradients: every entry within 1e-6 of the largest entry of its tensor
(tests/test_hip_grad.py); fmean / fvar under grad: rtol 1e-8, atol 1e-12."""
import ctypes as C

import numpy as np
import pytest
import torch

import gp_autograd_cases as gc
from gp_autograd_cases import CASES, PARAMS, within_rule

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64, device=DEV)


def _model(p, M, D, Do, grad=PARAMS):
    """a gp_tf.GPModel carrying the case's parameters as leaves; `grad`: the names that require grad"""
    from cbfssm.model import gp_tf
    gp = gp_tf.GPModel(in_dim=D, out_dim=Do, num_points=M, gp_var=0.4, gp_len=1.0, zeta_mean=0.1, zeta_pos=1.0, zeta_var=0.01,
                       seed=0, device=DEV)
    gp.zeta_pos, gp.zeta_mean, gp.zeta_var_unc = _dev(p['zeta_pos']), _dev(p['zeta_mean']), _dev(p['zeta_var_unc'])
    gp.kern.variance_unc, gp.kern.lengthscales_unc = _dev(p['variance_unc']), _dev(p['lengthscales_unc'])
    leaves = dict(zip(PARAMS, gp.parameters()))
    for k in grad:
        leaves[k].requires_grad_()
    return gp, leaves


def _abi_grads(M, D, Do, npts, p, X, Wm, Wv, kl_weight, data=True):
    """the three C calls; returns (gflat parts dict, gX or None)"""
    from cbfssm.hip import lib as _l, ops
    from cbfssm.hip.ops import _ptr, _stream
    lib = _l.load()
    pack = ops.GPPack(M, D, Do, torch.device(DEV), form_mode='dense')
    pt = {k: _dev(p[k]) for k in PARAMS}
    con = {k: (ops.tf_forward(pt[k]) if k.endswith('_unc') else pt[k]) for k in PARAMS}
    pack.prepare(con['zeta_pos'], con['lengthscales_unc'], con['variance_unc'], con['zeta_mean'], con['zeta_var_unc'])
    lay = pack.layout
    pflat = torch.cat([pt[k].reshape(-1) for k in PARAMS]).contiguous()
    cflat = torch.cat([con[k].reshape(-1) for k in PARAMS]).contiguous()
    red = image = gX = None
    if data:
        Xd, gm, gv = _dev(X), _dev(Wm), _dev(Wv)
        nwg = lib.cbfssm_gp_predict_bwd_workgroups(C.byref(lay), npts)
        assert nwg == min((npts + 15) // 16, nwg) and nwg >= 1
        gpart = torch.full(((nwg + 32) * lay.rev_slab,), float('nan'), dtype=torch.float64, device=DEV)
        nwork = lib.cbfssm_gp_predict_bwd_work_elems(C.byref(lay), npts)
        assert (nwork > 0) == bool(lay.rev_stash)
        work = torch.full((nwork,), float('nan'), dtype=torch.float64, device=DEV) if nwork else None
        image = torch.full((lay.NBLK * lay.NBLK * 256,), float('nan'), dtype=torch.float64, device=DEV) if lay.rev_stash else None
        gX = torch.full((npts, D), float('nan'), dtype=torch.float64, device=DEV)
        _l.check(lib.cbfssm_gp_predict_bwd_f64(C.byref(lay), _ptr(pack.buf), _ptr(Xd), npts, _ptr(gm), _ptr(gv), _ptr(gX),
                                               _ptr(gpart), _ptr(work), _ptr(image), _stream()), 'cbfssm_gp_predict_bwd_f64')
        red = torch.empty(lay.rev_slab, dtype=torch.float64, device=DEV)
        _l.check(lib.cbfssm_reduce_partials_f64(_ptr(gpart), lay.rev_slab, nwg, _ptr(red), _stream()), 'reduce')
    work_t = torch.empty(int(lib.cbfssm_train_tail_half_work_elems(C.byref(lay))), dtype=torch.float64, device=DEV)
    gflat = torch.full_like(pflat, float('nan'))
    _l.check(lib.cbfssm_gp_tail_f64(C.byref(lay), _ptr(pack.buf), _ptr(red), _ptr(image), 0, float(kl_weight), _ptr(pflat),
                                    _ptr(cflat), _ptr(work_t), _ptr(gflat), _stream()), 'cbfssm_gp_tail_f64')
    out, o = {}, 0
    for k in PARAMS:
        n = pt[k].numel()
        out[k] = gflat[o:o + n].reshape(pt[k].shape).cpu().numpy()
        o += n
    return out, (gX.cpu().numpy() if gX is not None else None), gflat


@pytest.mark.parametrize('M,D,Do,npts', CASES)
def test_c_abi_against_the_oracle(M, D, Do, npts):
    ref = gc.reference(M, D, Do, npts)
    p, X, Wm, Wv = gc.make_inputs(M, D, Do, npts)
    g, gX, gflat = _abi_grads(M, D, Do, npts, p, X, Wm, Wv, gc.KL_WEIGHT)
    g2, gX2, gflat2 = _abi_grads(M, D, Do, npts, p, X, Wm, Wv, gc.KL_WEIGHT)
    gk, _, _ = _abi_grads(M, D, Do, npts, p, X, Wm, Wv, 1.0, data=False)
    errs = [within_rule('gX', gX, ref['g_X'])]
    for k in PARAMS:
        errs.append(within_rule('loss: ' + k, g[k], ref['g_' + k].reshape(g[k].shape)))
    for k in PARAMS:
        errs.append(within_rule('prior_kl alone: ' + k, gk[k], ref['k_' + k].reshape(gk[k].shape)))
    assert np.array_equal(gX, gX2) and torch.equal(gflat, gflat2), 'two calls differ'


@pytest.mark.parametrize('M,D,Do,npts', CASES)
def test_autograd_against_the_oracle(M, D, Do, npts):
    ref = gc.reference(M, D, Do, npts)
    p, X, Wm, Wv = gc.make_inputs(M, D, Do, npts)
    gp, leaves = _model(p, M, D, Do)
    Xd = _dev(X).requires_grad_()
    fmean, fvar = gp.predict(Xd)
    kl = gp.prior_kl()
    assert fmean.grad_fn is not None and fvar.grad_fn is not None and kl.grad_fn is not None
    np.testing.assert_allclose(fmean.detach().cpu().numpy(), ref['fmean'], rtol=1e-8, atol=1e-12)
    np.testing.assert_allclose(fvar.detach().cpu().numpy(), ref['fvar'], rtol=1e-8, atol=1e-12)
    assert float(kl.detach()) == pytest.approx(ref['kl'], rel=1e-9)
    loss = (_dev(Wm) * fmean).sum() + (_dev(Wv) * fvar).sum() + gc.KL_WEIGHT * kl
    loss.backward()
    within_rule('gX', Xd.grad.cpu().numpy(), ref['g_X'])
    for k in PARAMS:
        within_rule(k, leaves[k].grad.cpu().numpy().reshape(ref['g_' + k].shape), ref['g_' + k])


def test_two_predicts_and_prior_kl_accumulate_into_the_same_leaves():
    M, D, Do, npts = 100, 21, 14, 41
    p, X, Wm, Wv = gc.make_inputs(M, D, Do, npts)
    rng = np.random.default_rng(5)
    X2, Wm2, Wv2 = 1.4 * rng.standard_normal((23, D)), rng.standard_normal((23, Do)), rng.standard_normal((23, Do))
    t, ogp = gc.oracle_model(p)
    fm1, fv1 = ogp.predict(torch.tensor(X))
    fm2, fv2 = ogp.predict(torch.tensor(X2))
    ((torch.tensor(Wm) * fm1).sum() + (torch.tensor(Wv) * fv1).sum() + (torch.tensor(Wm2) * fm2).sum()
     + (torch.tensor(Wv2) * fv2).sum() + gc.KL_WEIGHT * ogp.prior_kl()).backward()
    gp, leaves = _model(p, M, D, Do)
    a1, b1 = gp.predict(_dev(X))
    a2, b2 = gp.predict(_dev(X2))        # (re-prepares the shared pack between the first forward and its backward)
    loss = (_dev(Wm) * a1).sum() + (_dev(Wv) * b1).sum() + (_dev(Wm2) * a2).sum() + (_dev(Wv2) * b2).sum() \
        + gc.KL_WEIGHT * gp.prior_kl()
    loss.backward()
    for k in PARAMS:
        within_rule(k, leaves[k].grad.cpu().numpy(), t[k].grad.numpy())


def test_backward_does_not_read_the_shared_pack():
    """the pack is re-prepared with OTHER parameters between forward and backward: the gradients are those of the forward's"""
    M, D, Do, npts = 30, 7, 5, 16
    ref = gc.reference(M, D, Do, npts)
    p, X, Wm, Wv = gc.make_inputs(M, D, Do, npts)
    gp, leaves = _model(p, M, D, Do)
    Xd = _dev(X).requires_grad_()
    fmean, fvar = gp.predict(Xd)
    kl = gp.prior_kl()
    other, _, _, _ = gc.make_inputs(M, D, Do, npts, seed=99)
    gp._pack.prepare(_dev(other['zeta_pos']), torch.full((D,), 3.0, dtype=torch.float64, device=DEV),
                     torch.tensor([2.0], dtype=torch.float64, device=DEV), _dev(other['zeta_mean']),
                     torch.full((M, Do), 0.5, dtype=torch.float64, device=DEV))
    ((_dev(Wm) * fmean).sum() + (_dev(Wv) * fvar).sum() + gc.KL_WEIGHT * kl).backward()
    within_rule('gX', Xd.grad.cpu().numpy(), ref['g_X'])
    for k in PARAMS:
        within_rule(k, leaves[k].grad.cpu().numpy().reshape(ref['g_' + k].shape), ref['g_' + k])


def test_two_triangular_form(monkeypatch):
    """CBFSSM_GP_FORM=tri: the forward runs the reference's two triangular products, the adjoint is the same function's"""
    monkeypatch.setenv('CBFSSM_GP_FORM', 'tri')
    M, D, Do, npts = 130, 6, 4, 41
    ref = gc.reference(M, D, Do, npts)
    p, X, Wm, Wv = gc.make_inputs(M, D, Do, npts)
    gp, leaves = _model(p, M, D, Do)
    assert gp._pack.gp_form() == 'tri'
    Xd = _dev(X).requires_grad_()
    fmean, fvar = gp.predict(Xd)
    np.testing.assert_allclose(fmean.detach().cpu().numpy(), ref['fmean'], rtol=1e-8, atol=1e-12)
    np.testing.assert_allclose(fvar.detach().cpu().numpy(), ref['fvar'], rtol=1e-8, atol=1e-12)
    ((_dev(Wm) * fmean).sum() + (_dev(Wv) * fvar).sum() + gc.KL_WEIGHT * gp.prior_kl()).backward()
    within_rule('gX', Xd.grad.cpu().numpy(), ref['g_X'])
    for k in PARAMS:
        within_rule(k, leaves[k].grad.cpu().numpy().reshape(ref['g_' + k].shape), ref['g_' + k])


def test_only_the_requested_gradients_come_back():
    M, D, Do, npts = 100, 21, 14, 41
    ref = gc.reference(M, D, Do, npts)
    p, X, Wm, Wv = gc.make_inputs(M, D, Do, npts)
    # only X
    gp, leaves = _model(p, M, D, Do, grad=())
    Xd = _dev(X).requires_grad_()
    fmean, fvar = gp.predict(Xd)
    assert gp.prior_kl().grad_fn is None
    ((_dev(Wm) * fmean).sum() + (_dev(Wv) * fvar).sum()).backward()
    within_rule('gX', Xd.grad.cpu().numpy(), ref['g_X'])
    assert all(leaves[k].grad is None for k in PARAMS)
    # only zeta_mean
    gp, leaves = _model(p, M, D, Do, grad=('zeta_mean',))
    Xd = _dev(X)
    fmean, fvar = gp.predict(Xd)
    ((_dev(Wm) * fmean).sum() + (_dev(Wv) * fvar).sum() + gc.KL_WEIGHT * gp.prior_kl()).backward()
    within_rule('zeta_mean', leaves['zeta_mean'].grad.cpu().numpy(), ref['g_zeta_mean'])
    assert Xd.grad is None and all(leaves[k].grad is None for k in PARAMS if k != 'zeta_mean')


@pytest.mark.parametrize('M,D,Do,npts', [(100, 21, 14, 41), (130, 6, 4, 41)])
def test_no_grad_path_is_unchanged(M, D, Do, npts):
    from cbfssm.hip import lib as _l, ops
    p, X, _, _ = gc.make_inputs(M, D, Do, npts)
    gp, leaves = _model(p, M, D, Do, grad=())
    Xd = _dev(X)
    fmean, fvar = gp.predict(Xd)
    kl = gp.prior_kl()
    assert fmean.grad_fn is None and fvar.grad_fn is None and kl.grad_fn is None
    pack = ops.GPPack(M, D, Do, torch.device(DEV))
    pack.prepare(leaves['zeta_pos'], ops.tf_forward(leaves['lengthscales_unc']), ops.tf_forward(leaves['variance_unc']),
                 leaves['zeta_mean'], ops.tf_forward(leaves['zeta_var_unc']))
    fm0, fv0 = pack.predict(Xd)
    assert torch.equal(fmean, fm0) and torch.equal(fvar, fv0) and torch.equal(kl, pack.scal[_l.SCAL_KLZ])
    # the same with leaves that require grad, under torch.no_grad()
    gp2, _ = _model(p, M, D, Do)
    with torch.no_grad():
        fm1, fv1 = gp2.predict(Xd)
        kl1 = gp2.prior_kl()
    assert fm1.grad_fn is None and torch.equal(fm1, fm0) and torch.equal(fv1, fv0) and torch.equal(kl1, kl)
    # and the values under grad are the same bits
    fm2, fv2 = gp2.predict(Xd)
    assert fm2.grad_fn is not None and torch.equal(fm2.detach(), fm0) and torch.equal(fv2.detach(), fv0)
    assert torch.equal(gp2.prior_kl().detach(), kl)


def test_composition_with_a_physics_term_and_an_input_gain():
    """Voliro's pattern (cbfssm/model/voliro.py:106-123): fmean + X A with a learnable A, and a learnable gain in front of X"""
    M, D, Do, npts = 100, 21, 14, 41
    p, X, Wm, Wv = gc.make_inputs(M, D, Do, npts)
    rng = np.random.default_rng(11)
    A0, gain0 = 0.3 * rng.standard_normal((D, Do)), rng.uniform(0.7, 1.3, D)

    def loss_of(predict, kl, Xt, A, gain, Wm_, Wv_):
        Xg = Xt * gain
        fmean, fvar = predict(Xg)
        return (Wm_ * (fmean + Xg @ A)).sum() + (Wv_ * fvar).sum() + gc.KL_WEIGHT * kl()

    t, ogp = gc.oracle_model(p)
    Ar, gr = torch.tensor(A0, requires_grad=True), torch.tensor(gain0, requires_grad=True)
    loss_of(ogp.predict, ogp.prior_kl, torch.tensor(X), Ar, gr, torch.tensor(Wm), torch.tensor(Wv)).backward()
    gp, leaves = _model(p, M, D, Do)
    Ad, gd = _dev(A0).requires_grad_(), _dev(gain0).requires_grad_()
    loss_of(gp.predict, gp.prior_kl, _dev(X), Ad, gd, _dev(Wm), _dev(Wv)).backward()
    within_rule('A', Ad.grad.cpu().numpy(), Ar.grad.numpy())
    within_rule('gain', gd.grad.cpu().numpy(), gr.grad.numpy())
    for k in PARAMS:
        within_rule(k, leaves[k].grad.cpu().numpy(), t[k].grad.numpy())


def test_adam_lowers_the_loss_of_a_noisy_sine_regression():
    from cbfssm.model import gp_tf
    rng = np.random.default_rng(2)
    x = rng.uniform(-3, 3, (64, 1))
    y = _dev(np.sin(x) + 0.1 * rng.standard_normal(x.shape))
    xd = _dev(x)
    gp = gp_tf.GPModel(in_dim=1, out_dim=1, num_points=20, gp_var=0.5, gp_len=1.0, zeta_mean=0.05, zeta_pos=3.0, zeta_var=0.01,
                       seed=4, device=DEV)
    params = gp.parameters()
    for q in params:
        q.requires_grad_()
    opt = torch.optim.Adam(params, lr=0.05)

    def loss_fn():
        fmean, fvar = gp.predict(xd)
        # Gaussian negative log-likelihood with noise variance 0.01, plus the prior KL
        return (0.5 * ((y - fmean) ** 2 + fvar) / 0.01).sum() + gp.prior_kl()
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = loss_fn()
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    final = float(loss_fn().detach())
    initial = float(losses[0])
    print('initial %.6g final %.6g' % (initial, final))
    assert np.isfinite(final) and final < initial
