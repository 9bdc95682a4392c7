"""Full-covariance q(z) on the GPU: the differentiable conditional() in its three q_sqrt branches and GPModel(q_full=True),
through the C ABI and through cbfssm.hip.autograd / cbfssm.model.gp_tf, against reverse-mode autodiff on the CPU
(tests/gp_fullq_cases.py; for q_sqrt None / (M, Do) oracle/cbfssm_torch_ref.GPModel).  Rules: fmean / fvar rtol 1e-8,
atol 1e-11 (tests/test_gp_tf_surface_gpu.py); KL 1e-9 relative; every gradient tensor within 1e-6 of its largest entry
(gp_autograd_cases.within_rule, which prints the achieved ratio)."""
import ctypes as C

import numpy as np
import pytest
import torch

import gp_autograd_cases as gc
import gp_fullq_cases as fq
from gp_fullq_cases import CASES, PARAMS, within_rule

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
IDS = ['M%d-D%d-Do%d-n%d' % c for c in CASES]


def _dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64, device=DEV)


def _model(p, M, D, Do, grad=PARAMS):
    """a q_full gp_tf.GPModel carrying the case's parameters as leaves; `grad`: the names that require grad"""
    from cbfssm.model import gp_tf
    gp = gp_tf.GPModel(in_dim=D, out_dim=Do, num_points=M, gp_var=0.4, gp_len=1.0, zeta_mean=0.1, zeta_pos=1.0, zeta_var=0.01,
                       seed=0, device=DEV, q_full=True)
    gp.zeta_pos, gp.zeta_mean, gp.zeta_sqrt = _dev(p['zeta_pos']), _dev(p['zeta_mean']), _dev(p['zeta_sqrt'])
    gp.kern.variance_unc, gp.kern.lengthscales_unc = _dev(p['variance_unc']), _dev(p['lengthscales_unc'])
    leaves = dict(zip(PARAMS, gp.parameters()))
    for k in grad:
        leaves[k].requires_grad_()
    return gp, leaves


def _check_upper_zero(g, M):
    upper = np.triu(np.ones((M, M), dtype=bool), 1)
    assert np.all(g[:, upper] == 0.0), 'd/dq above the diagonal is not exactly zero'


def _abi(M, D, Do, npts, p, X, Wm, Wv, kl_weight, data=True, form='dense'):
    """the C calls in the order cbfssm.hip.autograd makes them; buffers poisoned with NaN.  form: 'dense' or 'tri', the pack's.
    returns (grads dict by PARAMS, gX, fmean, fvar, kl, everything concatenated for the bitwise comparison)"""
    from cbfssm.hip import lib as _l, ops
    from cbfssm.hip.ops import _ptr, _stream
    lib = _l.load()
    nan = float('nan')
    pack = ops.GPPack(M, D, Do, torch.device(DEV), form_mode=form)
    pt = {k: _dev(p[k]) for k in PARAMS}
    var, ls = ops.tf_forward(pt['variance_unc']), ops.tf_forward(pt['lengthscales_unc'])
    hole = torch.zeros(M * Do, dtype=torch.float64, device=DEV)
    pack.prepare(pt['zeta_pos'], ls, var, pt['zeta_mean'], hole.view(M, Do))
    lay = pack.layout
    q = pt['zeta_sqrt'].contiguous()
    pflat = torch.cat([pt['zeta_pos'].reshape(-1), pt['zeta_mean'].reshape(-1), hole, pt['variance_unc'].reshape(-1),
                       pt['lengthscales_unc'].reshape(-1)]).contiguous()
    cflat = torch.cat([pt['zeta_pos'].reshape(-1), pt['zeta_mean'].reshape(-1), hole, var.reshape(-1), ls.reshape(-1)]).contiguous()
    qpack = torch.full((lib.cbfssm_gp_fullq_pack_elems(C.byref(lay)),), nan, dtype=torch.float64, device=DEV)
    _l.check(lib.cbfssm_gp_fullq_prepare_f64(C.byref(lay), _ptr(q), _ptr(qpack), _stream()), 'prepare')
    kl = torch.full((1,), nan, dtype=torch.float64, device=DEV)
    _l.check(lib.cbfssm_gp_fullq_kl_f64(C.byref(lay), _ptr(pack.buf), _ptr(q), _ptr(qpack), _ptr(pt['zeta_mean'].contiguous()),
                                        _ptr(kl), _stream()), 'kl')
    red = image = gX = W = fmean = fvar = None
    if data:
        Xd, gm, gv = _dev(X), _dev(Wm), _dev(Wv)
        fmean = torch.full((npts, Do), nan, dtype=torch.float64, device=DEV)
        fvar = torch.full((npts, Do), nan, dtype=torch.float64, device=DEV)
        _l.check(lib.cbfssm_gp_fullq_predict_f64(C.byref(lay), _ptr(pack.buf), _ptr(qpack), _ptr(Xd), npts, _ptr(fmean),
                                                 _ptr(fvar), _stream()), 'forward')
        assert not torch.isnan(fmean).any() and not torch.isnan(fvar).any(), 'an output entry was not written'
        # the scalar-FMA forward of the evaluation-only conditional(), which reads the whole matrix: the same values
        fm0, fv0 = torch.empty_like(fmean), torch.empty_like(fvar)
        fwork = torch.empty(lib.cbfssm_gp_predict_fullq_work_elems(C.byref(lay), npts), dtype=torch.float64, device=DEV)
        _l.check(lib.cbfssm_gp_predict_fullq_f64(C.byref(lay), _ptr(pack.buf), _ptr(torch.tril(q).contiguous()), _ptr(Xd), npts,
                                                 _ptr(fm0), _ptr(fv0), _ptr(fwork), _stream()), 'old forward')
        np.testing.assert_allclose(fmean.cpu().numpy(), fm0.cpu().numpy(), rtol=1e-8, atol=1e-11)
        np.testing.assert_allclose(fvar.cpu().numpy(), fv0.cpu().numpy(), rtol=1e-8, atol=1e-11)
        nwg = lib.cbfssm_gp_fullq_bwd_workgroups(C.byref(lay), npts)
        assert 1 <= nwg <= (npts + 15) // 16
        gpart = torch.full(((nwg + 32) * lay.rev_slab,), nan, dtype=torch.float64, device=DEV)
        nwork = lib.cbfssm_gp_fullq_bwd_work_elems(C.byref(lay), npts)
        assert (nwork > 0) == bool(lay.rev_stash)
        work = torch.full((nwork,), nan, dtype=torch.float64, device=DEV) if nwork else None
        image = torch.full((lay.NBLK * lay.NBLK * 256,), nan, dtype=torch.float64, device=DEV) if lay.rev_stash else None
        a2 = torch.full((lib.cbfssm_gp_fullq_a2_elems(C.byref(lay), npts),), nan, dtype=torch.float64, device=DEV)
        gX = torch.full((npts, D), nan, dtype=torch.float64, device=DEV)
        _l.check(lib.cbfssm_gp_fullq_bwd_f64(C.byref(lay), _ptr(pack.buf), _ptr(qpack), _ptr(Xd), npts, _ptr(gm), _ptr(gv),
                                             _ptr(gX), _ptr(gpart), _ptr(a2), _ptr(work), _ptr(image), _stream()), 'bwd')
        red = torch.empty(lay.rev_slab, dtype=torch.float64, device=DEV)
        _l.check(lib.cbfssm_reduce_partials_f64(_ptr(gpart), lay.rev_slab, nwg, _ptr(red), _stream()), 'reduce')
        wwork = torch.full((lib.cbfssm_gp_fullq_wd_work_elems(C.byref(lay), npts),), nan, dtype=torch.float64, device=DEV)
        W = torch.full((Do, M, M), nan, dtype=torch.float64, device=DEV)
        _l.check(lib.cbfssm_gp_fullq_wd_f64(C.byref(lay), _ptr(a2), _ptr(gv), npts, _ptr(wwork), _ptr(W), _stream()), 'wd')
        assert torch.equal(W, W.transpose(1, 2)), 'W_d is not exactly symmetric'
    work_t = torch.empty(int(lib.cbfssm_train_tail_half_work_elems(C.byref(lay))), dtype=torch.float64, device=DEV)
    gflat = torch.full_like(pflat, nan)
    _l.check(lib.cbfssm_gp_tail_fullq_f64(C.byref(lay), _ptr(pack.buf), _ptr(qpack), _ptr(red), _ptr(image), 0, float(kl_weight),
                                          _ptr(pflat), _ptr(cflat), _ptr(work_t), _ptr(gflat), _stream()), 'tail')
    gq = torch.full((Do, M, M), nan, dtype=torch.float64, device=DEV)
    _l.check(lib.cbfssm_gp_fullq_lbar_f64(C.byref(lay), _ptr(pack.buf), _ptr(q), _ptr(W), float(kl_weight), _ptr(gq), _stream()),
             'lbar')
    o1, o2, o3 = M * D, M * D + M * Do, M * D + 2 * M * Do
    assert torch.all(gflat[o2:o3] == 0.0), 'the zeta_var entries of gflat are written as zero'
    out = {'zeta_pos': gflat[:o1].view(M, D), 'zeta_mean': gflat[o1:o2].view(M, Do), 'zeta_sqrt': gq,
           'variance_unc': gflat[o3:o3 + 1], 'lengthscales_unc': gflat[o3 + 1:]}
    out = {k: v.cpu().numpy() for k, v in out.items()}
    bits = torch.cat([gflat, gq.reshape(-1)] + ([gX.reshape(-1), fmean.reshape(-1), fvar.reshape(-1)] if data else []))
    return out, gX, fmean, fvar, kl, bits


@pytest.mark.parametrize('M,D,Do,npts', CASES, ids=IDS)
def test_c_abi_against_the_reference(M, D, Do, npts):
    ref = fq.reference(M, D, Do, npts)
    p, X, Wm, Wv = fq.make_inputs(M, D, Do, npts)
    g, gX, fmean, fvar, kl, bits = _abi(M, D, Do, npts, p, X, Wm, Wv, fq.KL_WEIGHT)
    _, _, _, _, _, bits2 = _abi(M, D, Do, npts, p, X, Wm, Wv, fq.KL_WEIGHT)
    gk, _, _, _, _, _ = _abi(M, D, Do, npts, p, X, Wm, Wv, 1.0, data=False)
    np.testing.assert_allclose(fmean.cpu().numpy(), ref['fmean'], rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(fvar.cpu().numpy(), ref['fvar'], rtol=1e-8, atol=1e-11)
    print('kl %.15g reference %.15g rel %.2e' % (float(kl), ref['kl'], abs(float(kl) - ref['kl']) / abs(ref['kl'])))
    assert float(kl) == pytest.approx(ref['kl'], rel=1e-9)
    within_rule('gX', gX.cpu().numpy(), ref['g_X'])
    for k in PARAMS:
        within_rule('loss: ' + k, g[k], ref['g_' + k].reshape(g[k].shape))
    for k in PARAMS:
        within_rule('prior_kl alone: ' + k, gk[k], ref['k_' + k].reshape(gk[k].shape))
    _check_upper_zero(g['zeta_sqrt'], M)
    _check_upper_zero(gk['zeta_sqrt'], M)
    assert torch.equal(bits, bits2), 'two calls differ'


@pytest.mark.parametrize('M,D,Do,npts', CASES, ids=IDS)
def test_autograd_against_the_reference(M, D, Do, npts):
    ref = fq.reference(M, D, Do, npts)
    p, X, Wm, Wv = fq.make_inputs(M, D, Do, npts)
    gp, leaves = _model(p, M, D, Do)
    Xd = _dev(X).requires_grad_()
    fmean, fvar = gp.predict(Xd)
    kl = gp.prior_kl()
    assert fmean.grad_fn is not None and fvar.grad_fn is not None and kl.grad_fn is not None
    np.testing.assert_allclose(fmean.detach().cpu().numpy(), ref['fmean'], rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(fvar.detach().cpu().numpy(), ref['fvar'], rtol=1e-8, atol=1e-11)
    assert float(kl.detach()) == pytest.approx(ref['kl'], rel=1e-9)
    ((_dev(Wm) * fmean).sum() + (_dev(Wv) * fvar).sum() + fq.KL_WEIGHT * kl).backward()
    within_rule('gX', Xd.grad.cpu().numpy(), ref['g_X'])
    for k in PARAMS:
        within_rule(k, leaves[k].grad.cpu().numpy().reshape(ref['g_' + k].shape), ref['g_' + k])
    _check_upper_zero(leaves['zeta_sqrt'].grad.cpu().numpy(), M)


# ---- conditional() ---------------------------------------------------------------------------------------------------

def _kern(p):
    from cbfssm.model import gp_tf
    kern = gp_tf.RBF(0.4, np.ones(len(p['lengthscales_unc'])), device=DEV)
    kern.variance_unc, kern.lengthscales_unc = _dev(p['variance_unc']), _dev(p['lengthscales_unc'])
    return kern


@pytest.mark.parametrize('M,D,Do,npts', [(12, 4, 3, 41), (100, 21, 14, 41), (113, 9, 1, 17), (200, 13, 7, 41)])
def test_conditional_full_matrix_branch_is_differentiable(M, D, Do, npts):
    from cbfssm.model import gp_tf
    ref = fq.reference(M, D, Do, npts)
    p, X, Wm, Wv = fq.make_inputs(M, D, Do, npts)
    kern = _kern(p)
    t = {'Xnew': _dev(X), 'X': _dev(p['zeta_pos']), 'f': _dev(p['zeta_mean']), 'q_sqrt': _dev(p['zeta_sqrt'])}
    for v in list(t.values()) + [kern.variance_unc, kern.lengthscales_unc]:
        v.requires_grad_()
    fmean, fvar = gp_tf.conditional(t['Xnew'], t['X'], kern, t['f'], t['q_sqrt'])
    assert fmean.grad_fn is not None and fvar.grad_fn is not None
    np.testing.assert_allclose(fmean.detach().cpu().numpy(), ref['fmean'], rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(fvar.detach().cpu().numpy(), ref['fvar'], rtol=1e-8, atol=1e-11)
    ((_dev(Wm) * fmean).sum() + (_dev(Wv) * fvar).sum()).backward()
    # the reference of the data terms alone: the loss's gradient minus 0.3 times the KL's
    want = {k: ref['g_' + k] - fq.KL_WEIGHT * ref['k_' + k] for k in PARAMS}
    within_rule('Xnew', t['Xnew'].grad.cpu().numpy(), ref['g_X'])
    within_rule('X', t['X'].grad.cpu().numpy(), want['zeta_pos'])
    within_rule('f', t['f'].grad.cpu().numpy(), want['zeta_mean'])
    within_rule('q_sqrt', t['q_sqrt'].grad.cpu().numpy(), want['zeta_sqrt'])
    within_rule('variance_unc', kern.variance_unc.grad.cpu().numpy().reshape(-1), want['variance_unc'].reshape(-1))
    within_rule('lengthscales_unc', kern.lengthscales_unc.grad.cpu().numpy(), want['lengthscales_unc'])
    _check_upper_zero(t['q_sqrt'].grad.cpu().numpy(), M)


def _diag_reference(p, X, Wm, Wv, q):
    """oracle/cbfssm_torch_ref.GPModel with zeta_var = q^2, differentiated with respect to q (q None: zeta_var = 0)"""
    from oracle import cbfssm_torch_ref as tref
    t = {k: torch.tensor(p[k], dtype=torch.float64, requires_grad=True) for k in ('zeta_pos', 'zeta_mean', 'variance_unc',
                                                                                   'lengthscales_unc')}
    qt = None if q is None else torch.tensor(q, dtype=torch.float64, requires_grad=True)
    gp = tref.GPModel(t['zeta_pos'], t['zeta_mean'], torch.zeros_like(t['zeta_mean']), t['variance_unc'], t['lengthscales_unc'])
    gp.zeta_var = torch.zeros_like(t['zeta_mean']) if q is None else qt * qt
    gp.zeta_std = torch.sqrt(gp.zeta_var) if q is None else torch.abs(qt)
    Xt = torch.tensor(X, requires_grad=True)
    fmean, fvar = gp.predict(Xt)
    ((torch.tensor(Wm) * fmean).sum() + (torch.tensor(Wv) * fvar).sum()).backward()
    out = {k: v.grad.numpy() for k, v in t.items()}
    out['Xnew'] = Xt.grad.numpy()
    out['q'] = None if q is None else qt.grad.numpy()
    return fmean.detach().numpy(), fvar.detach().numpy(), out


@pytest.mark.parametrize('branch', ['none', 'diag', 'diag_tiny_entry'])
@pytest.mark.parametrize('M,D,Do,npts', [(100, 21, 14, 41), (130, 6, 4, 41)])
def test_conditional_none_and_diagonal_branches_are_differentiable(M, D, Do, npts, branch):
    from cbfssm.model import gp_tf
    p, X, Wm, Wv = gc.make_inputs(M, D, Do, npts)
    q = None
    if branch != 'none':
        q = 0.2 * np.exp(np.random.default_rng(3).uniform(-0.5, 0.5, (M, Do)))
        q[::3] *= -1.0                                        # (only q^2 enters)
        if branch == 'diag_tiny_entry':
            q[5, 0] = 1e-6                                    # q^2 = 1e-12 < 1e-10: not a value of softplus + 1e-10
    fm_r, fv_r, want = _diag_reference(p, X, Wm, Wv, q)
    kern = _kern(p)
    t = {'Xnew': _dev(X), 'X': _dev(p['zeta_pos']), 'f': _dev(p['zeta_mean'])}
    qd = None if q is None else _dev(q)
    for v in list(t.values()) + [kern.variance_unc, kern.lengthscales_unc] + ([] if q is None else [qd]):
        v.requires_grad_()
    fmean, fvar = gp_tf.conditional(t['Xnew'], t['X'], kern, t['f'], qd)
    assert fmean.grad_fn is not None and fvar.grad_fn is not None
    np.testing.assert_allclose(fmean.detach().cpu().numpy(), fm_r, rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(fvar.detach().cpu().numpy(), fv_r, rtol=1e-8, atol=1e-11)
    ((_dev(Wm) * fmean).sum() + (_dev(Wv) * fvar).sum()).backward()
    within_rule('Xnew', t['Xnew'].grad.cpu().numpy(), want['Xnew'])
    within_rule('X', t['X'].grad.cpu().numpy(), want['zeta_pos'])
    within_rule('f', t['f'].grad.cpu().numpy(), want['zeta_mean'])
    within_rule('variance_unc', kern.variance_unc.grad.cpu().numpy().reshape(-1), want['variance_unc'].reshape(-1))
    within_rule('lengthscales_unc', kern.lengthscales_unc.grad.cpu().numpy(), want['lengthscales_unc'])
    if q is not None:
        g = qd.grad.cpu().numpy()
        within_rule('q_sqrt', g, want['q'])
        if branch == 'diag_tiny_entry':                       # the small entry's own gradient, relative to itself
            assert g[5, 0] == pytest.approx(want['q'][5, 0], rel=1e-6) and g[5, 0] != 0.0


@pytest.mark.parametrize('M,D,Do,npts', [(100, 21, 14, 41), (130, 6, 4, 41)])
def test_conditional_without_a_gradient_request_is_the_evaluation_path_bit_for_bit(M, D, Do, npts):
    from cbfssm.hip import lib as _l, ops
    from cbfssm.hip.ops import _ptr, _stream
    from cbfssm.model import gp_tf
    lib = _l.load()
    p, X, _, _ = fq.make_inputs(M, D, Do, npts)
    kern = _kern(p)
    Xd, Z, f, q3 = _dev(X), _dev(p['zeta_pos']), _dev(p['zeta_mean']), _dev(np.tril(p['zeta_sqrt']))
    q2 = _dev(0.2 * np.exp(np.random.default_rng(3).uniform(-0.5, 0.5, (M, Do))))

    def direct(zvar, q):
        pack = ops.GPPack(M, D, Do, torch.device(DEV))
        pack.prepare(Z, kern.lengthscales, kern.variance, f, zvar)
        if q is None:
            return pack.predict(Xd)
        fm, fv = torch.empty(npts, Do, dtype=torch.float64, device=DEV), torch.empty(npts, Do, dtype=torch.float64, device=DEV)
        work = torch.empty(int(lib.cbfssm_gp_predict_fullq_work_elems(C.byref(pack.layout), npts)), dtype=torch.float64, device=DEV)
        _l.check(lib.cbfssm_gp_predict_fullq_f64(C.byref(pack.layout), _ptr(pack.buf), _ptr(q), _ptr(Xd), npts, _ptr(fm), _ptr(fv),
                                                 _ptr(work), _stream()), 'fullq')
        return fm, fv

    zero = torch.zeros(M, Do, dtype=torch.float64, device=DEV)
    for q, want in ((None, direct(zero, None)), (q2, direct(q2 * q2, None)), (q3, direct(zero, q3))):
        fm, fv = gp_tf.conditional(Xd, Z, kern, f, q)
        assert fm.grad_fn is None and fv.grad_fn is None
        assert torch.equal(fm, want[0]) and torch.equal(fv, want[1])
        # arguments that require grad, under torch.no_grad(): the same path
        qg = None if q is None else q.clone().requires_grad_()
        with torch.no_grad():
            fm1, fv1 = gp_tf.conditional(Xd.clone().requires_grad_(), Z, kern, f, qg)
        assert fm1.grad_fn is None and torch.equal(fm1, want[0]) and torch.equal(fv1, want[1])
        # under grad: None / (M, Do) run the same forward kernel (the same bits), (Do, M, M) the MFMA forward (the rule)
        fm2, fv2 = gp_tf.conditional(Xd.clone().requires_grad_(), Z, kern, f, qg)
        assert fm2.grad_fn is not None
        if q is None or q.dim() == 2:
            assert torch.equal(fm2.detach(), want[0]) and torch.equal(fv2.detach(), want[1])
        else:
            np.testing.assert_allclose(fm2.detach().cpu().numpy(), want[0].cpu().numpy(), rtol=1e-8, atol=1e-11)
            np.testing.assert_allclose(fv2.detach().cpu().numpy(), want[1].cpu().numpy(), rtol=1e-8, atol=1e-11)


# ---- GPModel(q_full=True) --------------------------------------------------------------------------------------------

@pytest.mark.parametrize('M,D,Do,npts', [(12, 4, 3, 41), (100, 21, 14, 41), (113, 9, 1, 17)])
def test_full_form_with_diagonal_factors_equals_the_diagonal_model(M, D, Do, npts):
    from cbfssm.model import gp_tf
    p, X, Wm, Wv = gc.make_inputs(M, D, Do, npts)
    shared = ('zeta_pos', 'zeta_mean', 'variance_unc', 'lengthscales_unc')

    def build(q_full):
        gp = gp_tf.GPModel(in_dim=D, out_dim=Do, num_points=M, gp_var=0.4, gp_len=1.0, zeta_mean=0.1, zeta_pos=1.0, zeta_var=0.01,
                           seed=0, device=DEV, q_full=q_full)
        gp.zeta_pos, gp.zeta_mean = _dev(p['zeta_pos']), _dev(p['zeta_mean'])
        gp.kern.variance_unc, gp.kern.lengthscales_unc = _dev(p['variance_unc']), _dev(p['lengthscales_unc'])
        return gp
    gd = build(False)
    gd.zeta_var_unc = _dev(p['zeta_var_unc'])
    gf = build(True)
    std = torch.sqrt(gd.zeta_var)                              # (M, Do)
    gf.zeta_sqrt = torch.diag_embed(std.t()).contiguous()
    assert torch.allclose(gf.zeta_var, gd.zeta_var, rtol=1e-14, atol=0) and gf.zeta_std.shape == (Do, M, M)
    out = []
    for gp in (gd, gf):
        for t in gp.parameters():
            t.requires_grad_()
        Xd = _dev(X).requires_grad_()
        fmean, fvar = gp.predict(Xd)
        kl = gp.prior_kl()
        ((_dev(Wm) * fmean).sum() + (_dev(Wv) * fvar).sum() + gc.KL_WEIGHT * kl).backward()
        out.append((fmean.detach(), fvar.detach(), kl.detach(), Xd.grad))
    (fm0, fv0, kl0, gx0), (fm1, fv1, kl1, gx1) = out
    for a, b, name in ((fm1, fm0, 'fmean'), (fv1, fv0, 'fvar')):
        err = float((a - b).abs().max() / b.abs().max())
        print('%s: full vs diagonal %.2e of the largest entry' % (name, err))
        assert err < 1e-12
    assert float(kl1) == pytest.approx(float(kl0), rel=1e-12)
    within_rule('gX', gx1.cpu().numpy(), gx0.cpu().numpy())
    pd, pf = dict(zip(gc.PARAMS, gd.parameters())), dict(zip(PARAMS, gf.parameters()))
    for k in shared:
        within_rule(k, pf[k].grad.cpu().numpy(), pd[k].grad.cpu().numpy())
    # diag(Lbar_d) chains to the diagonal model's zeta_var_unc: d std / d unc = sigmoid(unc) / (2 std)
    gdiag = torch.diagonal(pf['zeta_sqrt'].grad, dim1=1, dim2=2).t()
    chain = gdiag * torch.sigmoid(pd['zeta_var_unc'].detach()) / (2.0 * std)
    within_rule('zeta_var_unc', chain.cpu().numpy(), pd['zeta_var_unc'].grad.cpu().numpy())


def test_two_backward_calls_are_bitwise_identical():
    M, D, Do, npts = 200, 13, 7, 41
    p, X, Wm, Wv = fq.make_inputs(M, D, Do, npts)
    runs = []
    for _ in range(2):
        gp, leaves = _model(p, M, D, Do)
        Xd = _dev(X).requires_grad_()
        fmean, fvar = gp.predict(Xd)
        ((_dev(Wm) * fmean).sum() + (_dev(Wv) * fvar).sum() + fq.KL_WEIGHT * gp.prior_kl()).backward()
        runs.append([Xd.grad] + [leaves[k].grad for k in PARAMS])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_only_the_requested_gradients_come_back():
    M, D, Do, npts = 100, 21, 14, 41
    ref = fq.reference(M, D, Do, npts)
    p, X, Wm, Wv = fq.make_inputs(M, D, Do, npts)
    gp, leaves = _model(p, M, D, Do, grad=())
    Xd = _dev(X).requires_grad_()
    fmean, fvar = gp.predict(Xd)
    assert gp.prior_kl().grad_fn is None
    ((_dev(Wm) * fmean).sum() + (_dev(Wv) * fvar).sum()).backward()
    within_rule('gX', Xd.grad.cpu().numpy(), ref['g_X'])
    assert all(leaves[k].grad is None for k in PARAMS)
    for only in ('zeta_sqrt', 'zeta_mean'):
        gp, leaves = _model(p, M, D, Do, grad=(only,))
        Xd = _dev(X)
        fmean, fvar = gp.predict(Xd)
        ((_dev(Wm) * fmean).sum() + (_dev(Wv) * fvar).sum() + fq.KL_WEIGHT * gp.prior_kl()).backward()
        within_rule(only, leaves[only].grad.cpu().numpy(), ref['g_' + only])
        assert Xd.grad is None and all(leaves[k].grad is None for k in PARAMS if k != only)


def test_backward_does_not_read_the_shared_pack():
    """the pack is re-prepared with OTHER parameters between forward and backward: the gradients are those of the forward's"""
    M, D, Do, npts = 12, 4, 3, 41
    ref = fq.reference(M, D, Do, npts)
    p, X, Wm, Wv = fq.make_inputs(M, D, Do, npts)
    gp, leaves = _model(p, M, D, Do)
    Xd = _dev(X).requires_grad_()
    fmean, fvar = gp.predict(Xd)
    kl = gp.prior_kl()
    other, _, _, _ = gc.make_inputs(M, D, Do, npts, seed=99)
    gp._pack.prepare(_dev(other['zeta_pos']), torch.full((D,), 3.0, dtype=torch.float64, device=DEV),
                     torch.tensor([2.0], dtype=torch.float64, device=DEV), _dev(other['zeta_mean']),
                     torch.full((M, Do), 0.5, dtype=torch.float64, device=DEV))
    ((_dev(Wm) * fmean).sum() + (_dev(Wv) * fvar).sum() + fq.KL_WEIGHT * kl).backward()
    within_rule('gX', Xd.grad.cpu().numpy(), ref['g_X'])
    for k in PARAMS:
        within_rule(k, leaves[k].grad.cpu().numpy().reshape(ref['g_' + k].shape), ref['g_' + k])


@pytest.mark.parametrize('M,D,Do,npts', CASES[:-1], ids=IDS[:-1])
def test_evaluation_of_a_full_q_model(M, D, Do, npts):
    """without a gradient request: the MFMA forward and the KL alone, the bits of the values under grad, no grad_fn"""
    ref = fq.reference(M, D, Do, npts)
    p, X, _, _ = fq.make_inputs(M, D, Do, npts)
    gp, _ = _model(p, M, D, Do, grad=())
    fmean, fvar = gp.predict(_dev(X))
    kl = gp.prior_kl()
    assert fmean.grad_fn is None and fvar.grad_fn is None and kl.grad_fn is None
    np.testing.assert_allclose(fmean.cpu().numpy(), ref['fmean'], rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(fvar.cpu().numpy(), ref['fvar'], rtol=1e-8, atol=1e-11)
    assert float(kl) == pytest.approx(ref['kl'], rel=1e-9)
    gp2, _ = _model(p, M, D, Do)
    fm2, fv2 = gp2.predict(_dev(X))
    assert fm2.grad_fn is not None and torch.equal(fm2.detach(), fmean) and torch.equal(fv2.detach(), fvar)
    assert torch.equal(gp2.prior_kl().detach(), kl)
    with torch.no_grad():
        fm3, fv3 = gp2.predict(_dev(X))
    assert fm3.grad_fn is None and torch.equal(fm3, fmean) and torch.equal(fv3, fvar)
    empty = gp.predict(torch.zeros(0, D, dtype=torch.float64, device=DEV))
    assert empty[0].shape == (0, Do) and empty[1].shape == (0, Do)


@pytest.mark.parametrize('M,D,Do,npts', [(113, 9, 1, 17), (100, 21, 14, 41), (300, 6, 4, 41)])
def test_two_triangular_form(monkeypatch, M, D, Do, npts):
    monkeypatch.setenv('CBFSSM_GP_FORM', 'tri')
    ref = fq.reference(M, D, Do, npts)
    p, X, Wm, Wv = fq.make_inputs(M, D, Do, npts)
    gp, leaves = _model(p, M, D, Do)
    assert gp._pack.gp_form() == 'tri'
    Xd = _dev(X).requires_grad_()
    fmean, fvar = gp.predict(Xd)
    np.testing.assert_allclose(fmean.detach().cpu().numpy(), ref['fmean'], rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(fvar.detach().cpu().numpy(), ref['fvar'], rtol=1e-8, atol=1e-11)
    ((_dev(Wm) * fmean).sum() + (_dev(Wv) * fvar).sum() + fq.KL_WEIGHT * gp.prior_kl()).backward()
    within_rule('gX', Xd.grad.cpu().numpy(), ref['g_X'])
    for k in PARAMS:
        within_rule(k, leaves[k].grad.cpu().numpy().reshape(ref['g_' + k].shape), ref['g_' + k])


def test_no_points_launch_nothing_and_give_zero_gradients():
    M, D, Do = 100, 21, 14
    p, _, _, _ = fq.make_inputs(M, D, Do, 41)
    gp, leaves = _model(p, M, D, Do)
    Xd = torch.zeros(0, D, dtype=torch.float64, device=DEV).requires_grad_()
    fmean, fvar = gp.predict(Xd)
    assert fmean.shape == (0, Do) and fvar.shape == (0, Do) and fmean.grad_fn is not None
    (fmean.sum() + fvar.sum()).backward()
    assert Xd.grad.shape == (0, D)
    for k in PARAMS:
        assert leaves[k].grad.shape == leaves[k].shape and torch.all(leaves[k].grad == 0.0), k


def test_rollout_and_filter_refuse_a_full_q_model():
    M, D, Do = 12, 4, 3
    p, _, _, _ = fq.make_inputs(M, D, Do, 41)
    gp, _ = _model(p, M, D, Do, grad=())
    h0 = torch.zeros(16, Do, dtype=torch.float64, device=DEV)
    a = torch.zeros(2, 16, D - Do, dtype=torch.float64, device=DEV)
    eps = torch.zeros(2, 16, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match='q_full'):
        gp.rollout(h0, a, eps)
    with pytest.raises(ValueError, match='q_full'):
        gp.filter(h0, a, torch.zeros(2, 16, Do, dtype=torch.float64, device=DEV), eps, None,
                  torch.ones(Do, dtype=torch.float64, device=DEV))


def test_adam_lowers_the_negative_elbo_of_a_noisy_sine_regression():
    from cbfssm.model import gp_tf
    rng = np.random.default_rng(2)
    x = rng.uniform(-3, 3, (200, 1))
    y = _dev(np.sin(x) + 0.1 * rng.standard_normal(x.shape))
    xd = _dev(x)
    gp = gp_tf.GPModel(in_dim=1, out_dim=1, num_points=20, gp_var=0.5, gp_len=1.0, zeta_mean=0.05, zeta_pos=3.0, zeta_var=0.01,
                       seed=4, device=DEV, q_full=True)
    params = gp.parameters()
    assert params[2].shape == (1, 20, 20) and torch.equal(params[2][0], float(np.sqrt(0.01)) * torch.eye(20, dtype=torch.float64, device=DEV))
    for q in params:
        q.requires_grad_()
    opt = torch.optim.Adam(params, lr=0.02)

    def loss_fn():
        fmean, fvar = gp.predict(xd)
        # Gaussian negative expected log-likelihood with noise variance 0.01, plus the prior KL
        return (0.5 * ((y - fmean) ** 2 + fvar) / 0.01).sum() + gp.prior_kl()
    initial = None
    for _ in range(50):
        opt.zero_grad()
        loss = loss_fn()
        loss.backward()
        opt.step()
        initial = float(loss.detach()) if initial is None else initial
    final = float(loss_fn().detach())
    print('initial %.6g final %.6g' % (initial, final))
    assert np.isfinite(final) and final < initial
    strict = torch.tril(gp.zeta_sqrt.detach(), -1)
    assert float(strict.abs().max()) > 0.0, 'zeta_sqrt has not left the diagonal'
    assert torch.all(torch.triu(gp.zeta_sqrt.detach(), 1) == 0.0)
