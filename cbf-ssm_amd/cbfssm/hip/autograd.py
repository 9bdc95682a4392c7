"""Differentiable torch functions over the HIP library: the CBF-SSM loss of a whole engine (`elbo_loss`), the two
functions of one sparse GP (`gp_predict`, `gp_prior_kl`, further down; `gp_predict_fullq`, `gp_prior_kl_fullq` with a
full-covariance q(z), `gp_conditional_diag` behind `gp_tf.conditional`), its recurrence over time (`gp_rollout`), the same
recurrence with a masked Gaussian filter update per step (`gp_filter`) and the rigid-body filter loop of the Voliro model
(`rigid_filter`, at the end).  `gp_linearize_eval` is evaluation only: the Jacobians of the GP mean and variance with respect
to the inputs, all output dimensions in one launch; `gp_ekf_eval`, evaluation only as well, runs the extended Kalman filter
those Jacobians are for -- a mean and a full state covariance per chain through time, conditioned where there are
observations -- as one launch; `gp_eks_eval` adds the Rauch-Tung-Striebel sweep behind it: smoothed and one-step predictive
moments, the smoothed initial belief and the lag-one cross-covariances.  `gp_moment_match_eval`, evaluation only, gives the
exact moments of the GP output under a Gaussian input -- mean, full output covariance, covariance with the input -- in one
launch, and `gp_moment_match` the same results with a grad_fn into the belief (mean, cov; the model is a constant of the
call): one fused adjoint launch; `gp_adf_eval` runs the assumed-density filter over them -- `gp_ekf_eval`'s recursion with
the exact moments in place of the linearisation -- as one launch for all steps, and `gp_ads_eval` the smoother behind it.

The CBF-SSM loss:

    loss = elbo_loss(engine, params, u, y, noise, condition=True)

`engine` is a cbfssm.hip.train.HipElboGrad, `params` the dict of its twelve unconstrained tensors (train.PARAM_NAMES) -- or a
cbfssm.hip.train_half.HipHalfGrad (CBFSSMHALF, PR-SSM) with the tensors it names (`engine.names`) --
`u` (B,T,dim_u) and `y` (B,T,dim_y) float64 device tensors, `noise` the dict of standard-normal draws the engine takes.
loss.backward() then fills .grad of every parameter tensor that requires it AND of whatever produced u and y: a learnable
input gain or bias, a sensor calibration, a feature map or an encoder in front of the model trains through the
hand-written time loops.  This is what tf.gradients(model.loss, model.sample_in) / (model.loss, model.sample_out) give
in the reference's graph (base_model.py:22-27; cbfssm/model/voliro.py:106-137 trains a GP through it).

The forward call runs the engine's loss_and_grads once -- forward evaluation and adjoint time loops -- and keeps copies
of the gradients; backward only scales them.  The input gradients (the engine's input_grads=True path: float64, no
process group) are computed only when u or y requires grad, or when `input_grads=True` asks for them; with
`input_grads=False` the call is the engine's default adjoint and u, y receive no gradient.  Nothing here computes on
the host or in the tensor library: a missing kernel is the engine's error.
"""
import collections
import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import lib as _l
from .ops import _ptr, _stream, tf_forward
from .train import PARAM_NAMES


class _ElboLoss(torch.autograd.Function):

    @staticmethod
    def forward(ctx, engine, condition, noise, input_grads, u, y, *params):
        names = _names(engine)
        pd = {k: p.detach() for k, p in zip(names, params)}
        want_in = bool(ctx.needs_input_grad[4] or ctx.needs_input_grad[5]) if input_grads is None else bool(input_grads)
        loss, grads, terms = engine.loss_and_grads(pd, u.detach(), y.detach(), noise, condition, input_grads=want_in)
        # (the engine's gradient tensors are views of buffers the next evaluation overwrites)
        ctx.grads = tuple(grads[k].clone() for k in names)
        ctx.gu = grads['u'].clone() if want_in else None
        ctx.gy = grads['y'].clone() if want_in else None
        ctx.shapes = tuple(p.shape for p in params)
        return loss.detach().clone()

    @staticmethod
    def backward(ctx, gout):
        need = ctx.needs_input_grad
        gu = ctx.gu * gout if (need[4] and ctx.gu is not None) else None
        gy = ctx.gy * gout if (need[5] and ctx.gy is not None) else None
        gp = tuple((g * gout).reshape(s) if need[6 + i] else None for i, (g, s) in enumerate(zip(ctx.grads, ctx.shapes)))
        return (None, None, None, None, gu, gy) + gp


def _names(engine):
    """the engine's parameter names: a forward-only engine lists its own, HipElboGrad has the twelve of CBFSSM"""
    return getattr(engine, 'names', None) or PARAM_NAMES


def elbo_loss(engine, params, u, y, noise, condition=True, input_grads=None):
    """The loss of one mini-batch as a 0-d tensor with a grad_fn (see the module docstring).

    input_grads: None -- d loss / d u and d loss / d y are computed when u or y requires grad; True -- always; False --
    never (u and y get no gradient; loss and parameter gradients are those of engine.loss_and_grads as it always was)."""
    names = _names(engine)
    missing = [k for k in names if k not in params]
    if missing:
        raise KeyError('elbo_loss: params lacks %s' % ', '.join(missing))
    if input_grads is False and (getattr(u, 'requires_grad', False) or getattr(y, 'requires_grad', False)):
        u, y = u.detach(), y.detach()
    return _ElboLoss.apply(engine, bool(condition), noise, input_grads, u, y, *[params[k] for k in names])


# ---- one sparse GP: GPModel.predict and GPModel.prior_kl (gp_tf.py:132-172) as torch functions -------------------------
#
#     fmean, fvar = gp_predict(pack, X, zeta_pos, zeta_mean, zeta_var_unc, variance_unc, lengthscales_unc)
#     kl = gp_prior_kl(pack, zeta_pos, zeta_mean, zeta_var_unc, variance_unc, lengthscales_unc)
#
# `pack` is an ops.GPPack of the right (M, D, Do); the five parameter tensors are the UNCONSTRAINED leaves (GPModel.parameters()),
# X is (npts, D); everything float64 on the pack's device.  The forward calls prepare the pack and evaluate as the
# evaluation-only path does; backward of gp_predict is cbfssm_gp_predict_bwd_f64 -> cbfssm_reduce_partials_f64 ->
# cbfssm_gp_tail_f64 with kl_weight 0, backward of gp_prior_kl is cbfssm_gp_tail_f64 without a slab and kl_weight 1, scaled by
# the incoming scalar on the device.  Nothing synchronises with the host.  The pack is shared and mutable (the next
# prepare overwrites it), so each call keeps a copy of the prepared buffer for its backward (0.3 MB at M = 100).  Once
# differentiable: the backward kernels are not themselves differentiated.

GP_PARAM_NAMES = ('zeta_pos', 'zeta_mean', 'zeta_var_unc', 'variance_unc', 'lengthscales_unc')


def _gp_flat(params):
    """(pflat, cflat): the five tensors behind each other, unconstrained and constrained (cbfssm_gp_tail_f64's order)."""
    zp, zm, zv, var, ls = [p.detach().reshape(-1) for p in params]
    pflat = torch.cat([zp, zm, zv, var, ls]).contiguous()
    cflat = torch.cat([zp, zm, tf_forward(zv), tf_forward(var), tf_forward(ls)]).contiguous()
    return pflat, cflat


def _gp_prepare(pack, params, cflat):
    M, D, Do = pack.M, pack.D, pack.Do
    assert tuple(params[0].shape) == (M, D) and tuple(params[1].shape) == (M, Do) and tuple(params[2].shape) == (M, Do)
    assert params[3].numel() == 1 and params[4].numel() == D
    o1, o2, o3, o4 = M * D, M * D + M * Do, M * D + 2 * M * Do, M * D + 2 * M * Do + 1
    pack.prepare(cflat[:o1].view(M, D), cflat[o4:], cflat[o3:o4], cflat[o1:o2].view(M, Do), cflat[o2:o3].view(M, Do))


def _gp_tail(layout, buf, red, image, kl_weight, pflat, cflat):
    lib = _l.load()
    work = torch.empty(int(lib.cbfssm_train_tail_half_work_elems(C.byref(layout))), dtype=torch.float64, device=buf.device)
    gflat = torch.empty_like(pflat)
    _l.check(lib.cbfssm_gp_tail_f64(C.byref(layout), _ptr(buf), _ptr(red), _ptr(image), 0, float(kl_weight), _ptr(pflat),
                                    _ptr(cflat), _ptr(work), _ptr(gflat), _stream()), 'cbfssm_gp_tail_f64')
    return gflat


def _gp_split(gflat, shapes, need):
    out, o = [], 0
    for s, nd in zip(shapes, need):
        n = 1
        for k in s:
            n *= k
        out.append(gflat[o:o + n].view(s) if nd else None)
        o += n
    return tuple(out)


class _GpPredict(torch.autograd.Function):

    @staticmethod
    def forward(ctx, pack, X, *params):
        pflat, cflat = _gp_flat(params)
        _gp_prepare(pack, params, cflat)
        Xd = X.detach().contiguous()
        fmean, fvar = pack.predict(Xd)
        ctx.layout, ctx.buf = pack.layout, pack.buf.clone()
        ctx.X, ctx.pflat, ctx.cflat = Xd, pflat, cflat
        ctx.shapes = tuple(tuple(p.shape) for p in params)
        return fmean, fvar

    @staticmethod
    @once_differentiable
    def backward(ctx, gmean, gvar):
        lib = _l.load()
        lay, buf, X = ctx.layout, ctx.buf, ctx.X
        need = ctx.needs_input_grad
        n, dev = X.shape[0], X.device
        need_p = any(need[2:])
        gX = torch.empty_like(X)
        if n == 0:
            gp = _gp_split(torch.zeros_like(ctx.pflat), ctx.shapes, need[2:])
            return (None, gX if need[1] else None) + gp
        gmean, gvar = gmean.contiguous(), gvar.contiguous()
        nwg = int(lib.cbfssm_gp_predict_bwd_workgroups(C.byref(lay), n))
        nwork = int(lib.cbfssm_gp_predict_bwd_work_elems(C.byref(lay), n))
        if nwg < 1 or nwork < 0:
            raise _l.CbfssmHipError('cbfssm_gp_predict_bwd_workgroups / _work_elems refused the layout')
        gpart = torch.empty((nwg + 32) * lay.rev_slab, dtype=torch.float64, device=dev)     # (+ CBFSSM_REDUCE_SPLIT)
        work = torch.empty(nwork, dtype=torch.float64, device=dev) if nwork else None
        image = torch.empty(lay.NBLK * lay.NBLK * 256, dtype=torch.float64, device=dev) if lay.rev_stash else None
        _l.check(lib.cbfssm_gp_predict_bwd_f64(C.byref(lay), _ptr(buf), _ptr(X), n, _ptr(gmean), _ptr(gvar), _ptr(gX),
                                               _ptr(gpart), _ptr(work), _ptr(image), _stream()), 'cbfssm_gp_predict_bwd_f64')
        gp = (None,) * 5
        if need_p:
            red = torch.empty(lay.rev_slab, dtype=torch.float64, device=dev)
            _l.check(lib.cbfssm_reduce_partials_f64(_ptr(gpart), lay.rev_slab, nwg, _ptr(red), _stream()),
                     'cbfssm_reduce_partials_f64')
            gp = _gp_split(_gp_tail(lay, buf, red, image, 0.0, ctx.pflat, ctx.cflat), ctx.shapes, need[2:])
        return (None, gX if need[1] else None) + gp


class _GpPriorKl(torch.autograd.Function):

    @staticmethod
    def forward(ctx, pack, *params):
        pflat, cflat = _gp_flat(params)
        _gp_prepare(pack, params, cflat)
        ctx.layout, ctx.buf = pack.layout, pack.buf.clone()
        ctx.pflat, ctx.cflat = pflat, cflat
        ctx.shapes = tuple(tuple(p.shape) for p in params)
        return pack.scal[_l.SCAL_KLZ].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        gflat = _gp_tail(ctx.layout, ctx.buf, None, None, 1.0, ctx.pflat, ctx.cflat) * gout
        return (None,) + _gp_split(gflat, ctx.shapes, ctx.needs_input_grad[1:])


def _gp_args(pack, params):
    if len(params) != 5:
        raise TypeError('expected the five tensors %s' % ', '.join(GP_PARAM_NAMES))
    dev = pack.buf.device
    return [torch.as_tensor(p, dtype=torch.float64, device=dev) for p in params]


def gp_predict(pack, X, *params):
    """GPModel.predict(X) -> (fmean (npts, Do), fvar (npts, Do)) with a grad_fn into X and the five parameter tensors."""
    X = torch.as_tensor(X, dtype=torch.float64, device=pack.buf.device)
    assert X.dim() == 2 and X.shape[1] == pack.D
    return _GpPredict.apply(pack, X, *_gp_args(pack, params))


def gp_prior_kl(pack, *params):
    """GPModel.prior_kl() as a 0-d tensor with a grad_fn into the five parameter tensors."""
    return _GpPriorKl.apply(pack, *_gp_args(pack, params))


# ---- one sparse GP with a full-covariance q(z): conditional() with q_sqrt (Do, M, M) (gp_tf.py:68-100) and the
# zeta_std.ndims == 3 branch of GPModel.predict (gp_tf.py:150-159) as torch functions ---------------------------------------
#
#     fmean, fvar = gp_predict_fullq(pack, X, zeta_pos, zeta_mean, q_sqrt, variance_unc, lengthscales_unc)
#     kl = gp_prior_kl_fullq(pack, zeta_pos, zeta_mean, q_sqrt, variance_unc, lengthscales_unc)
#
# q_sqrt holds the lower-triangular factors L_d, unconstrained; entries above the diagonal are never read and their gradient
# is exactly zero.  Forward of gp_predict_fullq: cbfssm_gp_fullq_prepare_f64 (S_d images, kept for the backward), then
# cbfssm_gp_fullq_predict_f64 on the f64 MFMA units.  Backward: cbfssm_gp_fullq_bwd_f64 -> cbfssm_reduce_partials_f64 ->
# cbfssm_gp_tail_fullq_f64 (kl_weight 0) for the four GP tensors, cbfssm_gp_fullq_wd_f64 -> cbfssm_gp_fullq_lbar_f64 for
# q_sqrt.  gp_prior_kl_fullq: cbfssm_gp_fullq_kl_f64; backward cbfssm_gp_tail_fullq_f64 without a slab (kl_weight 1) and
# cbfssm_gp_fullq_lbar_f64 without W.  As above: no host synchronisation, a copy of the prepared pack per call, once
# differentiable, only the requested gradients.

GP_FULLQ_PARAM_NAMES = ('zeta_pos', 'zeta_mean', 'zeta_sqrt', 'variance_unc', 'lengthscales_unc')


def _fq_flat(pack, zp, zm, var, ls):
    """(pflat, cflat) in cbfssm_gp_tail_fullq_f64's order: the zeta_var segment is a placeholder that no kernel reads"""
    hole = torch.zeros(pack.M * pack.Do, dtype=torch.float64, device=pack.buf.device)
    zp, zm, var, ls = [p.detach().reshape(-1) for p in (zp, zm, var, ls)]
    pflat = torch.cat([zp, zm, hole, var, ls]).contiguous()
    cflat = torch.cat([zp, zm, hole, tf_forward(var), tf_forward(ls)]).contiguous()
    return pflat, cflat


def _fq_prepare(pack, zp, zm, q, var, ls):
    M, D, Do = pack.M, pack.D, pack.Do
    assert tuple(zp.shape) == (M, D) and tuple(zm.shape) == (M, Do) and tuple(q.shape) == (Do, M, M)
    assert var.numel() == 1 and ls.numel() == D
    pflat, cflat = _fq_flat(pack, zp, zm, var, ls)
    o1, o2, o3 = M * D, M * D + M * Do, M * D + 2 * M * Do
    pack.prepare(cflat[:o1].view(M, D), cflat[o3 + 1:], cflat[o3:o3 + 1], cflat[o1:o2].view(M, Do), cflat[o2:o3].view(M, Do))
    return pflat, cflat


def _fq_qpack(lay, q):
    lib = _l.load()
    n = int(lib.cbfssm_gp_fullq_pack_elems(C.byref(lay)))
    if n < 1:
        raise _l.CbfssmHipError('cbfssm_gp_fullq_pack_elems refused the layout')
    qpack = torch.empty(n, dtype=torch.float64, device=q.device)
    _l.check(lib.cbfssm_gp_fullq_prepare_f64(C.byref(lay), _ptr(q), _ptr(qpack), _stream()), 'cbfssm_gp_fullq_prepare_f64')
    return qpack


def _fq_forward(lay, buf, qpack, X):
    """(fmean, fvar) of cbfssm_gp_fullq_predict_f64 on a prepared pack and q pack; nothing is launched without a point"""
    n = X.shape[0]
    fmean = torch.empty(n, lay.Do, dtype=torch.float64, device=buf.device)
    fvar = torch.empty_like(fmean)
    if n:
        _l.check(_l.load().cbfssm_gp_fullq_predict_f64(C.byref(lay), _ptr(buf), _ptr(qpack), _ptr(X), n, _ptr(fmean), _ptr(fvar),
                                                       _stream()), 'cbfssm_gp_fullq_predict_f64')
    return fmean, fvar


def _fq_kl(lay, buf, q, qpack, zeta_mean):
    kl = torch.empty(1, dtype=torch.float64, device=buf.device)
    _l.check(_l.load().cbfssm_gp_fullq_kl_f64(C.byref(lay), _ptr(buf), _ptr(q), _ptr(qpack), _ptr(zeta_mean), _ptr(kl), _stream()),
             'cbfssm_gp_fullq_kl_f64')
    return kl.reshape(())


def gp_fullq_eval(pack, X, q_sqrt, zeta_mean):
    """Evaluation only, on a PREPARED pack: (fmean, fvar) at X when X is given, else the prior KL.  Keeps nothing."""
    q = q_sqrt.detach().contiguous()
    if X is not None and X.shape[0] == 0:
        return _fq_forward(pack.layout, pack.buf, None, X)
    qpack = _fq_qpack(pack.layout, q)
    if X is not None:
        return _fq_forward(pack.layout, pack.buf, qpack, X.detach().contiguous())
    return _fq_kl(pack.layout, pack.buf, q, qpack, zeta_mean.detach().contiguous())


def _fq_tail(lay, buf, qpack, red, image, kl_weight, pflat, cflat):
    lib = _l.load()
    work = torch.empty(int(lib.cbfssm_train_tail_half_work_elems(C.byref(lay))), dtype=torch.float64, device=buf.device)
    gflat = torch.empty_like(pflat)
    _l.check(lib.cbfssm_gp_tail_fullq_f64(C.byref(lay), _ptr(buf), _ptr(qpack), _ptr(red), _ptr(image), 0, float(kl_weight),
                                          _ptr(pflat), _ptr(cflat), _ptr(work), _ptr(gflat), _stream()),
             'cbfssm_gp_tail_fullq_f64')
    return gflat


def _fq_split(gflat, gq, shapes, need):
    """gradients in the order (zeta_pos, zeta_mean, q_sqrt, variance_unc, lengthscales_unc)"""
    M_Do = shapes[1]
    gp = (None,) * 5 if gflat is None else _gp_split(gflat, (shapes[0], shapes[1], M_Do, shapes[3], shapes[4]),
                                                     (need[0], need[1], False, need[3], need[4]))
    return (gp[0], gp[1], gq if need[2] else None, gp[3], gp[4])


class _GpPredictFullq(torch.autograd.Function):

    @staticmethod
    def forward(ctx, pack, X, zp, zm, q, var, ls):
        lib = _l.load()
        pflat, cflat = _fq_prepare(pack, zp, zm, q, var, ls)
        Xd, qd = X.detach().contiguous(), q.detach().contiguous().clone()
        lay, n = pack.layout, X.shape[0]
        qpack = _fq_qpack(lay, qd) if n else None                            # (no launch without a point)
        fmean, fvar = _fq_forward(lay, pack.buf, qpack, Xd)
        ctx.layout, ctx.buf, ctx.qpack = lay, pack.buf.clone(), qpack
        ctx.X, ctx.q, ctx.pflat, ctx.cflat = Xd, qd, pflat, cflat
        ctx.shapes = tuple(tuple(p.shape) for p in (zp, zm, q, var, ls))
        return fmean, fvar

    @staticmethod
    @once_differentiable
    def backward(ctx, gmean, gvar):
        lib = _l.load()
        lay, buf, X, q = ctx.layout, ctx.buf, ctx.X, ctx.q
        need = ctx.needs_input_grad
        n, dev = X.shape[0], X.device
        gX = torch.empty_like(X)
        if n == 0:
            gp = _fq_split(torch.zeros_like(ctx.pflat), torch.zeros_like(q), ctx.shapes, need[2:])
            return (None, gX if need[1] else None) + gp
        gmean, gvar = gmean.contiguous(), gvar.contiguous()
        nwg = int(lib.cbfssm_gp_fullq_bwd_workgroups(C.byref(lay), n))
        nwork = int(lib.cbfssm_gp_fullq_bwd_work_elems(C.byref(lay), n))
        na2 = int(lib.cbfssm_gp_fullq_a2_elems(C.byref(lay), n))
        if nwg < 1 or nwork < 0 or na2 < 1:
            raise _l.CbfssmHipError('cbfssm_gp_fullq_bwd_workgroups / _work_elems / _a2_elems refused the layout')
        qpack = ctx.qpack
        gpart = torch.empty((nwg + 32) * lay.rev_slab, dtype=torch.float64, device=dev)     # (+ CBFSSM_REDUCE_SPLIT)
        a2 = torch.empty(na2, dtype=torch.float64, device=dev)
        work = torch.empty(nwork, dtype=torch.float64, device=dev) if nwork else None
        image = torch.empty(lay.NBLK * lay.NBLK * 256, dtype=torch.float64, device=dev) if lay.rev_stash else None
        _l.check(lib.cbfssm_gp_fullq_bwd_f64(C.byref(lay), _ptr(buf), _ptr(qpack), _ptr(X), n, _ptr(gmean), _ptr(gvar),
                                             _ptr(gX), _ptr(gpart), _ptr(a2), _ptr(work), _ptr(image), _stream()),
                 'cbfssm_gp_fullq_bwd_f64')
        gflat = gq = None
        if need[2] or need[3] or need[5] or need[6]:
            red = torch.empty(lay.rev_slab, dtype=torch.float64, device=dev)
            _l.check(lib.cbfssm_reduce_partials_f64(_ptr(gpart), lay.rev_slab, nwg, _ptr(red), _stream()),
                     'cbfssm_reduce_partials_f64')
            gflat = _fq_tail(lay, buf, qpack, red, image, 0.0, ctx.pflat, ctx.cflat)
        if need[4]:
            wwork = torch.empty(int(lib.cbfssm_gp_fullq_wd_work_elems(C.byref(lay), n)), dtype=torch.float64, device=dev)
            W = torch.empty_like(q)
            _l.check(lib.cbfssm_gp_fullq_wd_f64(C.byref(lay), _ptr(a2), _ptr(gvar), n, _ptr(wwork), _ptr(W), _stream()),
                     'cbfssm_gp_fullq_wd_f64')
            gq = torch.empty_like(q)
            _l.check(lib.cbfssm_gp_fullq_lbar_f64(C.byref(lay), None, _ptr(q), _ptr(W), 0.0, _ptr(gq), _stream()),
                     'cbfssm_gp_fullq_lbar_f64')
        return (None, gX if need[1] else None) + _fq_split(gflat, gq, ctx.shapes, need[2:])


class _GpPriorKlFullq(torch.autograd.Function):

    @staticmethod
    def forward(ctx, pack, zp, zm, q, var, ls):
        lib = _l.load()
        pflat, cflat = _fq_prepare(pack, zp, zm, q, var, ls)
        qd = q.detach().contiguous().clone()
        lay = pack.layout
        qpack = _fq_qpack(lay, qd)
        o1 = pack.M * pack.D
        kl = _fq_kl(lay, pack.buf, qd, qpack, cflat[o1:o1 + pack.M * pack.Do])
        ctx.layout, ctx.buf = lay, pack.buf.clone()
        ctx.q, ctx.qpack, ctx.pflat, ctx.cflat = qd, qpack, pflat, cflat
        ctx.shapes = tuple(tuple(p.shape) for p in (zp, zm, q, var, ls))
        return kl

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        lib = _l.load()
        need = ctx.needs_input_grad[1:]
        gflat = gq = None
        if need[0] or need[1] or need[3] or need[4]:
            gflat = _fq_tail(ctx.layout, ctx.buf, ctx.qpack, None, None, 1.0, ctx.pflat, ctx.cflat) * gout
        if need[2]:
            gq = torch.empty_like(ctx.q)
            _l.check(lib.cbfssm_gp_fullq_lbar_f64(C.byref(ctx.layout), _ptr(ctx.buf), _ptr(ctx.q), None, 1.0, _ptr(gq),
                                                  _stream()), 'cbfssm_gp_fullq_lbar_f64')
            gq = gq * gout
        return (None,) + _fq_split(gflat, gq, ctx.shapes, need)


# ---- conditional() with q_sqrt None or (M, Do) (gp_tf.py:68-88): gp_predict's kernels, with the marginal variances
# s2 = q_sqrt^2 themselves as the third tensor -- no positivity transform, so q_sqrt^2 below 1e-10 (not a value of
# softplus + 1e-10) is as good as any other.  d loss / d s2 is the sigma_z^2 section of the reduced slab as it stands.

def _slab_s2_index(lay, M, Do, dev):
    """positions of (m, d) in the sigma_z^2 section of the slab: an MFMA C-layout image [NBLK][4][64] behind the mean's"""
    m = torch.arange(M, device=dev).view(M, 1)
    d = torch.arange(Do, device=dev).view(1, Do)
    rr = m & 15
    return lay.NBLK * 256 + ((m >> 4) * 4 + (rr >> 2)) * 64 + 16 * (rr & 3) + d


class _GpConditionalDiag(torch.autograd.Function):

    @staticmethod
    def forward(ctx, pack, Xnew, Z, f, s2, var, ls):
        M, D, Do = pack.M, pack.D, pack.Do
        assert tuple(Z.shape) == (M, D) and tuple(f.shape) == (M, Do) and tuple(s2.shape) == (M, Do)
        assert var.numel() == 1 and ls.numel() == D
        zp, zm, zv, v, l = [p.detach().reshape(-1) for p in (Z, f, s2, var, ls)]
        pflat = torch.cat([zp, zm, torch.zeros_like(zv), v, l]).contiguous()      # (the zeta_var_unc entries are a placeholder)
        cflat = torch.cat([zp, zm, zv, tf_forward(v), tf_forward(l)]).contiguous()
        _gp_prepare(pack, (Z, f, s2, var, ls), cflat)
        Xd = Xnew.detach().contiguous()
        fmean, fvar = pack.predict(Xd)
        ctx.layout, ctx.buf = pack.layout, pack.buf.clone()
        ctx.X, ctx.pflat, ctx.cflat = Xd, pflat, cflat
        ctx.shapes = tuple(tuple(p.shape) for p in (Z, f, s2, var, ls))
        return fmean, fvar

    @staticmethod
    @once_differentiable
    def backward(ctx, gmean, gvar):
        lib = _l.load()
        lay, buf, X = ctx.layout, ctx.buf, ctx.X
        need = ctx.needs_input_grad
        n, dev = X.shape[0], X.device
        gX = torch.empty_like(X)
        if n == 0:
            gp = _gp_split(torch.zeros_like(ctx.pflat), ctx.shapes, need[2:])
            return (None, gX if need[1] else None) + gp
        gmean, gvar = gmean.contiguous(), gvar.contiguous()
        nwg = int(lib.cbfssm_gp_predict_bwd_workgroups(C.byref(lay), n))
        nwork = int(lib.cbfssm_gp_predict_bwd_work_elems(C.byref(lay), n))
        if nwg < 1 or nwork < 0:
            raise _l.CbfssmHipError('cbfssm_gp_predict_bwd_workgroups / _work_elems refused the layout')
        gpart = torch.empty((nwg + 32) * lay.rev_slab, dtype=torch.float64, device=dev)     # (+ CBFSSM_REDUCE_SPLIT)
        work = torch.empty(nwork, dtype=torch.float64, device=dev) if nwork else None
        image = torch.empty(lay.NBLK * lay.NBLK * 256, dtype=torch.float64, device=dev) if lay.rev_stash else None
        _l.check(lib.cbfssm_gp_predict_bwd_f64(C.byref(lay), _ptr(buf), _ptr(X), n, _ptr(gmean), _ptr(gvar), _ptr(gX),
                                               _ptr(gpart), _ptr(work), _ptr(image), _stream()), 'cbfssm_gp_predict_bwd_f64')
        gp = [None] * 5
        if any(need[2:]):
            red = torch.empty(lay.rev_slab, dtype=torch.float64, device=dev)
            _l.check(lib.cbfssm_reduce_partials_f64(_ptr(gpart), lay.rev_slab, nwg, _ptr(red), _stream()),
                     'cbfssm_reduce_partials_f64')
            if need[2] or need[3] or need[5] or need[6]:
                gp = list(_gp_split(_gp_tail(lay, buf, red, image, 0.0, ctx.pflat, ctx.cflat), ctx.shapes, need[2:]))
            if need[4]:
                M, Do = ctx.shapes[2]
                gp[2] = red[_slab_s2_index(lay, M, Do, dev)]
            else:
                gp[2] = None
        return (None, gX if need[1] else None) + tuple(gp)


def gp_conditional_diag(pack, Xnew, Z, f, s2, variance_unc, lengthscales_unc):
    """conditional(Xnew, Z, kern, f, q_sqrt) for q_sqrt None (s2 = 0) or (M, Do) (s2 = q_sqrt^2, CONSTRAINED marginal
    variances) -> (fmean, fvar) with a grad_fn into Xnew, Z, f, s2 and the kernel's two unconstrained tensors."""
    dev = pack.buf.device
    args = [torch.as_tensor(p, dtype=torch.float64, device=dev) for p in (Xnew, Z, f, s2, variance_unc, lengthscales_unc)]
    assert args[0].dim() == 2 and args[0].shape[1] == pack.D
    return _GpConditionalDiag.apply(pack, *args)


def _fq_args(pack, params):
    if len(params) != 5:
        raise TypeError('expected the five tensors %s' % ', '.join(GP_FULLQ_PARAM_NAMES))
    dev = pack.buf.device
    return [torch.as_tensor(p, dtype=torch.float64, device=dev) for p in params]


def gp_predict_fullq(pack, X, *params):
    """The full-covariance conditional -> (fmean (npts, Do), fvar (npts, Do)) with a grad_fn into X, zeta_pos, zeta_mean,
    q_sqrt (Do, M, M), variance_unc and lengthscales_unc."""
    X = torch.as_tensor(X, dtype=torch.float64, device=pack.buf.device)
    assert X.dim() == 2 and X.shape[1] == pack.D
    return _GpPredictFullq.apply(pack, X, *_fq_args(pack, params))


def gp_prior_kl_fullq(pack, *params):
    """KL(N(zeta_mean_d, L_d L_d^T) || N(0, K)) summed over the output dimensions, as a 0-d tensor with a grad_fn."""
    return _GpPriorKlFullq.apply(pack, *_fq_args(pack, params))


# ---- the recurrence of one sparse GP: h <- h + gp(h, a_t) + eps_t sqrt(fvar + var_add) over time, one launch ------------
#
#     traj, entropy = gp_rollout(pack, h0, a, eps, var_add, zeta_pos, zeta_mean, zeta_var_unc, variance_unc, lengthscales_unc,
#                                reverse=False)
#
# h0 (N, Do), a (T, N, Da) with Da = D - Do (None or (T, N, 0) when Da = 0), eps (T, N) standard normals, var_add (Do)
# CONSTRAINED values or None; traj (T, N, Do) time-major, entropy = 0.5 sum log(2 pi e (fvar + var_add)) a 0-d tensor.
# Voliro's recognition run (cbfssm/model/voliro.py:139-186) is reverse=True from h0 = 0 with a = (u_t, y_t) per particle;
# the free-running transition of a trained CBF-SSM (cbfssm/model/cbfssm.py:199-206,224) is reverse=False with a = u_t.
# Forward: cbfssm_gp_rollout_f64, the entropy partials summed in a fixed order by cbfssm_reduce_partials_f64.  Backward:
# cbfssm_gp_rollout_bwd_f64 -> cbfssm_reduce_partials_f64 -> cbfssm_gp_tail_f64 (kl_weight 0); gradients for h0, a, var_add
# and the five parameter tensors, none for eps.  Once differentiable, no host synchronisation; the call keeps a copy of the
# prepared pack, as gp_predict does.

def _rollout_forward(lay, buf, h0, a, eps, var_add, reverse, save):
    """(traj, vsave or None, entropy) of one forward launch on prepared pack operands"""
    lib = _l.load()
    T, N = eps.shape
    Do, dev = lay.Do, buf.device
    if T < 1:
        raise ValueError('gp_rollout: at least one time step')
    traj = torch.empty(T, N, Do, dtype=torch.float64, device=dev)
    vsave = torch.empty_like(traj) if save else None
    if N == 0:
        return traj, vsave, torch.zeros((), dtype=torch.float64, device=dev)
    npart = int(lib.cbfssm_gp_rollout_partials(C.byref(lay), N))
    if npart < 1:
        raise _l.CbfssmHipError('cbfssm_gp_rollout_partials refused the layout')
    ent_part = torch.empty(npart + 32, dtype=torch.float64, device=dev)                     # (+ CBFSSM_REDUCE_SPLIT)
    _l.check(lib.cbfssm_gp_rollout_f64(C.byref(lay), _ptr(buf), _ptr(h0), _ptr(a), _ptr(eps), _ptr(var_add), N, T,
                                       int(bool(reverse)), _ptr(traj), _ptr(vsave), _ptr(ent_part), _stream()),
             'cbfssm_gp_rollout_f64')
    ent = torch.empty(1, dtype=torch.float64, device=dev)
    _l.check(lib.cbfssm_reduce_partials_f64(_ptr(ent_part), 1, npart, _ptr(ent), _stream()), 'cbfssm_reduce_partials_f64')
    return traj, vsave, ent.reshape(())


def _rollout_args(pack, h0, a, eps, var_add):
    dev = pack.buf.device
    Do, Da = pack.Do, pack.D - pack.Do
    if Da < 0:
        raise ValueError('gp_rollout: the GP input dimension %d is smaller than its output dimension %d' % (pack.D, pack.Do))
    eps = torch.as_tensor(eps, dtype=torch.float64, device=dev)
    h0 = torch.as_tensor(h0, dtype=torch.float64, device=dev)
    assert eps.dim() == 2 and h0.dim() == 2 and h0.shape == (eps.shape[1], Do), 'eps (T, N), h0 (N, Do)'
    T, N = eps.shape
    if Da == 0:
        assert a is None or tuple(a.shape) == (T, N, 0), 'a: None or (T, N, 0) when the GP takes the state alone'
        a = None
    else:
        a = torch.as_tensor(a, dtype=torch.float64, device=dev)
        assert tuple(a.shape) == (T, N, Da), 'a (T, N, D - Do)'
    if var_add is not None:
        var_add = torch.as_tensor(var_add, dtype=torch.float64, device=dev)
        assert var_add.shape == (Do,), 'var_add (Do)'
    return h0, a, eps, var_add


class _GpRollout(torch.autograd.Function):

    @staticmethod
    def forward(ctx, pack, reverse, h0, a, eps, var_add, *params):
        pflat, cflat = _gp_flat(params)
        _gp_prepare(pack, params, cflat)
        h0d, epsd = h0.detach().contiguous(), eps.detach().contiguous()
        ad = a.detach().contiguous() if a is not None else None
        vad = var_add.detach().contiguous() if var_add is not None else None
        buf = pack.buf.clone()
        traj, vsave, ent = _rollout_forward(pack.layout, buf, h0d, ad, epsd, vad, reverse, True)
        ctx.layout, ctx.buf, ctx.reverse = pack.layout, buf, bool(reverse)
        ctx.has_a = ad is not None
        ctx.save_for_backward(h0d, epsd, traj, vsave, *([ad] if ad is not None else []))     # (traj is an output)
        ctx.pflat, ctx.cflat = pflat, cflat
        ctx.shapes = tuple(tuple(p.shape) for p in params)
        return traj, ent

    @staticmethod
    @once_differentiable
    def backward(ctx, gtraj, gent):
        lib = _l.load()
        lay, buf = ctx.layout, ctx.buf
        h0, eps, traj, vsave = ctx.saved_tensors[:4]
        a = ctx.saved_tensors[4] if ctx.has_a else None
        need = ctx.needs_input_grad
        T, N = eps.shape
        dev = eps.device
        gh0 = torch.empty_like(h0)
        ga = torch.empty_like(a) if a is not None else None
        if N == 0:
            gp = _gp_split(torch.zeros_like(ctx.pflat), ctx.shapes, need[6:])
            gva = torch.zeros(lay.Do, dtype=torch.float64, device=dev) if need[5] else None
            return (None, None, gh0 if need[2] else None, ga if need[3] else None, None, gva) + gp
        gtraj = gtraj.contiguous()
        gent = gent.reshape(1).contiguous()
        nwg = int(lib.cbfssm_gp_rollout_bwd_workgroups(C.byref(lay), N))
        nwork = int(lib.cbfssm_gp_rollout_bwd_work_elems(C.byref(lay), N, T))
        if nwg < 1 or nwork < 0:
            raise _l.CbfssmHipError('cbfssm_gp_rollout_bwd_workgroups / _work_elems refused the layout')
        gpart = torch.empty((nwg + 32) * lay.rev_slab, dtype=torch.float64, device=dev)     # (+ CBFSSM_REDUCE_SPLIT)
        work = torch.empty(nwork, dtype=torch.float64, device=dev) if nwork else None
        image = torch.empty(lay.NBLK * lay.NBLK * 256, dtype=torch.float64, device=dev) if lay.rev_stash else None
        _l.check(lib.cbfssm_gp_rollout_bwd_f64(C.byref(lay), _ptr(buf), _ptr(h0), _ptr(a), _ptr(eps), _ptr(traj), _ptr(vsave),
                                               _ptr(gtraj), _ptr(gent), N, T, int(ctx.reverse), _ptr(gh0), _ptr(ga),
                                               _ptr(gpart), _ptr(work), _ptr(image), _stream()), 'cbfssm_gp_rollout_bwd_f64')
        gp, gva = (None,) * 5, None
        if need[5] or any(need[6:]):
            red = torch.empty(lay.rev_slab, dtype=torch.float64, device=dev)
            _l.check(lib.cbfssm_reduce_partials_f64(_ptr(gpart), lay.rev_slab, nwg, _ptr(red), _stream()),
                     'cbfssm_reduce_partials_f64')
            if need[5]:
                small = lay.rev_slab - 192                  # the slab's scalars: [0, 16) d/d var_x by state dim
                gva = red[small:small + lay.Do].clone()
            if any(need[6:]):
                gp = _gp_split(_gp_tail(lay, buf, red, image, 0.0, ctx.pflat, ctx.cflat), ctx.shapes, need[6:])
        return (None, None, gh0 if need[2] else None, ga if need[3] else None, None, gva) + gp


def gp_rollout(pack, h0, a, eps, var_add, *params, reverse=False):
    """(traj (T, N, Do), entropy ()) of the recurrence above with a grad_fn into h0, a, var_add and the five parameter tensors."""
    h0, a, eps, var_add = _rollout_args(pack, h0, a, eps, var_add)
    return _GpRollout.apply(pack, bool(reverse), h0, a, eps.detach(), var_add, *_gp_args(pack, params))


def gp_rollout_eval(pack, h0, a, eps, var_add, reverse=False):
    """The forward launch alone on a pack that is already prepared: no saved variances, no grad_fn."""
    h0, a, eps, var_add = _rollout_args(pack, h0, a, eps, var_add)
    with torch.no_grad():
        traj, _, ent = _rollout_forward(pack.layout, pack.buf, h0.contiguous(), a.contiguous() if a is not None else None,
                                        eps.contiguous(), var_add.contiguous() if var_add is not None else None, reverse, False)
    return traj, ent


# ---- the local linear model of one sparse GP: d fmean / d X and d fvar / d X at a batch of points -------------------------
#
#     fmean, fvar, dmean, dvar = gp_linearize_eval(pack, X, variance=True)
#
# what the reference gets from tf.gradients(fmean[:, d], Xnew) / tf.gradients(fvar[:, d], Xnew) per output dimension d
# through gp_tf.py:132-161, as one launch for all dimensions (cbfssm_gp_linearize_f64: per 16 points one kernel tile,
# 1 + Do products with K^-1 and the (Z / lengthscale)^T products) instead of 2 Do backward calls through gp_predict.

def gp_linearize_eval(pack, X, variance=True):
    """(fmean (npts, Do), fvar (npts, Do), dmean (npts, Do, D), dvar (npts, Do, D) or None) on a pack that is already
    prepared: dmean[n, d, i] = d fmean[n, d] / d X[n, i], dvar the same of fvar.  variance=False leaves the variance
    Jacobian (and its K^-1 product per output dimension) out; dmean and fmean are bitwise those of the full call.
    Evaluation only: no grad_fn, no host synchronisation, nothing is launched without a point."""
    lib = _l.load()
    lay, dev = pack.layout, pack.buf.device
    X = torch.as_tensor(X, dtype=torch.float64, device=dev)
    assert X.dim() == 2 and X.shape[1] == pack.D, 'X (npts, D)'
    n, D, Do = X.shape[0], pack.D, pack.Do
    with torch.no_grad():
        X = X.detach().contiguous()
        fmean = torch.empty(n, Do, dtype=torch.float64, device=dev)
        fvar = torch.empty_like(fmean)
        dmean = torch.empty(n, Do, D, dtype=torch.float64, device=dev)
        dvar = torch.empty_like(dmean) if variance else None
        if n == 0:
            return fmean, fvar, dmean, dvar
        nwork = int(lib.cbfssm_gp_linearize_work_elems(C.byref(lay)))
        if nwork < 1:
            raise _l.CbfssmHipError('cbfssm_gp_linearize_work_elems refused the layout')
        work = torch.empty(nwork, dtype=torch.float64, device=dev)
        _l.check(lib.cbfssm_gp_linearize_f64(C.byref(lay), _ptr(pack.buf), _ptr(X), n, _ptr(fmean), _ptr(fvar), _ptr(dmean),
                                             _ptr(dvar), _ptr(work), _stream()), 'cbfssm_gp_linearize_f64')
    return fmean, fvar, dmean, dvar


# ---- exact Gaussian moments of one sparse GP under a Gaussian input: moment matching ---------------------------------------
#
#     fmean, fcov, xcov, info = gp_moment_match_eval(pack, mean, cov, cross=True)
#
# for x ~ N(mean[n], cov[n]) and the posterior of gp_tf.py:132-161: E[f], Cov(f, f) with the correlation between output
# dimensions that the shared uncertain input brings, Cov(f, x) -- closed form for the RBF kernel, one launch
# (cbfssm_gp_moment_match_f64: per point two D x D Cholesky factorisations, the M x M matrix of expected kernel products as
# register tiles) instead of an (npts, M, M) intermediate in the tensor library.

def gp_moment_match_eval(pack, mean, cov, cross=True):
    """(fmean (npts, Do), fcov (npts, Do, Do), xcov (npts, Do, D) or None, info (npts) int64) on a pack that is already
    prepared.  mean (npts, D); cov (npts, D, D), only the lower triangle is read, or None (zero: predict, with xcov = 0).
    cross=False leaves xcov out; the other results are bitwise those of the full call.  info[n] != 0: cov[n] is not
    positive semi-definite and the results of point n are NaN.  Evaluation only: no grad_fn, nothing is launched without
    a point; reading info as int64 is a device-side cast, not a host synchronisation."""
    lib = _l.load()
    lay, dev = pack.layout, pack.buf.device
    mean = torch.as_tensor(mean, dtype=torch.float64, device=dev)
    assert mean.dim() == 2 and mean.shape[1] == pack.D, 'mean (npts, D)'
    n, D, Do = mean.shape[0], pack.D, pack.Do
    if cov is not None:
        cov = torch.as_tensor(cov, dtype=torch.float64, device=dev)
        assert tuple(cov.shape) == (n, D, D), 'cov (npts, D, D)'
    with torch.no_grad():
        mean = mean.detach().contiguous()
        cov = cov.detach().contiguous() if cov is not None else None
        fmean = torch.empty(n, Do, dtype=torch.float64, device=dev)
        fcov = torch.empty(n, Do, Do, dtype=torch.float64, device=dev)
        xcov = torch.empty(n, Do, D, dtype=torch.float64, device=dev) if cross else None
        info = torch.empty(n, dtype=torch.float64, device=dev)
        if n == 0:
            return fmean, fcov, xcov, info.to(torch.int64)
        nwork = int(lib.cbfssm_gp_moment_match_work_elems(C.byref(lay)))
        if nwork < 1:
            raise _l.CbfssmHipError('cbfssm_gp_moment_match_work_elems refused the layout')
        work = torch.empty(nwork, dtype=torch.float64, device=dev)
        _l.check(lib.cbfssm_gp_moment_match_f64(C.byref(lay), _ptr(pack.buf), _ptr(mean), _ptr(cov), n, _ptr(fmean), _ptr(fcov),
                                                _ptr(xcov), _ptr(info), _ptr(work), _stream()), 'cbfssm_gp_moment_match_f64')
    return fmean, fcov, xcov, info.to(torch.int64)


# The same results with a grad_fn into the inputs of the call:
#
#     fmean, fcov, xcov, info = gp_moment_match(pack, mean, cov, cross=True)
#
# The model is a constant: the pack's values at the forward call are what the backward differentiates (the context keeps a
# copy of the pack, as _GpPredict does), and no parameter tensor receives a gradient.  The backward is one adjoint launch
# behind the forward's two pre-kernels (cbfssm_gp_moment_match_bwd_f64), which recomputes the forward quantities; a result the
# loss does not use arrives as None and goes down as a NULL cotangent, whose terms the kernel skips.

class _GpMomentMatch(torch.autograd.Function):

    @staticmethod
    def forward(ctx, pack, mean, cov, cross):
        fmean, fcov, xcov, info = gp_moment_match_eval(pack, mean, cov, cross=cross)
        ctx.set_materialize_grads(False)
        ctx.layout, ctx.buf = pack.layout, (pack.buf.clone() if mean.shape[0] else None)
        ctx.mean = mean.detach().contiguous()
        ctx.cov = cov.detach().contiguous() if cov is not None else None
        ctx.mark_non_differentiable(info)
        if cross:
            return fmean, fcov, xcov, info
        return fmean, fcov, info

    @staticmethod
    @once_differentiable
    def backward(ctx, gfmean, gfcov, *rest):
        gxcov = rest[0] if len(rest) == 2 else None
        lib = _l.load()
        lay, mean, cov = ctx.layout, ctx.mean, ctx.cov
        need = ctx.needs_input_grad
        n, dev = mean.shape[0], mean.device
        if gfmean is None and gfcov is None and gxcov is None:
            return None, None, None, None
        # NaN-filled, not uninitialised: the kernel writes every entry of both gradients and reads nothing of `work` that this
        # call did not write, and the fill is a few percent of the launch at most -- so every call is a poisoned-buffer run
        nan = float('nan')
        gmean = torch.full_like(mean, nan)
        gcov = torch.full_like(cov, nan) if cov is not None else None
        if n:
            gfmean = gfmean.contiguous() if gfmean is not None else None
            gfcov = gfcov.contiguous() if gfcov is not None else None
            gxcov = gxcov.contiguous() if gxcov is not None else None
            nwork = int(lib.cbfssm_gp_moment_match_bwd_work_elems(C.byref(lay)))
            if nwork < 1:
                raise _l.CbfssmHipError('cbfssm_gp_moment_match_bwd_work_elems refused the layout')
            work = torch.full((nwork,), nan, dtype=torch.float64, device=dev)
            _l.check(lib.cbfssm_gp_moment_match_bwd_f64(C.byref(lay), _ptr(ctx.buf), _ptr(mean), _ptr(cov), n, _ptr(gfmean),
                                                        _ptr(gfcov), _ptr(gxcov), _ptr(gmean), _ptr(gcov), None, _ptr(work),
                                                        _stream()), 'cbfssm_gp_moment_match_bwd_f64')
        return None, (gmean if need[1] else None), (gcov if cov is not None and need[2] else None), None


def gp_moment_match(pack, mean, cov, cross=True):
    """gp_moment_match_eval's results on a prepared pack, with a grad_fn on fmean, fcov and xcov into `mean` and `cov` when
    grad is enabled and one of them requires it (else the evaluation call itself).  The values are bitwise those of the
    evaluation call; info never carries a grad_fn.  The gradient for cov is that of the function of
    tril(cov) + tril(cov, -1)^T: exactly zero above the diagonal, both symmetric contributions on a strictly lower entry;
    cov=None has no gradient and the gradient for mean is then the input gradient of predict.  The model is a constant of
    the call: no parameter tensor is connected to these results.  Where info[n] != 0 the rows of point n of both gradients
    are NaN.  Once differentiable; float64."""
    dev = pack.buf.device
    mean = torch.as_tensor(mean, dtype=torch.float64, device=dev)
    assert mean.dim() == 2 and mean.shape[1] == pack.D, 'mean (npts, D)'
    if cov is not None:
        cov = torch.as_tensor(cov, dtype=torch.float64, device=dev)
        assert tuple(cov.shape) == (mean.shape[0], pack.D, pack.D), 'cov (npts, D, D)'
    if not (torch.is_grad_enabled() and (mean.requires_grad or (cov is not None and cov.requires_grad))):
        return gp_moment_match_eval(pack, mean, cov, cross=cross)
    out = _GpMomentMatch.apply(pack, mean, cov, bool(cross))
    if cross:
        return out
    return out[0], out[1], None, out[2]


# ... and with a grad_fn into the MODEL as well, the five tensors of GP_PARAM_NAMES:
#
#     fmean, fcov, xcov, info = gp_moment_match_params(pack, mean, cov, zeta_pos, zeta_mean, zeta_var_unc, variance_unc,
#                                                      lengthscales_unc, cross=True)
#
# Forward: the pack is prepared from the leaves, then the evaluation launch (bitwise its values).  Backward: the input
# adjoint launch (cbfssm_gp_moment_match_bwd_f64: gmean, gcov -- bitwise those of gp_moment_match), then, when a leaf wants
# a gradient, cbfssm_gp_moment_match_params_bwd_f64 (one reduced slab; it contracts gmean and gcov with the inputs for the
# belief's side of the lengthscale adjoint) and cbfssm_gp_tail_f64 with kl_weight 0.  The context keeps pack.buf.clone(),
# pflat and cflat, as _GpEkf does.  Every buffer of the backward is filled with NaN before the launches: the kernels read
# nothing they did not write.

class _GpMomentMatchParams(torch.autograd.Function):

    @staticmethod
    def forward(ctx, pack, cross, mean, cov, *params):
        pflat, cflat = _gp_flat(params)
        n = mean.shape[0]
        ctx.set_materialize_grads(False)
        ctx.pflat, ctx.cflat = pflat, cflat
        ctx.shapes = tuple(tuple(p.shape) for p in params)
        ctx.mean = mean.detach().contiguous()
        ctx.cov = cov.detach().contiguous() if cov is not None else None
        if n:                                           # (without a point nothing is prepared or launched)
            _gp_prepare(pack, params, cflat)
        fmean, fcov, xcov, info = gp_moment_match_eval(pack, ctx.mean, ctx.cov, cross=cross)
        ctx.layout, ctx.buf = pack.layout, (pack.buf.clone() if n else None)
        ctx.mark_non_differentiable(info)
        if cross:
            ctx.save_for_backward(xcov)                 # (an output: the lengthscales scale it)
            return fmean, fcov, xcov, info
        return fmean, fcov, info

    @staticmethod
    @once_differentiable
    def backward(ctx, gfmean, gfcov, *rest):
        gxcov = rest[0] if len(rest) == 2 else None
        lib = _l.load()
        lay, mean, cov = ctx.layout, ctx.mean, ctx.cov
        need = ctx.needs_input_grad                     # 2 mean, 3 cov, 4.. the leaves
        n, dev = mean.shape[0], mean.device
        if gfmean is None and gfcov is None and gxcov is None:
            return (None,) * 9
        nan = float('nan')
        if n == 0:
            gp = _gp_split(torch.zeros_like(ctx.pflat), ctx.shapes, need[4:])
            return (None, None, torch.zeros_like(mean) if need[2] else None,
                    torch.zeros_like(cov) if cov is not None and need[3] else None) + gp
        gmean = torch.full_like(mean, nan)
        gcov = torch.full_like(cov, nan) if cov is not None else None
        gfmean = gfmean.contiguous() if gfmean is not None else None
        gfcov = gfcov.contiguous() if gfcov is not None else None
        gxcov = gxcov.contiguous() if gxcov is not None else None
        nwork = int(lib.cbfssm_gp_moment_match_bwd_work_elems(C.byref(lay)))
        if nwork < 1:
            raise _l.CbfssmHipError('cbfssm_gp_moment_match_bwd_work_elems refused the layout')
        work = torch.full((nwork,), nan, dtype=torch.float64, device=dev)
        _l.check(lib.cbfssm_gp_moment_match_bwd_f64(C.byref(lay), _ptr(ctx.buf), _ptr(mean), _ptr(cov), n, _ptr(gfmean),
                                                    _ptr(gfcov), _ptr(gxcov), _ptr(gmean), _ptr(gcov), None, _ptr(work),
                                                    _stream()), 'cbfssm_gp_moment_match_bwd_f64')
        gp = (None,) * 5
        if any(need[4:]):
            xcov = ctx.saved_tensors[0] if ctx.saved_tensors else None
            nwork = int(lib.cbfssm_gp_moment_match_params_bwd_work_elems(C.byref(lay), n))
            ntail = int(lib.cbfssm_train_tail_half_work_elems(C.byref(lay)))
            if nwork < 1 or ntail < 1:
                raise _l.CbfssmHipError('cbfssm_gp_moment_match_params_bwd_work_elems refused the layout')
            work = torch.full((nwork,), nan, dtype=torch.float64, device=dev)
            red = torch.full((lay.rev_slab,), nan, dtype=torch.float64, device=dev)
            dense = torch.full((lay.M * lay.M,), nan, dtype=torch.float64, device=dev) if lay.rev_stash else None
            _l.check(lib.cbfssm_gp_moment_match_params_bwd_f64(C.byref(lay), _ptr(ctx.buf), _ptr(ctx.cflat), _ptr(mean),
                                                               _ptr(cov), n, _ptr(gfmean), _ptr(gfcov), _ptr(gxcov),
                                                               _ptr(gmean), _ptr(gcov), _ptr(xcov), _ptr(red), _ptr(dense),
                                                               _ptr(work), _stream()), 'cbfssm_gp_moment_match_params_bwd_f64')
            twork = torch.full((ntail,), nan, dtype=torch.float64, device=dev)
            gflat = torch.full_like(ctx.pflat, nan)
            _l.check(lib.cbfssm_gp_tail_f64(C.byref(lay), _ptr(ctx.buf), _ptr(red), _ptr(dense), lay.M if lay.rev_stash else 0,
                                            0.0, _ptr(ctx.pflat), _ptr(ctx.cflat), _ptr(twork), _ptr(gflat), _stream()),
                     'cbfssm_gp_tail_f64')
            gp = _gp_split(gflat, ctx.shapes, need[4:])
        return (None, None, gmean if need[2] else None, gcov if cov is not None and need[3] else None) + gp


def gp_moment_match_params(pack, mean, cov, *params, cross=True):
    """gp_moment_match's results with a grad_fn into `mean`, `cov` AND the five parameter tensors (_gp_args' order) when grad
    is enabled and one of them requires it: the pack is prepared from the parameters, the values are bitwise those of
    gp_moment_match_eval on that pack, info never carries a grad_fn.  Otherwise the pack is prepared and the evaluation call
    runs.  Conventions of gp_moment_match: the gradient for cov is that of the function of its lower triangle, a result the
    loss does not use goes down as a NULL cotangent (none used: nothing is launched), cov=None is allowed (the leaf
    gradients are then those of gp_predict for gmean = gfmean, gvar = diag gfcov), without a point nothing is prepared or
    launched and the leaf gradients are zeros.  Where info[n] != 0 the rows of point n of the gradients for mean and cov
    are NaN and so are all five leaf gradients, by select.  Once differentiable; float64; diagonal q(z); no host
    synchronisation."""
    dev = pack.buf.device
    mean = torch.as_tensor(mean, dtype=torch.float64, device=dev)
    assert mean.dim() == 2 and mean.shape[1] == pack.D, 'mean (npts, D)'
    if cov is not None:
        cov = torch.as_tensor(cov, dtype=torch.float64, device=dev)
        assert tuple(cov.shape) == (mean.shape[0], pack.D, pack.D), 'cov (npts, D, D)'
    params = _gp_args(pack, params)
    if not (torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in [mean, cov] + params)):
        if mean.shape[0]:
            pflat, cflat = _gp_flat(params)
            _gp_prepare(pack, params, cflat)
        return gp_moment_match_eval(pack, mean, cov, cross=cross)
    out = _GpMomentMatchParams.apply(pack, bool(cross), mean, cov, *params)
    if cross:
        return out
    return out[0], out[1], None, out[2]


# ---- the extended Kalman filter over the transition of one sparse GP: a Gaussian belief per chain through time -------------
#
#     means, covs, loglik = gp_ekf_eval(pack, m0, P0, a, y, var_x, var_y, cond=None)
#
#     for t in 0..T-1:
#         x = concat(m, a[t]);  f, fv = predict(x);  A = I + d fmean / d x [:, :Do]        (gp_tf.py:132-161 and its Jacobian)
#         m = m + f;  P = A P A^T + diag(fv + var_x)                                      (cbfssm.py:199-206)
#         where cond[t, n], for j in 0..Dy-1:  s = P[j, j] + var_y[j];  delta = y[t, n, j] - m[j];  g = P[:, j] / s
#                                              m += g delta;  P -= s g g^T;  loglik[n] -= (log(2 pi s) + delta^2 / s) / 2
#         means[t] = m;  covs[t] = P
#
# the scalar updates being the joint Kalman update with H = [I_Dy 0], R = diag(var_y) (cbfssm.py:245-251: the first dim_y
# state dimensions are observed).  One launch for all steps (cbfssm_gp_ekf_f64) instead of a loop over predict +
# transition_jacobians + batched tensor-library algebra with one prepare per step.

def gp_ekf_eval(pack, m0, P0, a, y, var_x, var_y, cond=None):
    """(means (T, N, Do), covs (T, N, Do, Do), loglik (N)) on a pack that is already prepared.  m0 (N, Do), P0 (N, Do, Do)
    or None (zero; only its lower triangle is read), a (T, N, D - Do) or None when the GP takes the state alone, y
    (T, N, Dy) with 1 <= Dy <= Do, var_x (Do) constrained values or None, var_y (Dy) constrained values, cond (T, N) of
    0 / 1 (any dtype; None: condition everywhere).  A y entry where cond = 0 is never used and may be NaN.  Evaluation
    only: no grad_fn, no host synchronisation, nothing is launched without a chain or a step (loglik is then zero)."""
    lib = _l.load()
    lay, dev = pack.layout, pack.buf.device
    Do, Da = pack.Do, pack.D - pack.Do
    if Da < 0:
        raise ValueError('gp_ekf: the GP input dimension %d is smaller than its output dimension %d' % (pack.D, pack.Do))
    f64 = lambda t: torch.as_tensor(t, dtype=torch.float64, device=dev).detach().contiguous()
    with torch.no_grad():
        y, m0, var_y = f64(y), f64(m0), f64(var_y)
        assert y.dim() == 3 and m0.dim() == 2 and m0.shape == (y.shape[1], Do), 'y (T, N, Dy), m0 (N, Do)'
        T, N, Dy = y.shape
        if not 1 <= Dy <= Do:
            raise ValueError('gp_ekf: y observes the first Dy state dimensions, 1 <= Dy <= %d (got %d)' % (Do, Dy))
        assert tuple(var_y.shape) == (Dy,), 'var_y (Dy)'
        if P0 is not None:
            P0 = f64(P0)
            assert tuple(P0.shape) == (N, Do, Do), 'P0 (N, Do, Do)'
        if Da == 0:
            assert a is None or tuple(a.shape) == (T, N, 0), 'a: None or (T, N, 0) when the GP takes the state alone'
            a = None
        else:
            a = f64(a)
            assert tuple(a.shape) == (T, N, Da), 'a (T, N, D - Do)'
        if var_x is not None:
            var_x = f64(var_x)
            assert tuple(var_x.shape) == (Do,), 'var_x (Do)'
        if cond is not None:
            cond = torch.as_tensor(cond, device=dev)
            assert tuple(cond.shape) == (T, N), 'cond (T, N)'
            cond = (cond != 0).to(torch.float64).contiguous()
        means = torch.empty(T, N, Do, dtype=torch.float64, device=dev)
        covs = torch.empty(T, N, Do, Do, dtype=torch.float64, device=dev)
        if N == 0 or T == 0:
            return means, covs, torch.zeros(N, dtype=torch.float64, device=dev)
        loglik = torch.empty(N, dtype=torch.float64, device=dev)
        nwork = int(lib.cbfssm_gp_ekf_work_elems(C.byref(lay)))
        if nwork < 1:
            raise _l.CbfssmHipError('cbfssm_gp_ekf_work_elems refused the layout')
        work = torch.empty(nwork, dtype=torch.float64, device=dev)
        _l.check(lib.cbfssm_gp_ekf_f64(C.byref(lay), _ptr(pack.buf), _ptr(m0), _ptr(P0), _ptr(a), _ptr(y), _ptr(cond),
                                       _ptr(var_x), _ptr(var_y), Dy, N, T, _ptr(means), _ptr(covs), _ptr(loglik), _ptr(work),
                                       _stream()), 'cbfssm_gp_ekf_f64')
    return means, covs, loglik


# ---- the Rauch-Tung-Striebel smoother behind that filter: every state given ALL observations of its chain ----------------
#
#     res = gp_eks_eval(pack, m0, P0, a, y, var_x, var_y, cond=None, lag_one=False)          (an EksResult)
#
#     forward: gp_ekf_eval as it is, which also leaves m-_t, P-_t (before conditioning) and A_t P_{t-1} of every step
#     (ms, Ps)[T-1] = (means, covs)[T-1]
#     for t in T-1..0:
#         G = (A_t P_{t-1})^T (P-_t)^-1                       (Cholesky factorisation of P-_t, two triangular solves)
#         ms[t-1] = m[t-1] + G (ms[t] - m-_t);  Ps[t-1] = P[t-1] + G (Ps[t] - P-_t) G^T;  lag_one[t] = G Ps[t]
#
# with (m, P)[-1] = (m0, P0): the last iteration gives the smoothed initial belief.  Four launches on one stream
# (cbfssm_gp_eks_f64) instead of ekf + one transition_jacobians per step + a loop of batched tensor-library solves.

EksResult = collections.namedtuple('EksResult', 'smeans scovs loglik means covs pmeans pcovs init_mean init_cov lag_one info')


def gp_eks_eval(pack, m0, P0, a, y, var_x, var_y, cond=None, lag_one=False):
    """EksResult(smeans (T, N, Do), scovs (T, N, Do, Do), loglik (N), means, covs (the filtered moments and loglik bitwise
    those of gp_ekf_eval), pmeans (T, N, Do), pcovs (T, N, Do, Do) (the one-step predictive moments, before conditioning),
    init_mean (N, Do), init_cov (N, Do, Do) (the smoothed belief before step 0), lag_one (T, N, Do, Do) with
    lag_one[t] = Cov(x_{t-1}, x_t | y) or None unless asked for, info (N) int64) on a pack that is already prepared;
    arguments as gp_ekf_eval.  info[n] = 0, or t + 1 where the factorisation of P-_t met a pivot <= 0 or not finite (P0 not
    positive semi-definite): that chain's smoothed results at times < t, its initial belief and lag_one[<= t] are NaN,
    everything else is unaffected.  Every scovs[t, n] and init_cov[n] is bitwise symmetric.  Evaluation only: no grad_fn,
    no host synchronisation, nothing is launched without a chain or a step (loglik is then zero)."""
    lib = _l.load()
    lay, dev = pack.layout, pack.buf.device
    Do, Da = pack.Do, pack.D - pack.Do
    if Da < 0:
        raise ValueError('gp_eks: the GP input dimension %d is smaller than its output dimension %d' % (pack.D, pack.Do))
    f64 = lambda t: torch.as_tensor(t, dtype=torch.float64, device=dev).detach().contiguous()
    with torch.no_grad():
        y, m0, var_y = f64(y), f64(m0), f64(var_y)
        assert y.dim() == 3 and m0.dim() == 2 and m0.shape == (y.shape[1], Do), 'y (T, N, Dy), m0 (N, Do)'
        T, N, Dy = y.shape
        if not 1 <= Dy <= Do:
            raise ValueError('gp_eks: y observes the first Dy state dimensions, 1 <= Dy <= %d (got %d)' % (Do, Dy))
        assert tuple(var_y.shape) == (Dy,), 'var_y (Dy)'
        if P0 is not None:
            P0 = f64(P0)
            assert tuple(P0.shape) == (N, Do, Do), 'P0 (N, Do, Do)'
        if Da == 0:
            assert a is None or tuple(a.shape) == (T, N, 0), 'a: None or (T, N, 0) when the GP takes the state alone'
            a = None
        else:
            a = f64(a)
            assert tuple(a.shape) == (T, N, Da), 'a (T, N, D - Do)'
        if var_x is not None:
            var_x = f64(var_x)
            assert tuple(var_x.shape) == (Do,), 'var_x (Do)'
        if cond is not None:
            cond = torch.as_tensor(cond, device=dev)
            assert tuple(cond.shape) == (T, N), 'cond (T, N)'
            cond = (cond != 0).to(torch.float64).contiguous()
        new = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
        means, covs, pmeans, pcovs, cross = new(T, N, Do), new(T, N, Do, Do), new(T, N, Do), new(T, N, Do, Do), new(T, N, Do, Do)
        smeans, scovs, sm_init, sP_init = new(T, N, Do), new(T, N, Do, Do), new(N, Do), new(N, Do, Do)
        lag1 = new(T, N, Do, Do) if lag_one else None
        if N == 0 or T == 0:
            return EksResult(smeans, scovs, torch.zeros(N, dtype=torch.float64, device=dev), means, covs, pmeans, pcovs, sm_init,
                             sP_init, lag1, torch.zeros(N, dtype=torch.int64, device=dev))
        loglik, info = new(N), new(N)
        nwork = int(lib.cbfssm_gp_eks_work_elems(C.byref(lay)))
        if nwork < 1:
            raise _l.CbfssmHipError('cbfssm_gp_eks_work_elems refused the layout')
        work = new(nwork)
        _l.check(lib.cbfssm_gp_eks_f64(C.byref(lay), _ptr(pack.buf), _ptr(m0), _ptr(P0), _ptr(a), _ptr(y), _ptr(cond),
                                       _ptr(var_x), _ptr(var_y), Dy, N, T, _ptr(means), _ptr(covs), _ptr(loglik), _ptr(pmeans),
                                       _ptr(pcovs), _ptr(cross), _ptr(smeans), _ptr(scovs), _ptr(sm_init), _ptr(sP_init),
                                       _ptr(lag1), _ptr(info), _ptr(work), _stream()), 'cbfssm_gp_eks_f64')
    return EksResult(smeans, scovs, loglik, means, covs, pmeans, pcovs, sm_init, sP_init, lag1, info.to(torch.int64))


# ---- the assumed-density (moment-matching) filter over the transition of one sparse GP, and the smoother behind it ---------
#
#     res = gp_adf_eval(pack, m0, P0, a, y, var_x, var_y, cond=None)                          (an AdfResult)
#     res = gp_ads_eval(pack, m0, P0, a, y, var_x, var_y, cond=None, lag_one=False)           (an EksResult)
#
#     for t in 0..T-1:
#         x = concat(m, a[t]);  S = blockdiag(P, 0)                                        (the auxiliary input is known)
#         fmean, fcov, xcov = moment_match(x, S);  Cx = xcov[:, :Do]                       (exact, gp_moment_match_eval)
#         m = m + fmean;  cross[t] = P + Cx;  P = P + Cx + Cx^T + fcov + diag(var_x);  pmeans[t], pcovs[t] = m, P
#         where cond[t, n], for j in 0..Dy-1:  s = P[j, j] + var_y[j];  delta = y[t, n, j] - m[j];  g = P[:, j] / s
#                                              m += g delta;  P -= s g g^T;  loglik[n] -= (log(2 pi s) + delta^2 / s) / 2
#         means[t] = m;  covs[t] = P
#
# gp_ekf_eval's recursion with the linearisation at the mean replaced by the exact moments of the GP under the belief: the
# two differ by tens of percent once the belief is as wide as a lengthscale.  One launch for all steps (cbfssm_gp_adf_f64),
# alpha and the W_d tiles formed once per call, instead of a loop of transition_moments (one prepare, two pre-kernels, one
# launch and about ten tensor-library ops per step) plus a dozen batched tensor-library ops for the update.  gp_ads_eval
# chains the gain and sweep launches of gp_eks_eval behind it (cbfssm_gp_ads_f64): with cross[t] = P + Cx = Cov(h_t, h_{t-1})
# the gain cross[t]^T (P-_t)^-1 is the ADF smoother gain.

AdfResult = collections.namedtuple('AdfResult', 'means covs loglik pmeans pcovs cross info')


def _adf_inputs(who, pack, m0, P0, a, y, var_x, var_y, cond):
    """the argument checks of gp_ekf_eval: (m0, P0, a, y, var_x, var_y, cond, T, N, Dy) as contiguous float64 or None"""
    dev = pack.buf.device
    Do, Da = pack.Do, pack.D - pack.Do
    if Da < 0:
        raise ValueError('%s: the GP input dimension %d is smaller than its output dimension %d' % (who, pack.D, pack.Do))
    f64 = lambda t: torch.as_tensor(t, dtype=torch.float64, device=dev).detach().contiguous()
    y, m0, var_y = f64(y), f64(m0), f64(var_y)
    assert y.dim() == 3 and m0.dim() == 2 and m0.shape == (y.shape[1], Do), 'y (T, N, Dy), m0 (N, Do)'
    T, N, Dy = y.shape
    if not 1 <= Dy <= Do:
        raise ValueError('%s: y observes the first Dy state dimensions, 1 <= Dy <= %d (got %d)' % (who, Do, Dy))
    assert tuple(var_y.shape) == (Dy,), 'var_y (Dy)'
    if P0 is not None:
        P0 = f64(P0)
        assert tuple(P0.shape) == (N, Do, Do), 'P0 (N, Do, Do)'
    if Da == 0:
        assert a is None or tuple(a.shape) == (T, N, 0), 'a: None or (T, N, 0) when the GP takes the state alone'
        a = None
    else:
        a = f64(a)
        assert tuple(a.shape) == (T, N, Da), 'a (T, N, D - Do)'
    if var_x is not None:
        var_x = f64(var_x)
        assert tuple(var_x.shape) == (Do,), 'var_x (Do)'
    if cond is not None:
        cond = torch.as_tensor(cond, device=dev)
        assert tuple(cond.shape) == (T, N), 'cond (T, N)'
        cond = (cond != 0).to(torch.float64).contiguous()
    return m0, P0, a, y, var_x, var_y, cond, T, N, Dy


def _adf_work(lib, lay, dev):
    nwork = int(lib.cbfssm_gp_adf_work_elems(C.byref(lay)))
    if nwork < 1:
        raise _l.CbfssmHipError('cbfssm_gp_adf_work_elems refused the layout')
    return torch.empty(nwork, dtype=torch.float64, device=dev)


def gp_adf_eval(pack, m0, P0, a, y, var_x, var_y, cond=None):
    """AdfResult(means (T, N, Do), covs (T, N, Do, Do), loglik (N), pmeans (T, N, Do), pcovs (T, N, Do, Do) (the one-step
    predictive moments, before conditioning), cross (T, N, Do, Do) with cross[t] = Cov(h_t, h_{t-1}), row = new state,
    info (N) int64) on a pack that is already prepared; arguments as gp_ekf_eval.  info[n] = 0, or t + 1 of the first step
    at which a factorisation of chain n met a pivot <= 0, not finite, or below the floor a positive semi-definite belief
    keeps it above (1 for I + S~, 1/2 for I/2 + S~) -- P0 not positive semi-definite: from that step on the chain's results and its loglik are NaN, no other chain is affected.  Every covs[t, n] and pcovs[t, n] is bitwise
    symmetric.  Evaluation only: no grad_fn, nothing is launched without a chain or a step (loglik and info are then zero);
    reading info as int64 is a device-side cast, not a host synchronisation."""
    lib = _l.load()
    lay, dev = pack.layout, pack.buf.device
    Do = pack.Do
    with torch.no_grad():
        m0, P0, a, y, var_x, var_y, cond, T, N, Dy = _adf_inputs('gp_adf', pack, m0, P0, a, y, var_x, var_y, cond)
        new = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
        means, covs, pmeans, pcovs, cross = new(T, N, Do), new(T, N, Do, Do), new(T, N, Do), new(T, N, Do, Do), new(T, N, Do, Do)
        if N == 0 or T == 0:
            return AdfResult(means, covs, torch.zeros(N, dtype=torch.float64, device=dev), pmeans, pcovs, cross,
                             torch.zeros(N, dtype=torch.int64, device=dev))
        loglik, info = new(N), new(N)
        work = _adf_work(lib, lay, dev)
        _l.check(lib.cbfssm_gp_adf_f64(C.byref(lay), _ptr(pack.buf), _ptr(m0), _ptr(P0), _ptr(a), _ptr(y), _ptr(cond),
                                       _ptr(var_x), _ptr(var_y), Dy, N, T, _ptr(means), _ptr(covs), _ptr(loglik), _ptr(pmeans),
                                       _ptr(pcovs), _ptr(cross), _ptr(info), _ptr(work), _stream()), 'cbfssm_gp_adf_f64')
    return AdfResult(means, covs, loglik, pmeans, pcovs, cross, info.to(torch.int64))


def gp_ads_eval(pack, m0, P0, a, y, var_x, var_y, cond=None, lag_one=False):
    """EksResult, fields as gp_eks_eval, of the Rauch-Tung-Striebel smoother behind gp_adf_eval: means, covs, loglik, pmeans
    and pcovs are gp_adf_eval's, bitwise.  info[n] is the forward pass's where that is non-zero -- the chain's smoothed
    results are then NaN throughout -- and otherwise the sweep's, as in gp_eks_eval.  Every scovs[t, n] and init_cov[n] is
    bitwise symmetric.  Evaluation only: no grad_fn, no host synchronisation, nothing is launched without a chain or a
    step (loglik and info are then zero)."""
    lib = _l.load()
    lay, dev = pack.layout, pack.buf.device
    Do = pack.Do
    with torch.no_grad():
        m0, P0, a, y, var_x, var_y, cond, T, N, Dy = _adf_inputs('gp_ads', pack, m0, P0, a, y, var_x, var_y, cond)
        new = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
        means, covs, pmeans, pcovs, cross = new(T, N, Do), new(T, N, Do, Do), new(T, N, Do), new(T, N, Do, Do), new(T, N, Do, Do)
        smeans, scovs, sm_init, sP_init = new(T, N, Do), new(T, N, Do, Do), new(N, Do), new(N, Do, Do)
        lag1 = new(T, N, Do, Do) if lag_one else None
        if N == 0 or T == 0:
            return EksResult(smeans, scovs, torch.zeros(N, dtype=torch.float64, device=dev), means, covs, pmeans, pcovs, sm_init,
                             sP_init, lag1, torch.zeros(N, dtype=torch.int64, device=dev))
        loglik, info = new(N), new(N)
        work = _adf_work(lib, lay, dev)
        _l.check(lib.cbfssm_gp_ads_f64(C.byref(lay), _ptr(pack.buf), _ptr(m0), _ptr(P0), _ptr(a), _ptr(y), _ptr(cond),
                                       _ptr(var_x), _ptr(var_y), Dy, N, T, _ptr(means), _ptr(covs), _ptr(loglik), _ptr(pmeans),
                                       _ptr(pcovs), _ptr(cross), _ptr(smeans), _ptr(scovs), _ptr(sm_init), _ptr(sP_init),
                                       _ptr(lag1), _ptr(info), _ptr(work), _stream()), 'cbfssm_gp_ads_f64')
    return EksResult(smeans, scovs, loglik, means, covs, pmeans, pcovs, sm_init, sP_init, lag1, info.to(torch.int64))


# The same filter with a grad_fn into the inputs of the call:
#
#     AdfResult = gp_adf(pack, m0, P0, a, y, var_x, var_y, cond=None)
#
# means, covs and loglik carry a grad_fn into m0, P0, a, y, var_x and var_y; pmeans, pcovs, cross and info do not.  The model
# is a constant, as in gp_moment_match: the context keeps a copy of the pack and no parameter tensor receives a gradient.  The
# forward is gp_adf_eval itself and saves nothing new (its records are its results); the backward is the two pre-kernels, ONE
# reverse-time launch and the fixed-order sum of the variance partials (cbfssm_gp_adf_bwd_f64).  Conventions: gp_ekf's (P0's
# lower triangle, None arguments, y and var_y under the mask, NULL cotangents).  Where info[n] != 0 the rows of chain n of the
# gradients for m0, P0, a and y are NaN and so are those for var_x and var_y; no other chain's rows are affected.

class _GpAdf(torch.autograd.Function):

    @staticmethod
    def forward(ctx, pack, cond, m0, P0, a, y, var_x, var_y):
        with torch.no_grad():
            m0d, P0d, ad, yd, vxd, vyd, cd, T, N, Dy = _adf_inputs('gp_adf', pack, m0, P0, a, y, var_x, var_y, cond)
        res = gp_adf_eval(pack, m0d, P0d, ad, yd, vxd, vyd, cond=cd)
        ctx.set_materialize_grads(False)                # an unused result reaches backward as None, and the entry point as NULL
        ctx.empty = (N == 0 or T == 0)
        ctx.layout, ctx.buf = pack.layout, (None if ctx.empty else pack.buf.clone())
        ctx.has = (P0d is not None, ad is not None, vxd is not None, cd is not None)
        ctx.dims = (T, N, Dy)
        ctx.save_for_backward(m0d, yd, vyd, res.means, res.covs, res.pmeans, res.pcovs, res.info.to(torch.float64),
                              *[t for t in (P0d, ad, vxd, cd) if t is not None])
        ctx.mark_non_differentiable(res.pmeans, res.pcovs, res.cross, res.info)
        return tuple(res)

    @staticmethod
    @once_differentiable
    def backward(ctx, gmeans, gcovs, gloglik, *rest):
        lib = _l.load()
        lay = ctx.layout
        need = ctx.needs_input_grad                     # 2 m0, 3 P0, 4 a, 5 y, 6 var_x, 7 var_y
        T, N, Dy = ctx.dims
        hasP, hasa, hasvx, hascond = ctx.has
        if gmeans is None and gcovs is None and gloglik is None:
            return (None,) * 8
        m0, y, var_y, means, covs, pmeans, pcovs, info = ctx.saved_tensors[:8]
        more = list(ctx.saved_tensors[8:])
        P0 = more.pop(0) if hasP else None
        a = more.pop(0) if hasa else None
        var_x = more.pop(0) if hasvx else None
        cond = more.pop(0) if hascond else None
        dev, Do = y.device, lay.Do
        # NaN-filled, not uninitialised, as in _GpMomentMatch.backward: the launch writes every entry of the gradients and
        # reads nothing of `work` that this call did not write, so every call is a poisoned-buffer run
        nan = 0.0 if ctx.empty else float('nan')        # (no chain or no step: nothing is launched, the gradients are zero)
        full = lambda *s: torch.full(s, nan, dtype=torch.float64, device=dev)
        gm0, gy, gvy = torch.full_like(m0, nan), torch.full_like(y, nan), full(Dy)
        gP0 = torch.full_like(P0, nan) if hasP else None
        ga = torch.full_like(a, nan) if hasa else None
        gvx = full(Do) if hasvx else None
        if not ctx.empty:
            con = lambda t: t.contiguous() if t is not None else None
            gmeans, gcovs, gloglik = con(gmeans), con(gcovs), con(gloglik)
            nwork = int(lib.cbfssm_gp_adf_bwd_work_elems(C.byref(lay), N))
            if nwork < 1:
                raise _l.CbfssmHipError('cbfssm_gp_adf_bwd_work_elems refused the layout')
            work = full(nwork)
            _l.check(lib.cbfssm_gp_adf_bwd_f64(C.byref(lay), _ptr(ctx.buf), _ptr(m0), _ptr(P0), _ptr(a), _ptr(y), _ptr(cond),
                                               _ptr(var_x), _ptr(var_y), Dy, _ptr(means), _ptr(covs), _ptr(pmeans),
                                               _ptr(pcovs), _ptr(info), _ptr(gmeans), _ptr(gcovs), _ptr(gloglik), N, T,
                                               _ptr(gm0), _ptr(gP0), _ptr(ga), _ptr(gy), _ptr(gvx), _ptr(gvy), _ptr(work),
                                               _stream()), 'cbfssm_gp_adf_bwd_f64')
        return (None, None, gm0 if need[2] else None, gP0 if need[3] else None, ga if need[4] else None,
                gy if need[5] else None, gvx if need[6] else None, gvy if need[7] else None)


def gp_adf(pack, m0, P0, a, y, var_x, var_y, cond=None):
    """gp_adf_eval's AdfResult on a prepared pack, with a grad_fn on means, covs and loglik into m0, P0, a, y, var_x and var_y
    when grad is enabled and one of them requires it (else the evaluation call itself).  The seven results are bitwise those
    of the evaluation call; pmeans, pcovs, cross and info never carry a grad_fn.  The model is a constant of the call: no
    parameter tensor is connected to these results.  The gradient conventions stand above _GpAdf.  Once differentiable;
    float64; no host synchronisation."""
    dev = pack.buf.device
    f64 = lambda t: torch.as_tensor(t, dtype=torch.float64, device=dev) if t is not None else None
    m0, P0, a, y, var_x, var_y = (f64(t) for t in (m0, P0, a, y, var_x, var_y))
    if not (torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (m0, P0, a, y, var_x, var_y))):
        return gp_adf_eval(pack, m0, P0, a, y, var_x, var_y, cond=cond)
    return AdfResult(*_GpAdf.apply(pack, cond, m0, P0, a, y, var_x, var_y))


# ---- the differentiable form of gp_ekf_eval: the marginal likelihood of a GP state-space model as a training objective ---
#
#     means, covs, loglik = gp_ekf(pack, m0, P0, a, y, var_x, var_y, zeta_pos, zeta_mean, zeta_var_unc, variance_unc,
#                                  lengthscales_unc, cond=None)
#
# Values: those of gp_ekf_eval on the prepared pack, bitwise (cbfssm_gp_ekf_save_f64, which also leaves m-, P-, A P and the
# Jacobian J of every step).  Backward: cbfssm_gp_ekf_bwd_f64 -> cbfssm_reduce_partials_f64 -> cbfssm_gp_tail_f64
# (kl_weight 0); gradients for m0, P0, a, y, var_x, var_y and the five parameter tensors, none for cond.  Conventions:
#   P0     only its lower triangle is read: the gradient is that of the function of tril(P0) + tril(P0, -1)^T, exactly zero
#          above the diagonal, a strictly lower entry carries both symmetric contributions
#   None   P0, var_x, a given as None have no gradient
#   y      exactly 0 where cond = 0 (by select: y may be NaN there); cond = 0 everywhere: zero gradients for y and var_y
#   all three outputs take cotangents; an unused output costs nothing; the covs cotangent need not be symmetric
# Once differentiable, float64, diagonal q(z), no host synchronisation, nothing launched without a chain or a step; the
# call keeps a copy of the prepared pack, as gp_predict does.

def _ekf_args(pack, m0, P0, a, y, var_x, var_y, cond):
    dev = pack.buf.device
    Do, Da = pack.Do, pack.D - pack.Do
    if Da < 0:
        raise ValueError('gp_ekf: the GP input dimension %d is smaller than its output dimension %d' % (pack.D, pack.Do))
    f64 = lambda t: torch.as_tensor(t, dtype=torch.float64, device=dev)
    y, m0, var_y = f64(y), f64(m0), f64(var_y)
    assert y.dim() == 3 and m0.dim() == 2 and m0.shape == (y.shape[1], Do), 'y (T, N, Dy), m0 (N, Do)'
    T, N, Dy = y.shape
    if not 1 <= Dy <= Do:
        raise ValueError('gp_ekf: y observes the first Dy state dimensions, 1 <= Dy <= %d (got %d)' % (Do, Dy))
    assert tuple(var_y.shape) == (Dy,), 'var_y (Dy)'
    if P0 is not None:
        P0 = f64(P0)
        assert tuple(P0.shape) == (N, Do, Do), 'P0 (N, Do, Do)'
    if Da == 0:
        assert a is None or tuple(a.shape) == (T, N, 0), 'a: None or (T, N, 0) when the GP takes the state alone'
        a = None
    else:
        a = f64(a)
        assert tuple(a.shape) == (T, N, Da), 'a (T, N, D - Do)'
    if var_x is not None:
        var_x = f64(var_x)
        assert tuple(var_x.shape) == (Do,), 'var_x (Do)'
    if cond is not None:
        cond = torch.as_tensor(cond, device=dev)
        assert tuple(cond.shape) == (T, N), 'cond (T, N)'
        cond = (cond != 0).to(torch.float64).contiguous()
    return m0, P0, a, y, var_x, var_y, cond


class _GpEkf(torch.autograd.Function):

    @staticmethod
    def forward(ctx, pack, cond, m0, P0, a, y, var_x, var_y, *params):
        lib = _l.load()
        pflat, cflat = _gp_flat(params)
        det = lambda t: t.detach().contiguous() if t is not None else None
        m0d, P0d, ad, yd, vxd, vyd = (det(t) for t in (m0, P0, a, y, var_x, var_y))
        T, N, Dy = yd.shape
        lay, dev, Do = pack.layout, yd.device, pack.Do
        new = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
        means, covs = new(T, N, Do), new(T, N, Do, Do)
        ctx.empty = (N == 0 or T == 0)
        ctx.set_materialize_grads(False)                # an unused output reaches backward as None, and the entry point as NULL
        ctx.layout, ctx.pflat, ctx.cflat = lay, pflat, cflat
        ctx.shapes = tuple(tuple(p.shape) for p in params)
        ctx.has = (P0d is not None, ad is not None, vxd is not None, cond is not None)
        ctx.dims = (T, N, Dy)
        if ctx.empty:                                   # (no chain or no step: nothing is prepared or launched)
            ctx.buf = None
            ctx.save_for_backward(m0d, yd, vyd)
            return means, covs, torch.zeros(N, dtype=torch.float64, device=dev)
        _gp_prepare(pack, params, cflat)
        buf = pack.buf.clone()
        loglik = new(N)
        pmeans, pcovs, cross, jac = new(T, N, Do), new(T, N, Do, Do), new(T, N, Do, Do), new(T, N, Do, Do)
        nwork = int(lib.cbfssm_gp_ekf_work_elems(C.byref(lay)))
        if nwork < 1:
            raise _l.CbfssmHipError('cbfssm_gp_ekf_work_elems refused the layout')
        work = new(nwork)
        _l.check(lib.cbfssm_gp_ekf_save_f64(C.byref(lay), _ptr(buf), _ptr(m0d), _ptr(P0d), _ptr(ad), _ptr(yd), _ptr(cond),
                                            _ptr(vxd), _ptr(vyd), Dy, N, T, _ptr(means), _ptr(covs), _ptr(loglik),
                                            _ptr(pmeans), _ptr(pcovs), _ptr(cross), _ptr(jac), _ptr(work), _stream()),
                 'cbfssm_gp_ekf_save_f64')
        ctx.buf = buf
        ctx.save_for_backward(m0d, yd, vyd, means, covs, pmeans, pcovs, cross, jac,
                              *[t for t in (P0d, ad, vxd, cond) if t is not None])           # (means, covs are outputs)
        return means, covs, loglik

    @staticmethod
    @once_differentiable
    def backward(ctx, gmeans, gcovs, gloglik):
        lib = _l.load()
        lay, buf = ctx.layout, ctx.buf
        need = ctx.needs_input_grad                     # 2 m0, 3 P0, 4 a, 5 y, 6 var_x, 7 var_y, 8.. the leaves
        T, N, Dy = ctx.dims
        m0, y, var_y = ctx.saved_tensors[:3]
        dev, Do = y.device, lay.Do
        hasP, hasa, hasvx, hascond = ctx.has
        if ctx.empty:
            z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)
            gp = _gp_split(torch.zeros_like(ctx.pflat), ctx.shapes, need[8:])
            return (None, None, z(N, Do) if need[2] else None, z(N, Do, Do) if need[3] and hasP else None,
                    z(T, N, lay.D - Do) if need[4] and hasa else None, z(T, N, Dy) if need[5] else None,
                    z(Do) if need[6] and hasvx else None, z(Dy) if need[7] else None) + gp
        means, covs, pmeans, pcovs, cross, jac = ctx.saved_tensors[3:9]
        rest = list(ctx.saved_tensors[9:])
        P0 = rest.pop(0) if hasP else None
        a = rest.pop(0) if hasa else None
        var_x = rest.pop(0) if hasvx else None
        cond = rest.pop(0) if hascond else None
        con = lambda t: t.contiguous() if t is not None else None
        gmeans, gcovs, gloglik = con(gmeans), con(gcovs), con(gloglik)
        gm0, gy = torch.empty_like(m0), torch.empty_like(y)
        gP0 = torch.empty(N, Do, Do, dtype=torch.float64, device=dev) if need[3] and hasP else None
        ga = torch.empty_like(a) if hasa else None
        nwg = int(lib.cbfssm_gp_ekf_bwd_workgroups(C.byref(lay), N))
        nwork = int(lib.cbfssm_gp_ekf_bwd_work_elems(C.byref(lay), N, T))
        if nwg < 1 or nwork < 1:
            raise _l.CbfssmHipError('cbfssm_gp_ekf_bwd_workgroups / _work_elems refused the layout')
        gpart = torch.empty((nwg + 32) * lay.rev_slab, dtype=torch.float64, device=dev)     # (+ CBFSSM_REDUCE_SPLIT)
        work = torch.empty(nwork, dtype=torch.float64, device=dev)
        image = torch.empty(lay.NBLK * lay.NBLK * 256, dtype=torch.float64, device=dev) if lay.rev_stash else None
        _l.check(lib.cbfssm_gp_ekf_bwd_f64(C.byref(lay), _ptr(buf), _ptr(m0), _ptr(P0), _ptr(a), _ptr(y), _ptr(cond),
                                           _ptr(var_x), _ptr(var_y), Dy, _ptr(means), _ptr(covs), _ptr(pmeans), _ptr(pcovs),
                                           _ptr(cross), _ptr(jac), _ptr(gmeans), _ptr(gcovs), _ptr(gloglik), N, T, _ptr(gm0),
                                           _ptr(gP0), _ptr(ga), _ptr(gy), _ptr(gpart), _ptr(work), _ptr(image), _stream()),
                 'cbfssm_gp_ekf_bwd_f64')
        gvx = gvy = None
        gp = (None,) * 5
        if need[6] or need[7] or any(need[8:]):
            red = torch.empty(lay.rev_slab, dtype=torch.float64, device=dev)
            _l.check(lib.cbfssm_reduce_partials_f64(_ptr(gpart), lay.rev_slab, nwg, _ptr(red), _stream()),
                     'cbfssm_reduce_partials_f64')
            small = lay.rev_slab - 192                  # the slab's scalars: [0, 16) d/d var_x, [16, 32) d/d var_y by state dim
            gvx = red[small:small + Do].clone()
            gvy = red[small + 16:small + 16 + Dy].clone()
            if any(need[8:]):
                gp = _gp_split(_gp_tail(lay, buf, red, image, 0.0, ctx.pflat, ctx.cflat), ctx.shapes, need[8:])
        return (None, None, gm0 if need[2] else None, gP0, ga if need[4] and hasa else None, gy if need[5] else None,
                gvx if need[6] and hasvx else None, gvy if need[7] else None) + gp


def gp_ekf(pack, m0, P0, a, y, var_x, var_y, *params, cond=None):
    """(means (T, N, Do), covs (T, N, Do, Do), loglik (N)): the values of gp_ekf_eval, bitwise, with a grad_fn into m0, P0,
    a, y, var_x, var_y and the five parameter tensors when grad is enabled and one of them requires it; otherwise the pack
    is prepared from the parameters and gp_ekf_eval runs: no records, no copy of the pack.  Arguments as gp_ekf_eval; the
    gradient conventions (P0's lower triangle, None arguments, y and var_y under the mask, cotangents) stand above this
    function."""
    m0, P0, a, y, var_x, var_y, cond = _ekf_args(pack, m0, P0, a, y, var_x, var_y, cond)
    params = _gp_args(pack, params)
    if not (torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in [m0, P0, a, y, var_x, var_y] + params)):
        if y.shape[0] * y.shape[1]:                     # (nothing is prepared or launched without a chain or a step)
            pflat, cflat = _gp_flat(params)
            _gp_prepare(pack, params, cflat)
        return gp_ekf_eval(pack, m0, P0, a, y, var_x, var_y, cond=cond)
    return _GpEkf.apply(pack, cond, m0, P0, a, y, var_x, var_y, *params)


# ---- the filter loop of one sparse GP: the rollout with a Gaussian filter update per step and chain behind a mask --------
#
#     traj, kl = gp_filter(pack, h0, a, ytilde, eps, var_x, var_y, zeta_pos, zeta_mean, zeta_var_unc, variance_unc,
#                          lengthscales_unc, cond=None, k_factor=1.0, reverse=False)
#
# the conditioned forward step of CBF-SSM (cbfssm/model/cbfssm.py:185-237) from per-chain data:
#
#     for t in 0..T-1 (reverse: T-1..0):
#         fmean, fvar = predict(concat(h, a[t]));  m = h + fmean;  v = fvar + var_x
#         cond[t, n]:  r = var_y + (k_factor - 1) v;  k = v / (r + v);  mu = m + k (ytilde[t] - m);  sig = (1 - k)^2 v + k^2 r
#                      h = mu + eps[t] sqrt(sig);  kl += 0.5 (log v - log sig + (sig + (mu - m)^2) / v - 1)
#         otherwise:   h = m + eps[t] sqrt(v)
#         traj[t] = h
#
# h0 (N, Do), a (T, N, Da) (None or (T, N, 0) when Da = 0), ytilde (T, N, Do), eps (T, N) standard normals, var_x (Do)
# CONSTRAINED values or None, var_y (Do) CONSTRAINED values, cond (T, N) of 0 / 1 (any dtype; None: condition everywhere).
# A ytilde entry where cond = 0 is never used and may be NaN; its gradient is exactly 0.  Forward: cbfssm_gp_filter_f64,
# the KL partials summed in a fixed order by cbfssm_reduce_partials_f64.  Backward: cbfssm_gp_filter_bwd_f64 ->
# cbfssm_reduce_partials_f64 -> cbfssm_gp_tail_f64 (kl_weight 0); gradients for h0, a, ytilde, var_x, var_y and the five
# parameter tensors, none for eps, cond, k_factor.  Once differentiable, no host synchronisation; the call keeps a copy of
# the prepared pack, as gp_predict does.

def _filter_forward(lay, buf, h0, a, ytilde, cond, eps, var_x, var_y, k_factor, reverse, save):
    """(traj, msave or None, vsave or None, kl) of one forward launch on prepared pack operands"""
    lib = _l.load()
    T, N = eps.shape
    Do, dev = lay.Do, eps.device
    traj = torch.empty(T, N, Do, dtype=torch.float64, device=dev)
    msave = torch.empty_like(traj) if save else None
    vsave = torch.empty_like(traj) if save else None
    if N == 0 or T == 0:
        return traj, msave, vsave, torch.zeros((), dtype=torch.float64, device=dev)
    npart = int(lib.cbfssm_gp_filter_partials(C.byref(lay), N))
    if npart < 1:
        raise _l.CbfssmHipError('cbfssm_gp_filter_partials refused the layout')
    kl_part = torch.empty(npart + 32, dtype=torch.float64, device=dev)                      # (+ CBFSSM_REDUCE_SPLIT)
    _l.check(lib.cbfssm_gp_filter_f64(C.byref(lay), _ptr(buf), _ptr(h0), _ptr(a), _ptr(ytilde), _ptr(cond), _ptr(eps),
                                      _ptr(var_x), _ptr(var_y), float(k_factor), N, T, int(bool(reverse)), _ptr(traj),
                                      _ptr(msave), _ptr(vsave), _ptr(kl_part), _stream()), 'cbfssm_gp_filter_f64')
    kl = torch.empty(1, dtype=torch.float64, device=dev)
    _l.check(lib.cbfssm_reduce_partials_f64(_ptr(kl_part), 1, npart, _ptr(kl), _stream()), 'cbfssm_reduce_partials_f64')
    return traj, msave, vsave, kl.reshape(())


def _filter_args(pack, h0, a, ytilde, eps, var_x, var_y, cond):
    h0, a, eps, var_x = _rollout_args(pack, h0, a, eps, var_x)
    dev = pack.buf.device
    T, N = eps.shape
    ytilde = torch.as_tensor(ytilde, dtype=torch.float64, device=dev)
    var_y = torch.as_tensor(var_y, dtype=torch.float64, device=dev)
    assert tuple(ytilde.shape) == (T, N, pack.Do) and tuple(var_y.shape) == (pack.Do,), 'ytilde (T, N, Do), var_y (Do)'
    if cond is not None:
        cond = torch.as_tensor(cond, device=dev)
        assert tuple(cond.shape) == (T, N), 'cond (T, N)'
        cond = (cond != 0).to(torch.float64).contiguous()
    return h0, a, ytilde, eps, var_x, var_y, cond


class _GpFilter(torch.autograd.Function):

    @staticmethod
    def forward(ctx, pack, reverse, k_factor, cond, eps, h0, a, ytilde, var_x, var_y, *params):
        pflat, cflat = _gp_flat(params)
        h0d, epsd, ytd, vyd = (t.detach().contiguous() for t in (h0, eps, ytilde, var_y))
        ad = a.detach().contiguous() if a is not None else None
        vxd = var_x.detach().contiguous() if var_x is not None else None
        buf = None
        if eps.numel():                                 # (no chain or no step: nothing is prepared or launched)
            _gp_prepare(pack, params, cflat)
            buf = pack.buf.clone()
        traj, msave, vsave, kl = _filter_forward(pack.layout, buf, h0d, ad, ytd, cond, epsd, vxd, vyd, k_factor, reverse, True)
        ctx.layout, ctx.buf, ctx.reverse, ctx.k_factor = pack.layout, buf, bool(reverse), float(k_factor)
        ctx.has_a, ctx.has_cond = ad is not None, cond is not None
        ctx.save_for_backward(h0d, epsd, ytd, vyd, traj, msave, vsave, *([ad] if ad is not None else []),
                              *([cond] if cond is not None else []))                         # (traj is an output)
        ctx.pflat, ctx.cflat = pflat, cflat
        ctx.shapes = tuple(tuple(p.shape) for p in params)
        return traj, kl

    @staticmethod
    @once_differentiable
    def backward(ctx, gtraj, gkl):
        lib = _l.load()
        lay, buf = ctx.layout, ctx.buf
        h0, eps, ytilde, var_y, traj, msave, vsave = ctx.saved_tensors[:7]
        rest = list(ctx.saved_tensors[7:])
        a = rest.pop(0) if ctx.has_a else None
        cond = rest.pop(0) if ctx.has_cond else None
        need = ctx.needs_input_grad                     # 5 h0, 6 a, 7 ytilde, 8 var_x, 9 var_y, 10.. the leaves
        T, N = eps.shape
        dev = eps.device
        gh0, gyt = torch.empty_like(h0), torch.empty_like(ytilde)
        ga = torch.empty_like(a) if a is not None else None
        gvx = gvy = None
        gp = (None,) * 5
        if N == 0 or T == 0:
            gh0 = gtraj.new_zeros(h0.shape)
            gvx, gvy = torch.zeros_like(var_y), torch.zeros_like(var_y)
            gp = _gp_split(torch.zeros_like(ctx.pflat), ctx.shapes, need[10:])
        else:
            gtraj = gtraj.contiguous()
            gkl = gkl.reshape(1).contiguous()
            nwg = int(lib.cbfssm_gp_filter_bwd_workgroups(C.byref(lay), N))
            nwork = int(lib.cbfssm_gp_filter_bwd_work_elems(C.byref(lay), N, T))
            if nwg < 1 or nwork < 0:
                raise _l.CbfssmHipError('cbfssm_gp_filter_bwd_workgroups / _work_elems refused the layout')
            gpart = torch.empty((nwg + 32) * lay.rev_slab, dtype=torch.float64, device=dev)     # (+ CBFSSM_REDUCE_SPLIT)
            work = torch.empty(nwork, dtype=torch.float64, device=dev) if nwork else None
            image = torch.empty(lay.NBLK * lay.NBLK * 256, dtype=torch.float64, device=dev) if lay.rev_stash else None
            _l.check(lib.cbfssm_gp_filter_bwd_f64(C.byref(lay), _ptr(buf), _ptr(h0), _ptr(a), _ptr(ytilde), _ptr(cond), _ptr(eps),
                                                  _ptr(var_y), ctx.k_factor, _ptr(traj), _ptr(msave), _ptr(vsave), _ptr(gtraj),
                                                  _ptr(gkl), N, T, int(ctx.reverse), _ptr(gh0), _ptr(ga), _ptr(gyt), _ptr(gpart),
                                                  _ptr(work), _ptr(image), _stream()), 'cbfssm_gp_filter_bwd_f64')
            if need[8] or need[9] or any(need[10:]):
                red = torch.empty(lay.rev_slab, dtype=torch.float64, device=dev)
                _l.check(lib.cbfssm_reduce_partials_f64(_ptr(gpart), lay.rev_slab, nwg, _ptr(red), _stream()),
                         'cbfssm_reduce_partials_f64')
                small = lay.rev_slab - 192              # the slab's scalars: [0, 16) d/d var_x, [16, 32) d/d var_y by state dim
                gvx = red[small:small + lay.Do].clone()
                gvy = red[small + 16:small + 16 + lay.Do].clone()
                if any(need[10:]):
                    gp = _gp_split(_gp_tail(lay, buf, red, image, 0.0, ctx.pflat, ctx.cflat), ctx.shapes, need[10:])
        return (None, None, None, None, None, gh0 if need[5] else None, ga if need[6] else None, gyt if need[7] else None,
                gvx if need[8] else None, gvy if need[9] else None) + gp


def gp_filter(pack, h0, a, ytilde, eps, var_x, var_y, *params, cond=None, k_factor=1.0, reverse=False):
    """(traj (T, N, Do), kl ()) of the loop above with a grad_fn into h0, a, ytilde, var_x, var_y and the five parameter
    tensors."""
    h0, a, ytilde, eps, var_x, var_y, cond = _filter_args(pack, h0, a, ytilde, eps, var_x, var_y, cond)
    return _GpFilter.apply(pack, bool(reverse), float(k_factor), cond, eps.detach(), h0, a, ytilde, var_x, var_y,
                           *_gp_args(pack, params))


def gp_filter_eval(pack, h0, a, ytilde, eps, var_x, var_y, cond=None, k_factor=1.0, reverse=False):
    """The forward launch alone on a pack that is already prepared: no saved rows, no grad_fn."""
    h0, a, ytilde, eps, var_x, var_y, cond = _filter_args(pack, h0, a, ytilde, eps, var_x, var_y, cond)
    with torch.no_grad():
        traj, _, _, kl = _filter_forward(pack.layout, pack.buf, h0.contiguous(), a.contiguous() if a is not None else None,
                                         ytilde.contiguous(), cond, eps.contiguous(),
                                         var_x.contiguous() if var_x is not None else None, var_y.contiguous(), k_factor,
                                         reverse, False)
    return traj, kl


# ---- Voliro's forward filter run: rigid-body step, Gaussian filter update, one sample and a KL term per step -------------
#
#     traj, kl = rigid_filter(body, x0, u, y, eps, var_x, var_y)
#
# body: a cbfssm.hip.lib.RigidBody (lib.rigid_body(mass_inv, inertia_inv, gravity, dt): host constants); x0 (N, 13),
# u (S, N, 6), y (S, N, 13), eps (S, N) standard normals, var_x / var_y (13) CONSTRAINED values; traj (S, N, 13) time-major,
# kl a 0-d tensor: the loop of cbfssm/model/voliro.py:188-242,314-338 (state: pos 0:3, quaternion 3:7 scalar first,
# linvel 7:10, angvel 10:13).  Forward: cbfssm_rigid_filter_f64, the KL partials summed in a fixed order by
# cbfssm_reduce_partials_f64.  Backward: cbfssm_rigid_filter_bwd_f64 (recomputes every step from the trajectory) ->
# cbfssm_reduce_partials_f64; gradients for x0, u, y, var_x, var_y, none for eps.  Once differentiable, no host
# synchronisation.  There is no tensor-library form of this loop in the package.

def _rigid_forward(body, x0, u, y, eps, var_x, var_y):
    lib = _l.load()
    S, N = eps.shape
    dev = x0.device
    if S < 1:
        raise ValueError('rigid_filter: at least one time step')
    traj = torch.empty(S, N, 13, dtype=torch.float64, device=dev)
    if N == 0:
        return traj, torch.zeros((), dtype=torch.float64, device=dev)
    npart = int(lib.cbfssm_rigid_filter_partials(N))
    if npart < 1:
        raise _l.CbfssmHipError('cbfssm_rigid_filter_partials refused N = %d' % N)
    kl_part = torch.empty(npart + 32, dtype=torch.float64, device=dev)                      # (+ CBFSSM_REDUCE_SPLIT)
    _l.check(lib.cbfssm_rigid_filter_f64(C.byref(body), _ptr(x0), _ptr(u), _ptr(y), _ptr(eps), _ptr(var_x), _ptr(var_y), N, S,
                                         _ptr(traj), _ptr(kl_part), _stream()), 'cbfssm_rigid_filter_f64')
    kl = torch.empty(1, dtype=torch.float64, device=dev)
    _l.check(lib.cbfssm_reduce_partials_f64(_ptr(kl_part), 1, npart, _ptr(kl), _stream()), 'cbfssm_reduce_partials_f64')
    return traj, kl.reshape(())


def _rigid_args(body, x0, u, y, eps, var_x, var_y):
    if not isinstance(body, _l.RigidBody):
        raise TypeError('rigid_filter: body must be a cbfssm.hip.lib.RigidBody (lib.rigid_body(...))')
    if not (torch.is_tensor(x0) and x0.is_cuda):
        raise ValueError('rigid_filter: x0 must be a device tensor')
    dev = x0.device
    x0, u, y, eps, var_x, var_y = (torch.as_tensor(t, dtype=torch.float64, device=dev) for t in (x0, u, y, eps, var_x, var_y))
    assert eps.dim() == 2, 'eps (S, N)'
    S, N = eps.shape
    assert tuple(x0.shape) == (N, 13) and tuple(u.shape) == (S, N, 6) and tuple(y.shape) == (S, N, 13), \
        'x0 (N, 13), u (S, N, 6), y (S, N, 13)'
    assert tuple(var_x.shape) == (13,) and tuple(var_y.shape) == (13,), 'var_x, var_y (13)'
    return x0, u, y, eps, var_x, var_y


class _RigidFilter(torch.autograd.Function):

    @staticmethod
    def forward(ctx, body, x0, u, y, eps, var_x, var_y):
        saved = tuple(t.detach().contiguous() for t in (x0, u, y, eps, var_x, var_y))
        traj, kl = _rigid_forward(body, *saved)
        ctx.body = body
        ctx.save_for_backward(*saved, traj)                                                  # (traj is an output)
        return traj, kl

    @staticmethod
    @once_differentiable
    def backward(ctx, gtraj, gkl):
        lib = _l.load()
        x0, u, y, eps, var_x, var_y, traj = ctx.saved_tensors
        need = ctx.needs_input_grad
        S, N = eps.shape
        dev = eps.device
        gx0, gu, gy = torch.empty_like(x0), torch.empty_like(u), torch.empty_like(y)
        gvx = gvy = None
        if N == 0:
            if need[5] or need[6]:
                gvx, gvy = torch.zeros_like(var_x), torch.zeros_like(var_y)
        else:
            gtraj = gtraj.contiguous()
            gkl = gkl.reshape(1).contiguous()
            nwg = int(lib.cbfssm_rigid_filter_partials(N))
            gpart = torch.empty((nwg + 32) * 32, dtype=torch.float64, device=dev)          # (+ CBFSSM_REDUCE_SPLIT)
            _l.check(lib.cbfssm_rigid_filter_bwd_f64(C.byref(ctx.body), _ptr(x0), _ptr(u), _ptr(y), _ptr(eps), _ptr(var_x),
                                                     _ptr(var_y), _ptr(traj), _ptr(gtraj), _ptr(gkl), N, S, _ptr(gx0),
                                                     _ptr(gu), _ptr(gy), _ptr(gpart), _stream()), 'cbfssm_rigid_filter_bwd_f64')
            if need[5] or need[6]:
                red = torch.empty(32, dtype=torch.float64, device=dev)
                _l.check(lib.cbfssm_reduce_partials_f64(_ptr(gpart), 32, nwg, _ptr(red), _stream()), 'cbfssm_reduce_partials_f64')
                gvx, gvy = red[0:13].clone(), red[13:26].clone()
        return (None, gx0 if need[1] else None, gu if need[2] else None, gy if need[3] else None, None,
                gvx if need[5] else None, gvy if need[6] else None)


def rigid_filter(body, x0, u, y, eps, var_x, var_y):
    """(traj (S, N, 13), kl ()) of the loop above with a grad_fn into x0, u, y, var_x and var_y."""
    x0, u, y, eps, var_x, var_y = _rigid_args(body, x0, u, y, eps, var_x, var_y)
    return _RigidFilter.apply(body, x0, u, y, eps.detach(), var_x, var_y)


def rigid_filter_eval(body, x0, u, y, eps, var_x, var_y):
    """The forward launch alone: no grad_fn, nothing kept."""
    args = _rigid_args(body, x0, u, y, eps, var_x, var_y)
    with torch.no_grad():
        return _rigid_forward(body, *(t.contiguous() for t in args))
