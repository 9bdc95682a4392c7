"""The fused GP filter loop on the GPU: cbfssm_gp_filter_f64 and cbfssm_gp_filter_bwd_f64 -> cbfssm_reduce_partials_f64 ->
cbfssm_gp_tail_f64 through the C ABI, and cbfssm.model.gp_tf.GPModel.filter / cbfssm.hip.autograd.gp_filter, against
reverse-mode autodiff of the recurrence over the CPU oracle (tests/gp_filter_cases.py, which states the rules: gradients
within 1e-6 of their tensor's largest entry, trajectories within 1e-8 of max |traj|, kl 1e-9 relative), against
gp_rollout where nothing conditions, against the product's own forward pass, and against a loop over gp_predict."""
import ctypes as C

import numpy as np
import pytest
import torch

import gp_filter_cases as fc
from gp_filter_cases import CASES, PARAMS, within_rule, traj_rule, kl_rule

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')


def _dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64, device=DEV)


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float64, device=DEV)


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


def _check_grads(got, ref, case):
    """the gradient rule on every tensor it applies to (a tensor without entries has nothing to check); exact zeros where
    the case conditions nowhere"""
    names, zeros = fc.grad_names(case)
    for k in names:
        g = np.asarray(got[k])
        r = ref['g_' + k].reshape(g.shape)
        if r.size:
            within_rule(k, g, r)
    for k in zeros:
        assert not np.any(np.asarray(got[k])), k + ' must be exactly 0'


def _abi(case, form='dense', backward=True):
    """forward and adjoint through the C ABI on NaN-prefilled outputs; returns a dict of host arrays"""
    from cbfssm.hip import lib as _l, ops
    from cbfssm.hip.ops import _ptr, _stream
    M, D, Do, N, T, reverse, with_vx, k_factor, mask = case
    Da = D - Do
    lib = _l.load()
    p, h0, a, ytilde, cond, eps, var_x, var_y, W = fc.make_inputs(*case)
    pack = ops.GPPack(M, D, Do, torch.device(DEV), form_mode=form)
    pt = {k: _dev(p[k]) for k in PARAMS}
    con = {k: (ops.tf_forward(pt[k]) if k.endswith('_unc') else pt[k]) for k in PARAMS}
    pack.prepare(con['zeta_pos'], con['lengthscales_unc'], con['variance_unc'], con['zeta_mean'], con['zeta_var_unc'])
    lay = pack.layout
    h0d, epsd, ytd, vyd = _dev(h0), _dev(eps), _dev(ytilde), _dev(var_y)
    ad = _dev(a) if Da else None
    vxd = _dev(var_x) if with_vx else None
    cd = _dev(cond) if cond is not None else None
    groups = (N + 15) // 16
    assert lib.cbfssm_gp_filter_partials(C.byref(lay), N) == groups
    traj, msave, vsave, kl_part = _nan(T, N, Do), _nan(T, N, Do), _nan(T, N, Do), _nan(groups + 32)
    _l.check(lib.cbfssm_gp_filter_f64(C.byref(lay), _ptr(pack.buf), _ptr(h0d), _ptr(ad), _ptr(ytd), _ptr(cd), _ptr(epsd),
                                      _ptr(vxd), _ptr(vyd), float(k_factor), N, T, int(reverse), _ptr(traj), _ptr(msave),
                                      _ptr(vsave), _ptr(kl_part), _stream()), 'cbfssm_gp_filter_f64')
    kl = _nan(1)
    _l.check(lib.cbfssm_reduce_partials_f64(_ptr(kl_part), 1, groups, _ptr(kl), _stream()), 'reduce')
    out = {'traj': traj.cpu().numpy(), 'msave': msave.cpu().numpy(), 'vsave': vsave.cpu().numpy(), 'kl': float(kl[0])}
    if not backward:
        return out
    nwg = lib.cbfssm_gp_filter_bwd_workgroups(C.byref(lay), N)
    nwork = lib.cbfssm_gp_filter_bwd_work_elems(C.byref(lay), N, T)
    assert nwg == groups and (nwork > 0) == bool(lay.rev_stash)
    gpart = _nan((nwg + 32) * lay.rev_slab)
    work = _nan(nwork) if nwork else None
    image = _nan(lay.NBLK * lay.NBLK * 256) if lay.rev_stash else None
    gh0, gyt = _nan(N, Do), _nan(T, N, Do)
    ga = _nan(T, N, Da) if Da else None
    gtraj, gkl = _dev(W), _dev([fc.KL_WEIGHT])
    _l.check(lib.cbfssm_gp_filter_bwd_f64(C.byref(lay), _ptr(pack.buf), _ptr(h0d), _ptr(ad), _ptr(ytd), _ptr(cd), _ptr(epsd),
                                          _ptr(vyd), float(k_factor), _ptr(traj), _ptr(msave), _ptr(vsave), _ptr(gtraj),
                                          _ptr(gkl), N, T, int(reverse), _ptr(gh0), _ptr(ga), _ptr(gyt), _ptr(gpart),
                                          _ptr(work), _ptr(image), _stream()), 'cbfssm_gp_filter_bwd_f64')
    red = _nan(lay.rev_slab)
    _l.check(lib.cbfssm_reduce_partials_f64(_ptr(gpart), lay.rev_slab, nwg, _ptr(red), _stream()), 'reduce')
    pflat = torch.cat([pt[k].reshape(-1) for k in PARAMS]).contiguous()
    cflat = torch.cat([con[k].reshape(-1) for k in PARAMS]).contiguous()
    work_t = torch.empty(int(lib.cbfssm_train_tail_half_work_elems(C.byref(lay))), dtype=torch.float64, device=DEV)
    gflat = torch.full_like(pflat, NAN)
    _l.check(lib.cbfssm_gp_tail_f64(C.byref(lay), _ptr(pack.buf), _ptr(red), _ptr(image), 0, 0.0, _ptr(pflat), _ptr(cflat),
                                    _ptr(work_t), _ptr(gflat), _stream()), 'cbfssm_gp_tail_f64')
    o = 0
    for k in PARAMS:
        n = pt[k].numel()
        out[k] = gflat[o:o + n].reshape(pt[k].shape).cpu().numpy()
        o += n
    small = lay.rev_slab - 192
    out['h0'] = gh0.cpu().numpy()
    out['a'] = ga.cpu().numpy() if Da else np.zeros((T, N, 0))
    out['ytilde'] = gyt.cpu().numpy()
    out['var_x'] = red[small:small + Do].cpu().numpy()
    out['var_y'] = red[small + 16:small + 16 + Do].cpu().numpy()
    out['gflat'] = gflat.cpu().numpy()
    return out


@pytest.mark.parametrize('case', CASES, ids=str)
def test_c_abi_against_the_reference(case):
    ref = fc.reference(case)
    o1, o2 = _abi(case), _abi(case)
    traj_rule('traj', o1['traj'], ref['traj'])
    kl_rule(o1['kl'], ref['kl'])
    assert np.all(np.isfinite(o1['msave'])) and np.all(np.isfinite(o1['vsave'])) and np.all(o1['vsave'] > 0)
    _check_grads(o1, ref, case)
    p, h0, a, ytilde, cond, eps, var_x, var_y, W = fc.make_inputs(*case)
    assert np.all(np.isfinite(o1['ytilde']))
    if cond is not None:
        assert not np.any(o1['ytilde'][cond == 0.0]), 'gytilde must be exactly 0 where cond = 0'
    for k in ('traj', 'msave', 'vsave', 'h0', 'a', 'ytilde', 'var_x', 'var_y', 'gflat'):
        assert np.all(np.isfinite(o1[k])), k
        assert np.array_equal(o1[k], o2[k]), 'two calls differ: ' + k
    assert o1['kl'] == o2['kl']


def _leaves(case):
    M, D, Do, N, T, reverse, with_vx, k_factor, mask = case
    p, h0, a, ytilde, cond, eps, var_x, var_y, W = fc.make_inputs(*case)
    lv = {'h0': _dev(h0).requires_grad_(), 'ytilde': _dev(ytilde).requires_grad_(), 'var_y': _dev(var_y).requires_grad_()}
    if D > Do:
        lv['a'] = _dev(a).requires_grad_()
    if with_vx:
        lv['var_x'] = _dev(var_x).requires_grad_()
    return p, lv, (_dev(cond) if cond is not None else None), _dev(eps), _dev(W)


def _collect(lv, leaves, case):
    T, N = case[4], case[3]
    got = {k: leaves[k].grad.cpu().numpy() for k in PARAMS}
    got.update({k: v.grad.cpu().numpy() for k, v in lv.items()})
    got.setdefault('a', np.zeros((T, N, 0)))
    return got


@pytest.mark.parametrize('case', CASES, ids=str)
def test_model_filter_against_the_reference(case):
    M, D, Do, N, T, reverse, with_vx, k_factor, mask = case
    ref = fc.reference(case)
    p, lv, cond, eps, W = _leaves(case)
    gp, leaves = _model(p, M, D, Do)
    traj, kl = gp.filter(lv['h0'], lv.get('a'), lv['ytilde'], eps, lv.get('var_x'), lv['var_y'], cond=cond, k_factor=k_factor,
                         reverse=reverse)
    assert traj.grad_fn is not None and kl.grad_fn is not None and traj.shape == (T, N, Do) and kl.shape == ()
    traj_rule('traj', traj.detach().cpu().numpy(), ref['traj'])
    kl_rule(float(kl.detach()), ref['kl'])
    ((W * traj).sum() + fc.KL_WEIGHT * kl).backward()
    assert all(leaves[k].grad is not None for k in PARAMS) and all(v.grad is not None for v in lv.values())
    _check_grads(_collect(lv, leaves, case), ref, case)


@pytest.mark.parametrize('case', [CASES[1], CASES[9]], ids=str)
def test_autograd_function_and_eval_path(case):
    from cbfssm.hip import autograd
    M, D, Do, N, T, reverse, with_vx, k_factor, mask = case
    ref = fc.reference(case)
    p, lv, cond, eps, W = _leaves(case)
    gp, leaves = _model(p, M, D, Do)
    traj, kl = autograd.gp_filter(gp._pack, lv['h0'], lv.get('a'), lv['ytilde'], eps, lv.get('var_x'), lv['var_y'],
                                  *gp.parameters(), cond=cond, k_factor=k_factor, reverse=reverse)
    assert traj.grad_fn is not None and kl.grad_fn is not None
    ((W * traj).sum() + fc.KL_WEIGHT * kl).backward()
    _check_grads(_collect(lv, leaves, case), ref, case)
    # nothing requires grad: the forward kernel alone, the same numbers bitwise
    gp0, _ = _model(p, M, D, Do, grad=())
    args = [lv['h0'].detach(), lv['a'].detach() if 'a' in lv else None, lv['ytilde'].detach(), eps,
            lv['var_x'].detach() if 'var_x' in lv else None, lv['var_y'].detach()]
    t0, k0 = gp0.filter(*args, cond=cond, k_factor=k_factor, reverse=reverse)
    assert t0.grad_fn is None and k0.grad_fn is None
    assert torch.equal(t0, traj.detach()) and torch.equal(k0, kl.detach())
    # no chain, no step: empty results, no launch
    te, ke = gp0.filter(args[0][:0], None if args[1] is None else args[1][:, :0], args[2][:, :0], eps[:, :0], args[4], args[5],
                        k_factor=k_factor, reverse=reverse)
    assert te.shape == (T, 0, Do) and float(ke) == 0.0
    te, ke = gp0.filter(args[0], None if args[1] is None else args[1][:0], args[2][:0], eps[:0], args[4], args[5])
    assert te.shape == (0, N, Do) and float(ke) == 0.0


@pytest.mark.parametrize('case', [CASES[1], CASES[4], CASES[6], CASES[10]], ids=str)
def test_nothing_conditioned_is_the_rollout(case):
    """cond = 0 everywhere against gp_rollout on the same inputs (ytilde all NaN: it is never read into a result)"""
    M, D, Do, N, T, reverse, with_vx, k_factor, mask = case
    p, lv, _, eps, W = _leaves(case)
    lv['ytilde'] = _nan(T, N, Do).requires_grad_()
    gpf, lf = _model(p, M, D, Do)
    traj, kl = gpf.filter(lv['h0'], lv.get('a'), lv['ytilde'], eps, lv.get('var_x'), lv['var_y'],
                          cond=torch.zeros(T, N, device=DEV), k_factor=k_factor, reverse=reverse)
    assert float(kl.detach()) == 0.0
    ((W * traj).sum() + fc.KL_WEIGHT * kl).backward()
    _, lv2, _, _, _ = _leaves(case)
    gpr, lr = _model(p, M, D, Do)
    traj_r, ent = gpr.rollout(lv2['h0'], lv2.get('a'), eps, lv2.get('var_x'), reverse=reverse)
    (W * traj_r).sum().backward()
    traj_rule('filter against the rollout', traj.detach().cpu().numpy(), traj_r.detach().cpu().numpy())
    for k in ('h0', 'a', 'var_x'):
        if k in lv:
            within_rule(k, lv[k].grad.cpu().numpy(), lv2[k].grad.cpu().numpy())
    for k in PARAMS:
        within_rule(k, lf[k].grad.cpu().numpy(), lr[k].grad.cpu().numpy())
    assert not torch.any(lv['var_y'].grad) and not torch.any(lv['ytilde'].grad)


# one case per K^-1 placement of the forward tile: registers (up to seven row blocks; CASES[4] is the trimmed tile),
# streamed with one row block per wave (ten), streamed with two per wave (from thirteen)
@pytest.mark.parametrize('case', [CASES[1], CASES[4], CASES[6], CASES[7]], ids=str)
def test_dense_and_two_triangular_forward_agree(case):
    ref = fc.reference(case)
    od, ot = _abi(case, 'dense', backward=False), _abi(case, 'tri', backward=False)
    traj_rule('tri against dense', ot['traj'], od['traj'])
    traj_rule('dense against the reference', od['traj'], ref['traj'])
    traj_rule('tri against the reference', ot['traj'], ref['traj'])
    kl_rule(ot['kl'], od['kl'])
    kl_rule(od['kl'], ref['kl'])
    kl_rule(ot['kl'], ref['kl'])


@pytest.mark.parametrize('condition', [True, False])
def test_against_the_products_own_forward_pass(condition):
    """pass_kernel<..., MODE_FWD> (pinned to the oracle elsewhere) through ops.HipElbo.run: the filter from x[0] with the
    tiled u, ytilde = [y | y2] and the mask condition || t < recog_len - 1 reproduces x[1:] and kl_x"""
    from cbfssm import synthetic as syn
    from cbfssm.hip import autograd, ops
    w = syn.tiny(M=20, dim_x=4, dim_u=2, dim_y=2, B=3, S=6, T=12, recog_len=4)
    cfg = w.model_config()
    p = syn.perturb_params(syn.make_params(w))
    u, y = syn.make_inputs(w)
    noise = syn.make_noise(w)
    eng = ops.HipElbo(cfg, DEV)
    eng.prepare(p)
    ws = eng.run(u, y, noise, condition=condition)
    B, S, T, N = w.B, w.S, w.T, w.B * w.S
    x, y2, kl_x = ws.x.clone(), ws.y2.clone(), float(ws.out[1])
    ud, yd = _dev(u), _dev(y)
    a = ud[:, :T - 1].permute(1, 0, 2)[:, :, None, :].expand(T - 1, B, S, w.dim_u).reshape(T - 1, N, w.dim_u)
    yt = yd[:, 1:].permute(1, 0, 2)[:, :, None, :].expand(T - 1, B, S, w.dim_y).reshape(T - 1, N, w.dim_y)
    ytilde = torch.cat([yt, y2[1:]], 2).contiguous()
    cond = torch.tensor([1.0 if (condition or t < w.recog_len - 1) else 0.0 for t in range(T - 1)], device=DEV)
    cond = cond[:, None].expand(T - 1, N).contiguous()
    eps = _dev(noise['eps_f']).reshape(T - 1, N)
    traj, kl = autograd.gp_filter_eval(eng.pack_f, x[0], a.contiguous(), ytilde, eps, eng.var_x, eng.var_y, cond=cond,
                                       k_factor=w.k_factor)
    traj_rule('filter against x[1:]', traj.cpu().numpy(), x[1:].cpu().numpy())
    kl_rule(float(kl), kl_x)
    assert kl_x > 0.0


def _predict_loop(gp, lv, cond, eps, k_factor, reverse):
    from cbfssm.hip import autograd
    return fc.filter_loop(lambda X: autograd.gp_predict(gp._pack, X, *gp.parameters()), lv['h0'],
                          lv['a'] if 'a' in lv else torch.zeros(eps.shape[0], eps.shape[1], 0, dtype=torch.float64, device=DEV),
                          lv['ytilde'], cond, eps, lv.get('var_x'), lv['var_y'], k_factor, reverse)


@pytest.mark.parametrize('case', [CASES[1], CASES[7]], ids=str)
def test_against_a_python_loop_over_gp_predict(case):
    """what the surface offered before: one gp_predict per step and tensor-library elementwise ops, on the GPU"""
    M, D, Do, N, T, reverse, with_vx, k_factor, mask = case

    def run(fused):
        p, lv, cond, eps, W = _leaves(case)
        gp, leaves = _model(p, M, D, Do)
        if fused:
            traj, kl = gp.filter(lv['h0'], lv.get('a'), lv['ytilde'], eps, lv.get('var_x'), lv['var_y'], cond=cond,
                                 k_factor=k_factor, reverse=reverse)
        else:
            traj, kl = _predict_loop(gp, lv, cond, eps, k_factor, reverse)
        ((W * traj).sum() + fc.KL_WEIGHT * kl).backward()
        return traj.detach().cpu().numpy(), float(kl.detach()), _collect(lv, leaves, case)
    tf_, kf, gf = run(True)
    tl, kl_, gl = run(False)
    traj_rule('fused against the loop', tf_, tl)
    kl_rule(kf, kl_)
    for k in gl:
        if gl[k].size:
            within_rule(k, gf[k], gl[k])
