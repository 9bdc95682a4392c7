"""The fused GP rollout on the GPU: cbfssm_gp_rollout_f64 and cbfssm_gp_rollout_bwd_f64 -> cbfssm_reduce_partials_f64 ->
cbfssm_gp_tail_f64 through the C ABI, and cbfssm.model.gp_tf.GPModel.rollout / cbfssm.hip.autograd.gp_rollout, against
reverse-mode autodiff of the recurrence over the CPU oracle (tests/gp_rollout_cases.py, which states the rules: gradients
within 1e-6 of their tensor's largest entry, trajectories within 1e-8 of max |traj|, entropy 1e-9 relative)."""
import ctypes as C

import numpy as np
import pytest
import torch

import gp_rollout_cases as rc
from gp_rollout_cases import CASES, PARAMS, within_rule, traj_rule, entropy_rule

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


def _check_grads(got, ref, names):
    """the gradient rule on every named tensor; a tensor without entries (a when Da = 0) has nothing to check but its shape"""
    for k in names:
        g = np.asarray(got[k])
        r = ref['g_' + k].reshape(g.shape)
        if r.size == 0:
            continue
        within_rule(k, g, r)


def _abi(case, form='dense', backward=True):
    """forward and adjoint through the C ABI on NaN-prefilled outputs; returns a dict of host arrays"""
    from cbfssm.hip import lib as _l, ops
    from cbfssm.hip.ops import _ptr, _stream
    M, D, Do, N, T, reverse, with_var = case
    Da = D - Do
    lib = _l.load()
    p, h0, a, eps, var_add, W = rc.make_inputs(*case)
    pack = ops.GPPack(M, D, Do, torch.device(DEV), form_mode=form)
    pt = {k: _dev(p[k]) for k in PARAMS}
    con = {k: (ops.tf_forward(pt[k]) if k.endswith('_unc') else pt[k]) for k in PARAMS}
    pack.prepare(con['zeta_pos'], con['lengthscales_unc'], con['variance_unc'], con['zeta_mean'], con['zeta_var_unc'])
    lay = pack.layout
    h0d, epsd = _dev(h0), _dev(eps)
    ad = _dev(a) if Da else None
    vad = _dev(var_add) if with_var else None
    groups = (N + 15) // 16
    assert lib.cbfssm_gp_rollout_partials(C.byref(lay), N) == groups
    traj, vsave, ent_part = _nan(T, N, Do), _nan(T, N, Do), _nan(groups + 32)
    _l.check(lib.cbfssm_gp_rollout_f64(C.byref(lay), _ptr(pack.buf), _ptr(h0d), _ptr(ad), _ptr(epsd), _ptr(vad), N, T,
                                       int(reverse), _ptr(traj), _ptr(vsave), _ptr(ent_part), _stream()), 'cbfssm_gp_rollout_f64')
    ent = _nan(1)
    _l.check(lib.cbfssm_reduce_partials_f64(_ptr(ent_part), 1, groups, _ptr(ent), _stream()), 'reduce')
    out = {'traj': traj.cpu().numpy(), 'vsave': vsave.cpu().numpy(), 'entropy': float(ent[0])}
    if not backward:
        return out
    nwg = lib.cbfssm_gp_rollout_bwd_workgroups(C.byref(lay), N)
    nwork = lib.cbfssm_gp_rollout_bwd_work_elems(C.byref(lay), N, T)
    assert nwg == groups and (nwork > 0) == bool(lay.rev_stash)
    gpart = _nan((nwg + 32) * lay.rev_slab)
    work = _nan(nwork) if nwork else None
    image = _nan(lay.NBLK * lay.NBLK * 256) if lay.rev_stash else None
    gh0 = _nan(N, Do)
    ga = _nan(T, N, Da) if Da else None
    gtraj, gent = _dev(W), _dev([rc.ENT_WEIGHT])
    _l.check(lib.cbfssm_gp_rollout_bwd_f64(C.byref(lay), _ptr(pack.buf), _ptr(h0d), _ptr(ad), _ptr(epsd), _ptr(traj),
                                           _ptr(vsave), _ptr(gtraj), _ptr(gent), N, T, int(reverse), _ptr(gh0), _ptr(ga),
                                           _ptr(gpart), _ptr(work), _ptr(image), _stream()), 'cbfssm_gp_rollout_bwd_f64')
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
    out['var_add'] = red[small:small + Do].cpu().numpy()
    out['gflat'] = gflat.cpu().numpy()
    return out


@pytest.mark.parametrize('case', CASES, ids=str)
def test_c_abi_against_the_reference(case):
    ref = rc.reference(case)
    o1, o2 = _abi(case), _abi(case)
    traj_rule('traj', o1['traj'], ref['traj'])
    entropy_rule(o1['entropy'], ref['entropy'])
    assert np.all(np.isfinite(o1['vsave'])) and np.all(o1['vsave'] > 0)
    names = ('h0', 'a') + (('var_add',) if case[6] else ()) + PARAMS
    _check_grads(o1, ref, names)
    for k in ('traj', 'vsave', 'h0', 'a', 'var_add', 'gflat'):
        assert np.array_equal(o1[k], o2[k]), 'two calls differ: ' + k
    assert o1['entropy'] == o2['entropy']


@pytest.mark.parametrize('case', CASES, ids=str)
def test_model_rollout_against_the_reference(case):
    M, D, Do, N, T, reverse, with_var = case
    ref = rc.reference(case)
    p, h0, a, eps, var_add, W = rc.make_inputs(*case)
    gp, leaves = _model(p, M, D, Do)
    h0d = _dev(h0).requires_grad_()
    ad = _dev(a).requires_grad_() if D > Do else None
    vad = _dev(var_add).requires_grad_() if with_var else None
    traj, ent = gp.rollout(h0d, ad, _dev(eps), vad, reverse=reverse)
    assert traj.grad_fn is not None and ent.grad_fn is not None and traj.shape == (T, N, Do) and ent.shape == ()
    traj_rule('traj', traj.detach().cpu().numpy(), ref['traj'])
    entropy_rule(float(ent.detach()), ref['entropy'])
    ((_dev(W) * traj).sum() + rc.ENT_WEIGHT * ent).backward()
    got = {k: leaves[k].grad.cpu().numpy() for k in PARAMS}
    got['h0'] = h0d.grad.cpu().numpy()
    got['a'] = ad.grad.cpu().numpy() if ad is not None else np.zeros((T, N, 0))
    names = ('h0', 'a') + PARAMS
    if with_var:
        got['var_add'] = vad.grad.cpu().numpy()
        names += ('var_add',)
    _check_grads(got, ref, names)


@pytest.mark.parametrize('case', [CASES[1], CASES[4], CASES[7], CASES[8]], ids=str)
def test_dense_and_two_triangular_forward_agree(case):
    ref = rc.reference(case)
    od, ot = _abi(case, 'dense', backward=False), _abi(case, 'tri', backward=False)
    traj_rule('tri against dense', ot['traj'], od['traj'])
    traj_rule('tri against the reference', ot['traj'], ref['traj'])
    entropy_rule(ot['entropy'], od['entropy'])
    entropy_rule(ot['entropy'], ref['entropy'])


@pytest.mark.parametrize('case', [CASES[1], CASES[7]], ids=str)
def test_against_a_python_loop_over_gp_predict(case):
    """what the library offered before: one gp_predict per step and tensor-library elementwise ops, on the GPU"""
    from cbfssm.hip import autograd
    M, D, Do, N, T, reverse, with_var = case
    p, h0, a, eps, var_add, W = rc.make_inputs(*case)

    def run(fused):
        gp, leaves = _model(p, M, D, Do)
        lv = {'h0': _dev(h0).requires_grad_(), 'a': _dev(a).requires_grad_()}
        if with_var:
            lv['var_add'] = _dev(var_add).requires_grad_()
        if fused:
            traj, ent = gp.rollout(lv['h0'], lv['a'], _dev(eps), lv.get('var_add'), reverse=reverse)
        else:
            traj, ent = rc.rollout(lambda X: autograd.gp_predict(gp._pack, X, *gp.parameters()), lv['h0'], lv['a'], _dev(eps),
                                   lv.get('var_add'), reverse)
        ((_dev(W) * traj).sum() + rc.ENT_WEIGHT * ent).backward()
        g = {k: v.grad.cpu().numpy() for k, v in lv.items()}
        g.update({k: leaves[k].grad.cpu().numpy() for k in PARAMS})
        return traj.detach().cpu().numpy(), float(ent.detach()), g
    tf_, ef, gf = run(True)
    tl, el, gl = run(False)
    traj_rule('fused against the loop', tf_, tl)
    entropy_rule(ef, el)
    for k in gl:
        within_rule(k, gf[k], gl[k])


def test_chain_groups_do_not_interact():
    """chains 0..15 of an N = 37 run equal an N = 16 run of the same chains bitwise, on the trajectory and on ga"""
    from cbfssm.hip import autograd
    case = CASES[1]
    M, D, Do, N, T, reverse, with_var = case
    p, h0, a, eps, var_add, W = rc.make_inputs(*case)

    def run(n):
        gp, _ = _model(p, M, D, Do)
        ad = _dev(a[:, :n]).requires_grad_()
        traj, ent = gp.rollout(_dev(h0[:n]), ad, _dev(eps[:, :n]), None, reverse=reverse)
        ((_dev(W[:, :n]) * traj).sum() + rc.ENT_WEIGHT * ent).backward()
        return traj.detach(), ad.grad
    t37, g37 = run(37)
    t16, g16 = run(16)
    assert torch.equal(t37[:, :16], t16) and torch.equal(g37[:, :16], g16)


@pytest.mark.parametrize('case', [CASES[4], CASES[7]], ids=str)
def test_path_without_a_gradient_request(case):
    M, D, Do, N, T, reverse, with_var = case
    p, h0, a, eps, var_add, W = rc.make_inputs(*case)
    gp, _ = _model(p, M, D, Do, grad=())
    args = (_dev(h0), _dev(a), _dev(eps), _dev(var_add))
    t0, e0 = gp.rollout(*args, reverse=reverse)
    assert t0.grad_fn is None and e0.grad_fn is None
    gp2, _ = _model(p, M, D, Do)
    with torch.no_grad():
        t1, e1 = gp2.rollout(*args, reverse=reverse)
    assert t1.grad_fn is None and torch.equal(t1, t0) and torch.equal(e1, e0)
    t2, e2 = gp2.rollout(*args, reverse=reverse)
    assert t2.grad_fn is not None and e2.grad_fn is not None
    assert torch.equal(t2.detach(), t0) and torch.equal(e2.detach(), e0)


def test_composition_in_the_pattern_of_voliros_recognition_run():
    """voliro.py:139-186: the auxiliary input is a per-chain sample of ANOTHER GP's output (times a learnable matrix) next to
    the observations, the run starts from h = 0 and goes backwards in time; gradients reach the second GP and the matrix"""
    import gp_autograd_cases as gc
    M, D, Do, N, T = 20, 19, 6, 37, 8
    du, dy, M2, D2 = 8, 5, 30, 7                      # a = (u (8), y (5)); second GP: 7 inputs -> 5 outputs
    p, _, _, eps, _, W = rc.make_inputs(M, D, Do, N, T, True, False)
    p2, _, _, _ = gc.make_inputs(M2, D2, 5, 1)
    rng = np.random.default_rng(3)
    X2 = 1.4 * rng.standard_normal((T * N, D2))
    A0 = 0.5 * rng.standard_normal((5, du))
    e2 = rng.standard_normal((T * N, 1))
    y = 1.4 * rng.standard_normal((T, N, dy))

    def loss_of(predict2, roll, cv, A):
        fm, fv = predict2(cv(X2))
        u = ((fm + cv(e2) * torch.sqrt(fv)) @ A).reshape(T, N, du)
        traj, ent = roll(torch.zeros(N, Do, dtype=torch.float64, device=A.device), torch.cat([u, cv(y)], 2))
        return (cv(W) * traj).sum() + rc.ENT_WEIGHT * ent

    t1, o1 = gc.oracle_model(p)
    t2, o2 = gc.oracle_model(p2)
    Ar = torch.tensor(A0, requires_grad=True)
    lr = loss_of(o2.predict, lambda h, a: rc.rollout(o1.predict, h, a, torch.tensor(eps), None, True), torch.tensor, Ar)
    lr.backward()
    g1, l1 = _model(p, M, D, Do)
    g2, l2 = _model(p2, M2, D2, 5)
    Ad = _dev(A0).requires_grad_()
    ld = loss_of(g2.predict, lambda h, a: g1.rollout(h, a, _dev(eps), None, reverse=True), _dev, Ad)
    ld.backward()
    assert float(ld.detach()) == pytest.approx(float(lr.detach()), rel=1e-9)
    within_rule('matrix', Ad.grad.cpu().numpy(), Ar.grad.numpy())
    for k in PARAMS:
        within_rule('rollout GP: ' + k, l1[k].grad.cpu().numpy(), t1[k].grad.numpy())
        within_rule('input GP: ' + k, l2[k].grad.cpu().numpy(), t2[k].grad.numpy())


def test_ten_adam_steps_track_the_oracle():
    import gp_autograd_cases as gc
    case = CASES[0]
    M, D, Do, N, T, reverse, with_var = case
    p, h0, a, eps, var_add, W = rc.make_inputs(*case)
    t, _ = gc.oracle_model(p)
    gp, leaves = _model(p, M, D, Do)
    opt_r = torch.optim.Adam([t[k] for k in PARAMS], lr=0.01)
    opt_d = torch.optim.Adam([leaves[k] for k in PARAMS], lr=0.01)
    from oracle import cbfssm_torch_ref as tref
    for step in range(10):
        opt_r.zero_grad()
        ogp = tref.GPModel(*[t[k] for k in PARAMS])
        traj, ent = rc.rollout(ogp.predict, torch.tensor(h0), torch.tensor(a), torch.tensor(eps), None, reverse)
        lr = (torch.tensor(W) * traj).sum() + rc.ENT_WEIGHT * ent
        lr.backward()
        opt_r.step()
        opt_d.zero_grad()
        traj, ent = gp.rollout(_dev(h0), _dev(a), _dev(eps), None, reverse=reverse)
        ld = (_dev(W) * traj).sum() + rc.ENT_WEIGHT * ent
        ld.backward()
        opt_d.step()
        rel = abs(float(ld.detach()) - float(lr.detach())) / abs(float(lr.detach()))
        print('step %d  oracle %.9e  hip %.9e  rel %.2e' % (step, float(lr.detach()), float(ld.detach()), rel))
        assert rel < 1e-6, (step, rel)
