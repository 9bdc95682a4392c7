"""The differentiable GPModel.ekf on the GPU: cbfssm_gp_ekf_save_f64 and cbfssm_gp_ekf_bwd_f64 through
cbfssm.hip.autograd.gp_ekf and GPModel.ekf(..., differentiable=True), against reference (a) of tests/gp_ekf_grad_cases.py
(the CPU oracle's predict, Jacobians by create_graph autodiff, the joint Kalman update, differentiated by autograd).

Rule: the project's gradient rule -- every entry of each of the eleven gradients (m0, P0, a, y, var_x, var_y and the five
parameter tensors) within 1e-6 of the largest entry of its reference tensor (gp_autograd_cases.within_rule); a reference
gradient that is exactly zero must be met exactly.  The forward values are held to test_gp_ekf_gpu's 1e-8 rule and are bitwise
those of gp_ekf_eval.

Measured on an MI355X (profiles/gp_ekf_grad/README.md): over the 36 grid rows in the three forms at most 8.3e-11 (variance_unc
at (257, 6, 3)); 1.3e-10 after forty steps (var_y, where the two CPU references differ by 2.3e-10).  The file takes about six
seconds."""
import numpy as np
import pytest
import torch

import gp_ekf_cases as ec
import gp_ekf_grad_cases as egc
import gp_tile_grid as grid
from gp_autograd_cases import PARAMS, within_rule

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
VALUE_RULE = 1e-8


def _dev(a):
    return None if a is None else torch.tensor(np.asarray(a), dtype=torch.float64, device=DEV)


def _model(p, M, D, Do, grad=PARAMS, q_full=False):
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


def _pack(M, D, Do, mode):
    from cbfssm.hip import ops
    return ops.GPPack(M, D, Do, torch.device(DEV), form_mode=mode)


def _inputs(c, **over):
    """(leaves dict on the device, the positional arguments m0, P0, a, y, var_x, var_y, cond)"""
    i = dict(ec.make_inputs(c))
    i.update(over)
    lv = {k: _dev(i[k]).requires_grad_() for k in egc.grad_names(c)}
    args = tuple(lv.get(k) for k in ('m0', 'P0', 'a', 'y', 'var_x', 'var_y'))
    return lv, args, _dev(i['cond'])


def _grads(c, which='full', mode=None, **over):
    """forward under grad and one backward: (outputs, {name: gradient}) -- through GPModel.ekf, or through autograd.gp_ekf on
    a pack of the forced form"""
    M, D, Do = c[:3]
    p = ec.make_inputs(c)['p']
    lv, args, cond = _inputs(c, **over)
    if mode is None:
        gp = _model(p, M, D, Do)
        params = dict(zip(PARAMS, gp.parameters()))
        out = gp.ekf(*args, cond=cond, differentiable=True)
    else:
        from cbfssm.hip import autograd as ag
        params = {k: _dev(p[k]).requires_grad_() for k in PARAMS}
        pack = _pack(M, D, Do, mode)
        out = ag.gp_ekf(pack, *args, *[params[k] for k in PARAMS], cond=cond)
        assert pack.gp_form() == mode
    assert all(t.grad_fn is not None for t in out)
    loss = egc.loss_of(c, which, *out)
    names = list(lv) + list(PARAMS)
    gs = torch.autograd.grad(loss, [lv[k] for k in lv] + [params[k] for k in PARAMS], allow_unused=True)
    return out, {k: g for k, g in zip(names, gs)}


def _check(c, out, gs, tag, which='full'):
    ref = egc.reference(c, which)
    for k, t in zip(('means', 'covs', 'loglik'), out):
        e = egc.rel_err(t.detach().cpu().numpy(), ref[k])
        print('%s %-5s %-6s err/max %.2e' % (c, tag, k, e))
        assert e < VALUE_RULE, (c, tag, k, e)
    assert set(gs) == set(egc.grad_names(c)) | set(PARAMS)
    for k, g in gs.items():
        r = ref['g_' + k]
        assert g is not None, (c, tag, k)
        g = g.cpu().numpy()
        if np.abs(r).max() == 0.0:
            assert g.shape == r.shape and np.all(g == 0.0), (c, tag, k)
            continue
        within_rule('%s %s %s' % (c[:3], tag, k), g, r)


# ---- every compiled leaf, in the three forms of the pack
@pytest.mark.parametrize('name', grid.ROW_IDS)
def test_every_compiled_leaf_against_the_oracle(name):
    c = ec.grid_case(grid.ROW_BY_NAME[name])
    for mode in (None, 'dense', 'tri'):
        out, gs = _grads(c, mode=mode)
        _check(c, out, gs, mode or 'auto')


# ---- masks and edges
@pytest.mark.parametrize('c', ec.MASK_CASES + ec.EDGE_CASES, ids=str)
def test_masks_and_edges_against_the_oracle(c):
    out, gs = _grads(c)
    _check(c, out, gs, 'auto')


@pytest.mark.parametrize('c', [ec.case(30, 7, 5), ec.case(200, 13, 7)], ids=str)
def test_forward_values_are_bitwise_those_of_the_evaluation(c):
    M, D, Do = c[:3]
    out, _ = _grads(c)
    lv, args, cond = _inputs(c)
    ev = _model(ec.make_inputs(c)['p'], M, D, Do, grad=()).ekf(*[None if t is None else t.detach() for t in args], cond=cond)
    for x, z in zip(out, ev):
        assert torch.equal(x.detach(), z)


# ---- exactness
def test_p0_gradient_is_zero_above_the_diagonal_and_reads_the_lower_triangle():
    c = ec.case(30, 7, 5)
    _, gs = _grads(c)
    g = gs['P0']
    assert torch.equal(torch.triu(g, 1), torch.zeros_like(g)) and float(torch.tril(g, -1).abs().max()) > 0.0
    P0 = ec.make_inputs(c)['P0']
    _, gs2 = _grads(c, P0=np.tril(P0) + 7.0 * np.triu(np.ones_like(P0), 1))           # the upper triangle is never read
    for k in gs:
        assert torch.equal(gs[k], gs2[k]), k


def test_y_gradient_is_zero_where_nothing_is_conditioned():
    c = ec.case(30, 7, 5)
    i = ec.make_inputs(c)
    assert np.all(np.isnan(i['y'][i['cond'] == 0]))
    _, gs = _grads(c)
    off = _dev(i['cond']) == 0
    assert torch.all(gs['y'][off] == 0.0) and float(gs['y'][~off].abs().max()) > 0.0
    for g in gs.values():
        assert torch.isfinite(g).all()
    z = ec.case(30, 7, 5, mask='zeros')
    _, gz = _grads(z, y=np.full_like(ec.make_inputs(z)['y'], np.nan))
    assert torch.equal(gz['y'], torch.zeros_like(gz['y'])) and torch.equal(gz['var_y'], torch.zeros_like(gz['var_y']))
    for g in gz.values():
        assert torch.isfinite(g).all()


@pytest.mark.parametrize('c', [ec.case(100, 21, 14), ec.case(200, 13, 7)], ids=str)
def test_two_backward_calls_are_bitwise_equal(c):
    _, g1 = _grads(c)
    _, g2 = _grads(c)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


@pytest.mark.parametrize('M,D,Do', ec.CHAIN_GROUP_SHAPES)
def test_the_first_chain_group_does_not_see_the_second(M, D, Do):
    c = ec.case(M, D, Do)
    c16 = ec.case(M, D, Do, N=16)
    i = ec.make_inputs(c)
    head = {k: (None if i[k] is None else np.ascontiguousarray(i[k][:, :16])) for k in ('a', 'y', 'cond')}
    head.update(m0=i['m0'][:16].copy(), P0=i['P0'][:16].copy(), p=i['p'], var_x=i['var_x'], var_y=i['var_y'])
    Wm, Wc, Wl = egc.weights(c)

    def run(case, over, n):
        p = ec.make_inputs(c)['p']
        lv, args, cond = _inputs(case, **over)
        out = _model(p, M, D, Do).ekf(*args, cond=cond, differentiable=True)
        loss = (_dev(Wm[:, :n]) * out[0]).sum() + (_dev(Wc[:, :n]) * out[1]).sum() + (_dev(Wl[:n]) * out[2]).sum()
        return dict(zip(('m0', 'P0', 'a', 'y'), torch.autograd.grad(loss, [lv[k] for k in ('m0', 'P0', 'a', 'y')])))

    full, part = run(c, {}, 21), run(c16, head, 16)
    assert torch.equal(full['m0'][:16], part['m0']) and torch.equal(full['P0'][:16], part['P0'])
    assert torch.equal(full['a'][:, :16], part['a']) and torch.equal(full['y'][:, :16], part['y'])


# ---- partial cotangents
@pytest.mark.parametrize('which', egc.PARTIALS)
def test_partial_cotangents(which, monkeypatch):
    """an unused output costs nothing: its cotangent reaches the entry point as NULL (not as a tensor of zeros), and the
    gradients are those of reference (a)"""
    from cbfssm.hip import lib
    l = lib.load()
    real, seen = l.cbfssm_gp_ekf_bwd_f64, []

    def spy(*args):
        seen.append(tuple(x is None for x in args[16:19]))              # gmeans, gcovs, gloglik
        return real(*args)

    monkeypatch.setattr(l, 'cbfssm_gp_ekf_bwd_f64', spy)
    c = egc.PARTIAL_CASE
    out, gs = _grads(c, which=which)
    assert seen == [{'loglik': (True, True, False), 'last_mean': (False, True, True)}[which]]
    _check(c, out, gs, which, which)


# ---- surface
def test_python_surface():
    c = ec.case(30, 7, 5)
    M, D, Do, N, T, Dy = c[:6]
    p = ec.make_inputs(c)['p']
    lv, args, cond = _inputs(c)
    out = _model(p, M, D, Do).ekf(*args, cond=cond, differentiable=True)
    assert all(t.requires_grad and t.grad_fn is not None for t in out)
    out = _model(p, M, D, Do).ekf(*args, cond=cond)
    assert all(not t.requires_grad and t.grad_fn is None for t in out)
    # nothing asks for a gradient: the evaluation, no grad_fn
    det = [None if t is None else t.detach() for t in args]
    out = _model(p, M, D, Do, grad=()).ekf(*det, cond=cond, differentiable=True)
    assert all(t.grad_fn is None for t in out)
    with torch.no_grad():
        out = _model(p, M, D, Do).ekf(*args, cond=cond, differentiable=True)
    assert all(t.grad_fn is None for t in out)
    with pytest.raises(ValueError):
        _model(p, M, D, Do, q_full=True).ekf(*det, cond=cond, differentiable=True)
    M2, D2, Do2 = ec.ILL_REFUSED
    import gp_autograd_cases as gc
    z = torch.zeros
    with pytest.raises(ValueError):
        _model(gc.make_inputs(M2, D2, Do2, 1)[0], M2, D2, Do2).ekf(z(3, Do2, device=DEV), None, None, z(2, 3, 1, device=DEV), None,
                                                                  z(1, device=DEV) + 0.1, differentiable=True)
    # no chain, no step: shapes, zero gradients, nothing launched
    gp = _model(p, M, D, Do)
    m0, P0, a, y, var_x, var_y = args
    for chains in (True, False):
        if chains:
            e = gp.ekf(m0, P0, a[:0], y[:0], var_x, var_y, cond=cond[:0], differentiable=True)
            assert e[0].shape == (0, N, Do) and e[1].shape == (0, N, Do, Do) and torch.equal(e[2], torch.zeros_like(e[2]))
        else:
            e = gp.ekf(m0[:0], P0[:0], a[:, :0], y[:, :0], var_x, var_y, cond=cond[:, :0], differentiable=True)
            assert e[0].shape == (T, 0, Do) and e[1].shape == (T, 0, Do, Do) and e[2].shape == (0,)
        g = torch.autograd.grad(e[2].sum() + e[0].sum(), [lv['m0'], lv['var_y'], gp.zeta_mean], allow_unused=True)
        assert all(x is None or torch.equal(x, torch.zeros_like(x)) for x in g)


def test_the_shared_pack_may_be_prepared_again_before_the_backward():
    c = ec.case(100, 21, 14)
    M, D, Do = c[:3]
    p = ec.make_inputs(c)['p']
    _, ref = _grads(c)
    lv, args, cond = _inputs(c)
    gp = _model(p, M, D, Do)
    out = gp.ekf(*args, cond=cond, differentiable=True)
    with torch.no_grad():                                # other parameters through the same pack
        keep = gp.zeta_mean.detach().clone()
        gp.zeta_mean.mul_(-3.0)
        gp.predict(torch.zeros(4, D, dtype=torch.float64, device=DEV))
        gp.zeta_mean.copy_(keep)
    names = list(lv) + list(PARAMS)
    gs = torch.autograd.grad(egc.loss_of(c, 'full', *out), [lv[k] for k in lv] + list(gp.parameters()))
    for k, g in zip(names, gs):
        assert torch.equal(g, ref[k]), k


# ---- training
def test_ten_adam_steps_lower_the_negative_log_likelihood():
    c = egc.TRAIN_CASE
    M, D, Do = c[:3]
    i = ec.make_inputs(c)
    gp = _model(i['p'], M, D, Do)
    _, args, cond = _inputs(c)
    args = [None if t is None else t.detach() for t in args]
    opt = torch.optim.Adam(gp.parameters(), lr=1e-2)
    hist = []
    for _ in range(11):
        opt.zero_grad()
        loss = -gp.ekf(*args, cond=cond, differentiable=True)[2].sum()
        hist.append(float(loss.detach()))
        loss.backward()
        opt.step()
    print('-loglik: %.6f -> %.6f' % (hist[0], hist[-1]))
    assert np.all(np.isfinite(hist)) and hist[-1] < hist[0]
