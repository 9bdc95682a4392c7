"""The input gradients of GPModel.adf on the GPU: cbfssm_gp_adf_bwd_f64 through cbfssm.hip.autograd.gp_adf and
GPModel.adf(..., input_grads=True), against torch autograd through coding (a) of tests/gp_adf_grad_cases.py on the CPU (the
Gram coding of the moments and the joint update, which tests/test_gp_adf_grad_cpu.py pins to a second coding, to the
hand-written reverse recursion and to central differences).

Rule: the project's for gradients -- gp_autograd_cases.within_rule at 1e-6 of the largest entry of the reference tensor, for
every name of grad_names(c); the device cross-check against a loop of transition_moments(..., input_grads=True) is held to
the same rule.  Every check prints its figure; the figures of one run on an MI355X are in profiles/gp_adf_grad/parity.txt."""
import numpy as np
import pytest
import torch

import gp_adf_cases as ac
import gp_adf_grad_cases as ag
import gp_ekf_cases as ec
import gp_surface_poison as gsp
import gp_tile_grid as grid
from gp_autograd_cases import PARAMS, within_rule
from test_gp_ekf_gpu import _dev, _model, _pack

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RULE = 1e-6
FIELDS = ('means', 'covs', 'loglik', 'pmeans', 'pcovs', 'cross', 'info')


def _leaves(c, **over):
    """(the leaves by name, the six arguments, cond) of a case on the device; y keeps its NaN"""
    i = dict(ec.make_inputs(c))
    i.update(over)
    lv = {k: _dev(i[k]).requires_grad_() for k in ag.grad_names(c)}
    return lv, tuple(lv.get(k) for k in ('m0', 'P0', 'a', 'y', 'var_x', 'var_y')), _dev(i['cond'])


def _loss(c, which, res, W=None):
    if W is None:
        return ag.loss_of(c, which, res.means, res.covs, res.loglik)
    Wm, Wc, Wl = (_dev(w) for w in W)
    return (Wm * res.means).sum() + (Wc * res.covs).sum() + (Wl * res.loglik).sum()


def _run(c, which='full', fn=None, W=None, **over):
    """(AdfResult, {name: gradient}) of the case's loss through fn(args, cond) -> AdfResult"""
    M, D, Do = c[:3]
    lv, args, cond = _leaves(c, **over)
    if fn is None:
        gp = _model(ec.make_inputs(c)['p'], M, D, Do)
        fn = lambda a, cd: gp.adf(*a, cond=cd, input_grads=True)     # noqa: E731
    res = fn(args, cond)
    assert res._fields == FIELDS
    assert all(getattr(res, k).grad_fn is not None for k in FIELDS[:3])
    assert all(getattr(res, k).grad_fn is None and not getattr(res, k).requires_grad for k in FIELDS[3:])
    gs = torch.autograd.grad(_loss(c, which, res, W), list(lv.values()), allow_unused=True)
    return res, dict(zip(lv, gs))


def _check(c, tag, gs, ref):
    worst = 0.0
    assert list(gs) == ag.grad_names(c)
    for k, g in gs.items():
        assert g is not None, (c, tag, k)
        if not ref['g_' + k].any():                      # (nothing conditioned: an all-zero reference must be met exactly)
            assert not g.any(), (c, tag, k)
            continue
        within_rule('%s %s g_%s' % (c, tag, k), g.cpu().numpy(), ref['g_' + k], RULE)
        worst = max(worst, ag.rel_err(g.cpu().numpy(), ref['g_' + k]))
    if 'P0' in gs:
        up = torch.triu(gs['P0'], 1)
        assert torch.equal(up, torch.zeros_like(up)) and not torch.signbit(up).any(), 'g_P0 above the diagonal'
    cond = ec.make_inputs(c)['cond']
    if cond is not None:
        assert not gs['y'][_dev(cond) == 0].any(), 'g_y where cond = 0'
    print('%s %s worst over %s: %.2e' % (c, tag, list(gs), worst))
    return worst


def _same_as_the_evaluation_call(c, res, **over):
    M, D, Do = c[:3]
    _, args, cond = _leaves(c, **over)
    ev = _model(ec.make_inputs(c)['p'], M, D, Do).adf(*[None if t is None else t.detach() for t in args], cond=cond)
    for k in FIELDS:
        assert torch.equal(getattr(res, k).detach(), getattr(ev, k)), k


# ---- parity
@pytest.mark.parametrize('name', [r[0] for r in ac.GRID_ROWS])
def test_every_compiled_leaf(name):
    """one small shape per compiled (tile height, DK) leaf, two chain groups with the second ragged, a random mask with NaN in
    y, in the form the automatic switch picks and with the pack forced to dense and to two-triangular"""
    from cbfssm.hip import autograd as hag
    c = ec.grid_case(grid.ROW_BY_NAME[name])
    M, D, Do = c[:3]
    ref = ag.reference(c)
    res, gs = _run(c)
    _check(c, 'auto', gs, ref)
    _same_as_the_evaluation_call(c, res)
    p = ec.make_inputs(c)['p']
    for mode in ('dense', 'tri'):
        pack = _pack(p, M, D, Do, mode)
        _check(c, mode, _run(c, fn=lambda a, cd: hag.gp_adf(pack, *a, cond=cd))[1], ref)


@pytest.mark.parametrize('c', ec.MASK_CASES + ec.EDGE_CASES, ids=str)
def test_masks_and_edges(c):
    res, gs = _run(c)
    _check(c, 'auto', gs, ag.reference(c))
    _same_as_the_evaluation_call(c, res)
    if c[6] == 'zeros':
        assert torch.equal(gs['y'], torch.zeros_like(gs['y'])) and torch.equal(gs['var_y'], torch.zeros_like(gs['var_y']))
    assert ('P0' in gs) == c[8] and ('var_x' in gs) == c[7] and ('a' in gs) == (c[1] > c[2])


# ---- cotangents and masks
@pytest.mark.parametrize('which', ag.PARTIALS)
def test_partial_losses_pass_null_cotangents(which):
    c = ag.PARTIAL_CASE
    _check(c, which, _run(c, which)[1], ag.reference(c, which))


def test_a_loss_of_the_covariances_alone():
    c = ag.PARTIAL_CASE
    Wm, Wc, Wl = ag.weights(c)
    lv = ag.leaves(c)
    covs = ag.adf_torch(c, ag.gg.gram_moments, lv, True)[1]
    ref = dict(zip(('g_' + k for k in lv), torch.autograd.grad((torch.tensor(Wc) * covs).sum(), list(lv.values()))))
    ref = {k: v.numpy() for k, v in ref.items()}
    lvd, args, cond = _leaves(c)
    res = _model(ec.make_inputs(c)['p'], *c[:3]).adf(*args, cond=cond, input_grads=True)
    gs = dict(zip(lvd, torch.autograd.grad((_dev(Wc) * res.covs).sum(), list(lvd.values()))))
    _check(c, 'covs alone', gs, ref)


def test_unused_results_launch_nothing(monkeypatch):
    """all three cotangents None (set_materialize_grads(False)): the gradients are None and the entry point is not called"""
    import types
    from cbfssm.hip import autograd as hag
    from cbfssm.hip import lib
    c = ag.PARTIAL_CASE
    calls = []
    real = lib.load().cbfssm_gp_adf_bwd_f64
    monkeypatch.setattr(lib.load(), 'cbfssm_gp_adf_bwd_f64', lambda *a: calls.append(1) or real(*a))
    ctx = types.SimpleNamespace(layout=lib.pack_layout(*c[:3]), needs_input_grad=(False, False) + (True,) * 6,
                                dims=(c[4], c[3], c[5]), has=(True,) * 4, empty=False)
    with torch.no_grad():
        assert hag._GpAdf.backward(ctx, None, None, None, None, None, None, None) == (None,) * 8
    assert not calls
    # and the patched entry point is what a used result reaches
    _check(c, 'counted', _run(c, 'last_mean')[1], ag.reference(c, 'last_mean'))
    assert calls == [1]


def test_unobserved_entries_reach_no_gradient():
    """the NaNs of y where cond = 0 replaced by other values: no gradient bit changes, and g_y is exactly 0 there"""
    c = ec.case(100, 12, 9)
    i = ec.make_inputs(c)
    assert np.isnan(i['y']).any()
    _, g1 = _run(c)
    _, g2 = _run(c, y=np.where(np.isnan(i['y']), 123.456, i['y']))
    for k in g1:
        assert torch.isfinite(g1[k]).all() and torch.equal(g1[k], g2[k]), k
    assert not g1['y'][_dev(i['cond']) == 0].any()


# ---- conventions
def test_python_surface():
    c = ec.case(30, 7, 5)
    M, D, Do, N, T, Dy = c[:6]
    p = ec.make_inputs(c)['p']
    # input_grads=True without a gradient request, or under no_grad, is the evaluation call
    lv, args, cond = _leaves(c)
    gp = _model(p, M, D, Do, grad=PARAMS)
    out = gp.adf(*[t.detach() for t in args], cond=cond, input_grads=True)
    assert all(t.grad_fn is None and not t.requires_grad for t in out)
    with torch.no_grad():
        out = gp.adf(*args, cond=cond, input_grads=True)
    assert all(t.grad_fn is None for t in out)
    # the default keyword still gives no grad_fn
    assert all(t.grad_fn is None and not t.requires_grad for t in gp.adf(*args, cond=cond))
    # the model is a constant of the call: leaves that require grad end with .grad None, and are not connected
    res = gp.adf(*args, cond=cond, input_grads=True)
    loss = _loss(c, 'full', res)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(loss, gp.parameters()[0], retain_graph=True)
    loss.backward()
    assert all(leaf.grad is None for leaf in gp.parameters()) and all(t.grad is not None for t in lv.values())
    ref = ag.reference(c)
    _check(c, 'backward()', {k: t.grad for k, t in lv.items()}, ref)
    with pytest.raises(RuntimeError):                    # once differentiable, and the graph is freed
        loss.backward()
    # only one input asks
    lv, args, cond = _leaves(c)
    only = [t.detach() for t in args]
    only[2] = args[2]
    res = _model(p, M, D, Do).adf(*only, cond=cond, input_grads=True)
    (ga,) = torch.autograd.grad(_loss(c, 'full', res), [args[2]])
    within_rule('a alone', ga.cpu().numpy(), ref['g_a'], RULE)
    # the gradient is that of the model the forward saw
    lv, args, cond = _leaves(c)
    gp = _model(p, M, D, Do)
    res = gp.adf(*args, cond=cond, input_grads=True)
    with torch.no_grad():
        gp.zeta_mean.mul_(1.7)
    gp.predict(torch.cat([args[0], args[2][0]], 1).detach())
    _check(c, 'model of the forward', dict(zip(lv, torch.autograd.grad(_loss(c, 'full', res), list(lv.values())))), ref)
    # no chain, no step: results with a grad_fn, zero gradients, nothing launched
    m0, P0, a, y, var_x, var_y = args
    gp = _model(p, M, D, Do)
    res = gp.adf(m0, P0, a[:0], y[:0], var_x, var_y, cond=cond[:0], input_grads=True)
    assert res.means.shape == (0, N, Do) and res.loglik.grad_fn is not None
    (g,) = torch.autograd.grad(res.loglik.sum() + res.means.sum(), [m0])
    assert torch.equal(g, torch.zeros_like(m0))
    # full-covariance q(z): refused
    with pytest.raises(ValueError):
        _model(p, M, D, Do, q_full=True).adf(*args, cond=cond, input_grads=True)


# ---- bitwise properties
@pytest.mark.parametrize('c', [ec.case(100, 21, 14), ec.case(200, 13, 7)], ids=str)
def test_two_calls_are_bitwise_equal(c):
    (r1, g1), (r2, g2) = _run(c), _run(c)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    for k in FIELDS:
        assert torch.equal(getattr(r1, k), getattr(r2, k)), k


@pytest.mark.parametrize('M,D,Do', ec.CHAIN_GROUP_SHAPES)
def test_the_first_chain_group_does_not_see_the_second(M, D, Do):
    """chains 0..15 of an N = 21 call against an N = 16 call: the per-chain gradients, bitwise"""
    c = ec.case(M, D, Do)
    i = ec.make_inputs(c)
    head = {k: np.ascontiguousarray(i[k][:, :16]) for k in ('a', 'y', 'cond')}
    head.update(m0=i['m0'][:16].copy(), P0=i['P0'][:16].copy())
    Wm, Wc, Wl = ag.weights(c)
    _, full = _run(c, W=(Wm, Wc, Wl))
    _, part = _run(c, W=(Wm[:, :16], Wc[:, :16], Wl[:16]), **head)
    assert part['m0'].shape[0] == 16
    for k in ('m0', 'P0'):
        assert torch.equal(full[k][:16], part[k]), k
    for k in ('a', 'y'):
        assert torch.equal(full[k][:, :16], part[k]), k


@pytest.mark.parametrize('c', [ec.case(100, 21, 14), ec.case(180, 6, 2)], ids=str)
def test_poisoned_buffers(c):
    """the three words of tests/gp_surface_poison.py in every buffer the glue allocates uninitialised, and in the pack before
    the call and before backward(): results and gradients are bitwise those of the word-0 run"""
    M, D, Do = c[:3]
    p = ec.make_inputs(c)['p']
    outs = {}
    for name in gsp.ORDER:
        word = gsp.WORDS[name]
        with gsp.poisoned_allocations(word) as log:
            gp = _model(p, M, D, Do)
            lv, args, cond = _leaves(c)
            gsp.poison_pack(gp, word)
            res = gp.adf(*args, cond=cond, input_grads=True)
            gsp.poison_pack(gp, word)
            gs = torch.autograd.grad(_loss(c, 'full', res), list(lv.values()))
        torch.cuda.synchronize()
        assert len(log.product()) >= 8                   # the forward's seven results and its work
        outs[name] = {**{k: getattr(res, k).detach() for k in FIELDS}, **{'g_' + k: g for k, g in zip(lv, gs)}}
    for name in gsp.ORDER[1:]:
        for k, v in outs['zero'].items():
            assert torch.equal(v, outs[name][k]), (name, k)
    _check(c, 'poison', {k[2:]: v for k, v in outs['nan'].items() if k.startswith('g_')}, ag.reference(c))


# ---- info
def test_a_flagged_chain_is_nan_and_stays_alone():
    c, n = ac.FAIL_CASE, ac.FAIL_CHAIN
    keep = torch.tensor([k for k in range(c[3]) if k != n], device=DEV)
    (rg, good), (rb, bad) = _run(c), _run(c, P0=ac.fail_P0())
    assert int(rb.info[n]) != 0 and not rb.info[keep].any() and not rg.info.any()
    for k in ('m0', 'P0'):
        assert torch.isnan(bad[k][n]).all(), k
        assert torch.equal(bad[k][keep], good[k][keep]), k
    for k in ('a', 'y'):
        assert torch.isnan(bad[k][:, n]).all(), k
        assert torch.equal(bad[k][:, keep], good[k][:, keep]), k
    assert torch.isnan(bad['var_x']).all() and torch.isnan(bad['var_y']).all()
    assert all(torch.isfinite(g).all() for g in good.values())


# ---- a device cross-check: the per-step loop a caller writes without the fused adjoint
def loop_of_transition_moments(gp, m0, P0, a, y, var_x, var_y, cond):
    """transition_moments(..., input_grads=True) per step plus the scalar updates in the tensor library, on the tape"""
    T, N, Dy = y.shape
    Do = m0.shape[1]
    m, P = m0, P0
    ll = torch.zeros(N, dtype=torch.float64, device=m0.device)
    means, covs = [], []
    for t in range(T):
        m, P, _, _ = gp.transition_moments(m, P, None if a is None else a[t], input_grads=True)
        P = P + torch.diag_embed(var_x.expand(N, Do))
        on = cond[t] != 0
        yt = torch.where(on[:, None], y[t], torch.zeros_like(y[t]))
        for j in range(Dy):
            s = P[:, j, j] + var_y[j]
            dl = yt[:, j] - m[:, j]
            g = P[:, :, j] / s[:, None]
            m = torch.where(on[:, None], m + g * dl[:, None], m)
            P = torch.where(on[:, None, None], P - s[:, None, None] * g[:, :, None] * g[:, None, :], P)
            ll = torch.where(on, ll - 0.5 * (torch.log(2.0 * np.pi * s) + dl * dl / s), ll)
        means.append(m)
        covs.append(P)
    return torch.stack(means), torch.stack(covs), ll


@pytest.mark.parametrize('c', [ec.case(20, 19, 6, N=37, T=8), ec.case(30, 7, 5, N=16, T=40, Dy=2)], ids=str)
def test_a_loop_of_transition_moments_gives_the_same_gradients(c):
    M, D, Do = c[:3]
    gp = _model(ec.make_inputs(c)['p'], M, D, Do)
    _, fused = _run(c, fn=lambda a, cd: gp.adf(*a, cond=cd, input_grads=True))
    lv, args, cond = _leaves(c)
    means, covs, ll = loop_of_transition_moments(gp, *args, cond)
    loop = dict(zip(lv, torch.autograd.grad(ag.loss_of(c, 'full', means, covs, ll), list(lv.values()))))
    for k in fused:
        within_rule('%s fused vs loop g_%s' % (c, k), fused[k].cpu().numpy(), loop[k].cpu().numpy(), RULE)


# ---- use
def test_twenty_adam_steps_on_an_input_sequence_lower_an_expected_cost():
    """open-loop planning: cond = 0, the expected quadratic cost E[(h_T - target)^T (h_T - target)] summed over the steps"""
    c = ec.case(30, 7, 5, T=8, mask='zeros')
    M, D, Do, N, T = c[:5]
    i = ec.make_inputs(c)
    gp = _model(i['p'], M, D, Do)
    _, (m0, P0, a0, y, var_x, var_y), cond = _leaves(c)
    m0, P0, y, var_x, var_y = (t.detach() for t in (m0, P0, y, var_x, var_y))
    a = a0.detach().clone().requires_grad_()
    target = _dev(np.random.default_rng(3).standard_normal(Do))
    opt = torch.optim.Adam([a], lr=0.05)
    costs = []
    for _ in range(20):
        opt.zero_grad()
        res = gp.adf(m0, P0, a, y, var_x, var_y, cond=cond, input_grads=True)
        cost = (((res.means - target) ** 2).sum(2) + torch.einsum('tnii->tn', res.covs)).sum() / N
        cost.backward()
        opt.step()
        costs.append(float(cost.detach()))
    print('expected cost over twenty Adam steps: %.6f -> %.6f' % (costs[0], costs[-1]))
    assert costs[-1] < costs[0] and all(np.isfinite(costs))
