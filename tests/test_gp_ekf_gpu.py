"""GPModel.ekf on the GPU: cbfssm_gp_ekf_f64 through cbfssm.hip.autograd.gp_ekf_eval and cbfssm.model.gp_tf.GPModel.ekf,
against reference (a) of tests/gp_ekf_cases.py (the CPU oracle's predict, Jacobians by autodiff, the joint Kalman update).
Rule: every entry of means and covs within 1e-8 of the largest entry of the reference tensor, loglik within 1e-8 of
max |loglik| (the trajectory rule of the rollout and filter tests); a reference log-likelihood of exactly zero (nothing
conditioned) must be met exactly.  No ill-conditioned case runs: neither candidate passes the keep criterion
(tests/gp_ekf_cases.py says why).

The three cross-checks against existing kernels are held to 1e-12 of the largest entry: they compare the same closed form
evaluated by two kernels on the same device, not a kernel against a CPU coding.

Measured on an MI355X (profiles/gp_ekf/README.md): over the 36 grid rows in the three forms at most 9.5e-12 (means), 1.3e-11
(covs), 1.4e-12 (loglik), all at (257, 6, 3) where the two CPU references differ by 1.7e-11; 1.3e-11 after forty steps;
at most 3.3e-14 on the other mask and edge cases; the cross-checks 2.0e-15, 4.1e-16, 3.3e-16 and 7.3e-16.  The file takes
about three seconds."""
import numpy as np
import pytest
import torch

import gp_ekf_cases as ec
import gp_tile_grid as grid
from gp_autograd_cases import PARAMS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RULE, CROSS_RULE = 1e-8, 1e-12


def _dev(a):
    return None if a is None else torch.tensor(np.asarray(a), dtype=torch.float64, device=DEV)


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


def _args(c, **over):
    """the device arguments (m0, P0, a, y, var_x, var_y) and cond of a case; a is None where the GP takes the state alone"""
    i = dict(ec.make_inputs(c))
    i.update(over)
    a = _dev(i['a']) if c[1] > c[2] else None
    return (_dev(i['m0']), _dev(i['P0']), a, _dev(i['y']), _dev(i['var_x']), _dev(i['var_y'])), _dev(i['cond'])


def _ekf(c, **over):
    M, D, Do = c[:3]
    args, cond = _args(c, **over)
    return _model(ec.make_inputs(c)['p'], M, D, Do).ekf(*args, cond=cond)


def _check(c, out, tag, rule=RULE):
    ref = ec.reference_joint(c)
    errs = {}
    for k, t in zip(('means', 'covs', 'loglik'), out):
        g, r = t.cpu().numpy(), ref[k]
        assert g.shape == r.shape, (k, g.shape, r.shape)
        assert np.all(np.isfinite(g)), (c, tag, k)
        scale = np.abs(r).max()
        if scale == 0.0:
            assert k == 'loglik' and np.all(g == 0.0), (c, tag, k)
            errs[k] = 0.0
            continue
        errs[k] = float(np.abs(g - r).max() / scale)
        print('%s %-5s %-6s max|ref| %.3e  err/max %.2e' % (c, tag, k, scale, errs[k]))
    assert all(e < rule for e in errs.values()), (c, tag, errs)
    return errs


# ---- every compiled leaf
@pytest.mark.parametrize('name', grid.ROW_IDS)
def test_every_compiled_leaf_against_the_oracle(name):
    """one small shape per compiled (tile height, DK) leaf, two chain groups with the second ragged, a random mask with NaN in
    y, in the form the automatic switch picks and with the pack forced to dense and to two-triangular"""
    c = ec.grid_case(grid.ROW_BY_NAME[name])
    M, D, Do = c[:3]
    from cbfssm.hip import autograd as ag
    _check(c, _ekf(c), 'auto')
    args, cond = _args(c)
    p = ec.make_inputs(c)['p']
    for mode in ('dense', 'tri'):
        _check(c, ag.gp_ekf_eval(_pack(p, M, D, Do, mode), *args, cond=cond), mode)


# ---- masks and edges
@pytest.mark.parametrize('c', ec.MASK_CASES + ec.EDGE_CASES, ids=str)
def test_masks_and_edges_against_the_oracle(c):
    out = _ekf(c)
    _check(c, out, 'auto')
    covs = out[1]
    assert torch.equal(covs, covs.transpose(2, 3))                       # bitwise symmetric
    scale = float(covs.abs().max())
    assert float(torch.linalg.eigvalsh(covs.cpu()).min()) >= -1e-12 * scale


def test_a_gp_with_fewer_inputs_than_outputs_is_refused():
    """(64, 2, 3) of gp_linearize_cases.ILL_CASES: D < Do.  (Its other case, (130, 3, 2), does not pass the keep criterion of
    an ill-conditioned case -- see gp_ekf_cases -- so no ill-conditioned case runs here.)"""
    M, D, Do = ec.ILL_REFUSED
    import gp_autograd_cases as gc
    p = gc.make_inputs(M, D, Do, 1)[0]
    z = torch.zeros
    with pytest.raises(ValueError):
        _model(p, M, D, Do).ekf(z(3, Do, device=DEV), None, None, z(2, 3, 1, device=DEV), None, z(1, device=DEV) + 0.1)


# ---- cross-checks against existing kernels
CROSS = ec.case(100, 21, 14, T=1, mask='zeros')


def _cross(name, g, r):
    err = float((g - r).abs().max() / r.abs().max())
    print('%-46s max|ref| %.3e  err/max %.2e' % (name, float(r.abs().max()), err))
    assert err <= CROSS_RULE, (name, err)


def test_one_free_step_from_a_point_belief_is_predict():
    c = CROSS
    M, D, Do = c[:3]
    (m0, _, a, y, var_x, var_y), cond = _args(c)
    gp = _model(ec.make_inputs(c)['p'], M, D, Do)
    means, covs, ll = gp.ekf(m0, None, a, y, var_x, var_y, cond=cond)
    fmean, fvar = gp.predict(torch.cat([m0, a[0]], 1))
    _cross('means[0] = m0 + fmean', means[0], m0 + fmean)
    _cross('covs[0] = diag(fvar + var_x)', covs[0], torch.diag_embed(fvar + var_x))
    assert torch.equal(ll, torch.zeros_like(ll))


def test_one_free_step_is_the_congruence_with_transition_jacobians():
    c = CROSS
    M, D, Do = c[:3]
    (m0, P0, a, y, var_x, var_y), cond = _args(c)
    gp = _model(ec.make_inputs(c)['p'], M, D, Do)
    covs = gp.ekf(m0, P0, a, y, var_x, var_y, cond=cond)[1]
    A, _ = gp.transition_jacobians(m0, a[0])
    _, fvar = gp.predict(torch.cat([m0, a[0]], 1))
    _cross('covs[0] = A P0 A^T + diag(fvar + var_x)', covs[0], A @ P0 @ A.transpose(1, 2) + torch.diag_embed(fvar + var_x))


def test_one_fully_observed_step_from_a_point_belief_is_the_filter_mean():
    c = ec.case(100, 21, 14, T=1, Dy=14, mask='ones')
    M, D, Do = c[:3]
    (m0, _, a, y, var_x, var_y), cond = _args(c)
    assert cond is None
    gp = _model(ec.make_inputs(c)['p'], M, D, Do)
    means = gp.ekf(m0, None, a, y, var_x, var_y)[0]
    traj, _ = gp.filter(m0, a, y, torch.zeros(1, c[3], dtype=torch.float64, device=DEV), var_x, var_y, k_factor=1.0)
    _cross('means[0] = traj[0] of filter(eps = 0)', means[0], traj[0])


# ---- properties
@pytest.mark.parametrize('c', [ec.case(100, 21, 14), ec.case(200, 13, 7)], ids=str)
def test_two_calls_are_bitwise_equal(c):
    for x, z in zip(_ekf(c), _ekf(c)):
        assert torch.equal(x, z)


@pytest.mark.parametrize('M,D,Do', ec.CHAIN_GROUP_SHAPES)
def test_the_first_chain_group_does_not_see_the_second(M, D, Do):
    c = ec.case(M, D, Do)
    i = ec.make_inputs(c)
    head = {k: (None if i[k] is None else np.ascontiguousarray(i[k][:, :16])) for k in ('a', 'y', 'cond')}
    head.update(m0=i['m0'][:16].copy(), P0=i['P0'][:16].copy())
    full, part = _ekf(c), _ekf(c, **head)
    assert part[0].shape[1] == 16
    assert torch.equal(full[0][:, :16], part[0]) and torch.equal(full[1][:, :16], part[1]) and torch.equal(full[2][:16], part[2])


def test_nothing_conditioned_reads_no_observation():
    c = ec.case(30, 7, 5, mask='zeros')
    i = ec.make_inputs(c)
    out = _ekf(c)
    nan = _ekf(c, y=np.full_like(i['y'], np.nan))
    assert torch.equal(out[2], torch.zeros_like(out[2]))
    for x, z in zip(out, nan):
        assert torch.isfinite(z).all() and torch.equal(x, z)


def test_outputs_are_fully_written():
    """the entry point on output buffers filled with NaN: every entry comes back written"""
    import ctypes as C
    from cbfssm.hip import lib, ops
    c = ec.case(30, 7, 5)
    M, D, Do, N, T, Dy = c[:6]
    (m0, P0, a, y, var_x, var_y), cond = _args(c)
    pack = _pack(ec.make_inputs(c)['p'], M, D, Do, 'dense')
    l = lib.load()
    nan = lambda *s: torch.full(s, float('nan'), dtype=torch.float64, device=DEV)
    means, covs, ll = nan(T, N, Do), nan(T, N, Do, Do), nan(N)
    work = torch.empty(int(l.cbfssm_gp_ekf_work_elems(C.byref(pack.layout))), dtype=torch.float64, device=DEV)
    ptr = ops._ptr
    rc = l.cbfssm_gp_ekf_f64(C.byref(pack.layout), ptr(pack.buf), ptr(m0), ptr(P0), ptr(a), ptr(y), ptr(cond), ptr(var_x),
                             ptr(var_y), Dy, N, T, ptr(means), ptr(covs), ptr(ll), ptr(work), ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    _check(c, (means, covs, ll), 'raw')


def test_python_surface():
    c = ec.case(30, 7, 5)
    M, D, Do, N, T, Dy = c[:6]
    p = ec.make_inputs(c)['p']
    (m0, P0, a, y, var_x, var_y), cond = _args(c)
    # no chain, no step: empty tensors of the right shapes, nothing launched
    gp = _model(p, M, D, Do)
    means, covs, ll = gp.ekf(m0[:0], P0[:0], a[:, :0], y[:, :0], var_x, var_y, cond=cond[:, :0])
    assert means.shape == (T, 0, Do) and covs.shape == (T, 0, Do, Do) and ll.shape == (0,)
    means, covs, ll = gp.ekf(m0, P0, a[:0], y[:0], var_x, var_y, cond=cond[:0])
    assert means.shape == (0, N, Do) and covs.shape == (0, N, Do, Do) and ll.shape == (N,)
    assert torch.equal(ll, torch.zeros_like(ll))
    # evaluation only, whatever the leaves and the inputs ask for
    gp = _model(p, M, D, Do, grad=PARAMS)
    req = lambda t: t.clone().requires_grad_()
    out = gp.ekf(req(m0), req(P0), req(a), y, req(var_x), req(var_y), cond=cond)
    assert all(not t.requires_grad and t.grad_fn is None for t in out)
    _check(c, out, 'leaves require grad')
    # full-covariance q(z): refused
    with pytest.raises(ValueError):
        _model(p, M, D, Do, q_full=True).ekf(m0, P0, a, y, var_x, var_y, cond=cond)
