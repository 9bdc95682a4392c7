"""GPModel.eks on the GPU: cbfssm_gp_eks_f64 through cbfssm.hip.autograd.gp_eks_eval and cbfssm.model.gp_tf.GPModel.eks,
against reference (a) of tests/gp_eks_cases.py (the Rauch-Tung-Striebel recursion over a CPU forward pass that uses the
oracle's predict, Jacobians by autodiff and the joint Kalman update).  Rule: every entry of smeans, scovs, init_mean,
init_cov, pmeans, pcovs and lag_one within 1e-8 of the largest entry of the reference tensor (the trajectory rule of the
rollout, filter and ekf tests); a reference tensor that is exactly zero (init_cov when P0 is None) must be met exactly.  No
ill-conditioned case runs, for the reasons tests/gp_ekf_cases.py gives.

The cross-check against transition_jacobians + predict is held to 1e-12 of the largest entry: the same closed form evaluated
by two kernels on the same device.  The filtered results are compared with GPModel.ekf bitwise.

Measured on an MI355X (profiles/gp_eks/README.md), worst of the seven tensors: over the 36 grid rows 6.7e-12 in the
automatic and the dense form and 1.3e-11 in the two-triangular form (scovs, pcovs), all at (257, 6, 3); 2.3e-11 (smeans) after
forty steps, where the two CPU references differ by 2.0e-11; at most 3.9e-13 on the other mask and edge cases; the
cross-checks 3.3e-16 (pcovs[0]), 2.0e-15 (pmeans[0]) and 1.5e-16 (cross[0]).  The file takes about 3.6 seconds without the two
tests over 65 541 steps at its end, whose times profiles/gp_surface_poison/README.md gives."""
import ctypes as C

import numpy as np
import pytest
import torch

import gp_ekf_cases as ec
import gp_eks_cases as sc
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


def _gp(c):
    return _model(ec.make_inputs(c)['p'], *c[:3])


def _eks(c, lag_one=True, **over):
    args, cond = _args(c, **over)
    return _gp(c).eks(*args, cond=cond, lag_one=lag_one)


def _check(c, res, tag, keys=sc.KEYS):
    ref = sc.reference_rts(c)
    errs = {}
    for k in keys:
        g, r = getattr(res, k).cpu().numpy(), ref[k]
        assert g.shape == r.shape, (k, g.shape, r.shape)
        assert np.all(np.isfinite(g)), (c, tag, k)
        errs[k] = sc.rel_err(g, r)
        print('%s %-5s %-9s max|ref| %.3e  err/max %.2e' % (c, tag, k, np.abs(r).max(), errs[k]))
    assert all(e < RULE for e in errs.values()), (c, tag, errs)
    assert torch.equal(res.info, torch.zeros_like(res.info)) and res.info.dtype == torch.int64
    return errs


def _same(x, z):
    """bitwise equal results (NaN equal to NaN), None equal to None"""
    if x is None or z is None:
        return x is None and z is None
    return x.shape == z.shape and bool(torch.equal(torch.nan_to_num(x, nan=1.25e300), torch.nan_to_num(z, nan=1.25e300))) \
        and bool(torch.equal(torch.isnan(x), torch.isnan(z)))


def _sym(P0):
    """the lower triangle, mirrored: what the kernels read of P0"""
    low = torch.tril(P0)
    return low + torch.tril(P0, -1).transpose(-1, -2)


# ---- every compiled leaf of the forward kernel
@pytest.mark.parametrize('name', grid.ROW_IDS)
def test_every_compiled_leaf_against_the_rts_reference(name):
    """one small shape per compiled (tile height, DK) leaf of the forward kernel -- Do from 1 to 16 for the sweep --, two
    chain groups with the second ragged (N = 21: six sweep waves, the last with one chain), a random mask with NaN in y, in
    the form the automatic switch picks and with the pack forced to dense and to two-triangular"""
    c = ec.grid_case(grid.ROW_BY_NAME[name])
    M, D, Do = c[:3]
    from cbfssm.hip import autograd as ag
    _check(c, _eks(c), 'auto')
    args, cond = _args(c)
    p = ec.make_inputs(c)['p']
    for mode in ('dense', 'tri'):
        _check(c, ag.gp_eks_eval(_pack(p, M, D, Do, mode), *args, cond=cond, lag_one=True), mode)


# ---- masks and edges, with the properties every call must have
@pytest.mark.parametrize('c', ec.MASK_CASES + ec.EDGE_CASES, ids=str)
def test_masks_and_edges_against_the_rts_reference(c):
    T = c[4]
    res = _eks(c)
    _check(c, res, 'auto')
    # the filtered results are those of ekf, bitwise; the last smoothed belief is the last filtered one, bitwise
    args, cond = _args(c)
    for x, z in zip((res.means, res.covs, res.loglik), _gp(c).ekf(*args, cond=cond)):
        assert torch.equal(x, z)
    assert torch.equal(res.smeans[T - 1], res.means[T - 1]) and torch.equal(res.scovs[T - 1], res.covs[T - 1])
    # without conditioning the predicted moments are the filtered ones, bitwise
    if cond is not None:
        off = cond == 0
        assert torch.equal(res.pmeans[off], res.means[off]) and torch.equal(res.pcovs[off], res.covs[off])
    # bitwise symmetric, positive semi-definite up to rounding
    for P in (res.scovs, res.init_cov, res.pcovs):
        assert torch.equal(P, P.transpose(-1, -2))
        assert float(torch.linalg.eigvalsh(P.cpu()).min()) >= -1e-12 * float(P.abs().max())
    # lag_one=False: None, and the other results bitwise the same
    off = _eks(c, lag_one=False)
    assert off.lag_one is None and res.lag_one.shape == res.scovs.shape
    for k in sc.KEYS[:-1] + ('loglik', 'means', 'covs', 'info'):
        assert torch.equal(getattr(res, k), getattr(off, k)), k


def test_without_observations_the_smoother_returns_the_filter():
    c = ec.case(30, 7, 5, mask='zeros')
    res = _eks(c)
    (m0, P0, *_), _ = _args(c)
    assert torch.equal(res.smeans, res.means) and torch.equal(res.scovs, res.covs)
    assert torch.equal(res.init_mean, m0) and torch.equal(res.init_cov, _sym(P0))
    assert torch.equal(res.loglik, torch.zeros_like(res.loglik))


def test_nothing_conditioned_reads_no_observation():
    c = ec.case(30, 7, 5, mask='zeros')
    out = _eks(c)
    nan = _eks(c, y=np.full_like(ec.make_inputs(c)['y'], np.nan))
    for x, z in zip(out, nan):
        assert torch.isfinite(z.to(torch.float64)).all() and torch.equal(x, z)
    # a random mask with NaN at cond = 0 (every grid case) already reached no output: _check asserts finite results


# ---- cross-check against existing kernels
def test_the_first_predicted_covariance_is_the_congruence_with_transition_jacobians():
    c = ec.case(100, 21, 14, T=1, mask='zeros')
    (m0, P0, a, y, var_x, var_y), cond = _args(c)
    gp = _gp(c)
    res = gp.eks(m0, P0, a, y, var_x, var_y, cond=cond)
    A, _ = gp.transition_jacobians(m0, a[0])
    fmean, fvar = gp.predict(torch.cat([m0, a[0]], 1))
    for name, g, r in (('pcovs[0] = A P0 A^T + diag(fvar + var_x)', res.pcovs[0],
                        A @ P0 @ A.transpose(1, 2) + torch.diag_embed(fvar + var_x)),
                       ('pmeans[0] = m0 + fmean', res.pmeans[0], m0 + fmean)):
        err = float((g - r).abs().max() / r.abs().max())
        print('%-46s max|ref| %.3e  err/max %.2e' % (name, float(r.abs().max()), err))
        assert err <= CROSS_RULE, (name, err)


# ---- properties
@pytest.mark.parametrize('c', [ec.case(100, 21, 14), ec.case(200, 13, 7)], ids=str)
def test_two_calls_are_bitwise_equal(c):
    for x, z in zip(_eks(c), _eks(c)):
        assert torch.equal(x, z)


@pytest.mark.parametrize('M,D,Do', ec.CHAIN_GROUP_SHAPES)
def test_the_first_chain_group_does_not_see_the_second(M, D, Do):
    c = ec.case(M, D, Do)
    i = ec.make_inputs(c)
    head = {k: (None if i[k] is None else np.ascontiguousarray(i[k][:, :16])) for k in ('a', 'y', 'cond')}
    head.update(m0=i['m0'][:16].copy(), P0=i['P0'][:16].copy())
    full, part = _eks(c), _eks(c, **head)
    assert part.smeans.shape[1] == 16
    for k in ('smeans', 'scovs', 'means', 'covs', 'pmeans', 'pcovs', 'lag_one'):
        assert torch.equal(getattr(full, k)[:, :16], getattr(part, k)), k
    for k in ('loglik', 'init_mean', 'init_cov', 'info'):
        assert torch.equal(getattr(full, k)[:16], getattr(part, k)), k


def _raw(c, lag=True, **over):
    """the entry point on output buffers filled with NaN: (rc, dict of the buffers)"""
    from cbfssm.hip import lib, ops
    M, D, Do, N, T, Dy = c[:6]
    (m0, P0, a, y, var_x, var_y), cond = _args(c, **over)
    pack = _pack(ec.make_inputs(c)['p'], M, D, Do, 'dense')
    l = lib.load()
    nan = lambda *s: torch.full(s, float('nan'), dtype=torch.float64, device=DEV)
    vec, mat = (T, N, Do), (T, N, Do, Do)
    b = {'means': nan(*vec), 'covs': nan(*mat), 'loglik': nan(N), 'pmeans': nan(*vec), 'pcovs': nan(*mat), 'cross': nan(*mat),
         'smeans': nan(*vec), 'scovs': nan(*mat), 'init_mean': nan(N, Do), 'init_cov': nan(N, Do, Do),
         'lag_one': nan(*mat) if lag else None, 'info': nan(N)}
    work = torch.empty(int(l.cbfssm_gp_eks_work_elems(C.byref(pack.layout))), dtype=torch.float64, device=DEV)
    ptr = ops._ptr
    rc = l.cbfssm_gp_eks_f64(C.byref(pack.layout), ptr(pack.buf), ptr(m0), ptr(P0), ptr(a), ptr(y), ptr(cond), ptr(var_x),
                             ptr(var_y), Dy, N, T, *[ptr(v) for v in b.values()], ptr(work), ops._stream())
    torch.cuda.synchronize()
    return rc, b


def test_outputs_are_fully_written_and_cross_is_A_times_P():
    """every entry comes back written, lag1 may be NULL, and cross[0] = A_0 P0 with A_0 from transition_jacobians"""
    import collections
    c = ec.case(30, 7, 5)
    rc, b = _raw(c)
    assert rc == 0
    assert all(bool(torch.isfinite(v).all()) for v in b.values())
    assert torch.equal(b['info'], torch.zeros_like(b['info']))
    _check(c, collections.namedtuple('Raw', list(b))(**dict(b, info=b['info'].to(torch.int64))), 'raw')
    (m0, P0, a, *_), _ = _args(c)
    A, _ = _gp(c).transition_jacobians(m0, a[0])
    ref = A @ _sym(P0)
    err = float((b['cross'][0] - ref).abs().max() / ref.abs().max())
    print('cross[0] = A P0: err/max %.2e' % err)
    assert err <= CROSS_RULE
    rc, b0 = _raw(c, lag=False)
    assert rc == 0
    for k in b:
        assert _same(b[k], b0[k]) or k == 'lag_one', k


def test_a_failed_factorisation_is_reported_and_turns_one_chain_into_nan():
    """P0 = -4 I in one chain: P-_0 of that chain has a negative eigenvalue (test_gp_eks_cpu.py).  A NaN result and a code
    in info, not a device fault."""
    c, n = sc.FAIL_CASE, sc.FAIL_CHAIN
    good, bad = _eks(c), _eks(c, P0=sc.fail_P0())
    assert int(bad.info[n]) == 1 and int(bad.info.abs().sum()) == 1
    assert torch.equal(good.info, torch.zeros_like(good.info))
    assert torch.isnan(bad.init_mean[n]).all() and torch.isnan(bad.init_cov[n]).all() and torch.isnan(bad.lag_one[0, n]).all()
    assert torch.isfinite(bad.smeans[0, n]).all() and torch.equal(bad.smeans[0, n], bad.means[0, n])
    assert torch.isfinite(bad.scovs[0, n]).all() and torch.equal(bad.scovs[0, n], bad.covs[0, n])
    others = [k for k in range(c[3]) if k != n]
    for k in ('smeans', 'scovs', 'means', 'covs', 'pmeans', 'pcovs', 'lag_one'):
        assert torch.equal(getattr(good, k)[:, others], getattr(bad, k)[:, others]), k
    for k in ('loglik', 'init_mean', 'init_cov'):
        assert torch.equal(getattr(good, k)[others], getattr(bad, k)[others]), k
    _check(c, good, 'good')


# ---- more steps than the gain kernel's grid has rows: its loop `for t = blockIdx.y; t < T; t += gridDim.y` goes round
LONG_HORIZON = ec.case(12, 4, 3, N=5, T=65535 + 6, Dy=3, mask='ones')


def _solve_spd(P, B):
    """P^-1 B for symmetric positive definite P (..., d, d) by elimination without pivoting, in the dtype of the arguments
    (np.linalg does not take np.longdouble)"""
    P, B = P.copy(), B.copy()
    d = P.shape[-1]
    for k in range(d):
        for i in range(k + 1, d):
            f = P[..., i, k] / P[..., k, k]
            P[..., i, :] -= f[..., None] * P[..., k, :]
            B[..., i, :] -= f[..., None] * B[..., k, :]
    X = np.empty_like(B)
    for k in range(d - 1, -1, -1):
        acc = B[..., k, :].copy()
        for j in range(k + 1, d):
            acc -= P[..., k, j, None] * X[..., j, :]
        X[..., k, :] = acc / P[..., k, k, None]
    return X


def rts_numpy(means, covs, pmeans, pcovs, cross, m0, P0, dtype=np.float64):
    """the formulas of gp_eks_cases.reference_rts over filtered results (T, N, ...), vectorised over the chains: the gains
    G_t = (cross_t)^T (P-_t)^-1 of all steps at once (they depend on the filter alone), then the backward sweep"""
    means, covs, pmeans, pcovs, cross, m0, P0 = [np.asarray(v, dtype=dtype) for v in (means, covs, pmeans, pcovs, cross, m0, P0)]
    T = means.shape[0]
    G = np.swapaxes(_solve_spd(pcovs, cross), -1, -2)                          # P- symmetric: (P-^-1 cross)^T
    GT = np.swapaxes(G, -1, -2)
    smeans, scovs, lag1 = np.empty_like(means), np.empty_like(covs), np.empty_like(covs)
    ms, Ps = means[T - 1], covs[T - 1]
    smeans[T - 1], scovs[T - 1] = ms, Ps
    for t in range(T - 1, -1, -1):
        mf, Pf = (means[t - 1], covs[t - 1]) if t > 0 else (m0, P0)
        lag1[t] = G[t] @ Ps
        ms = mf + (G[t] @ (ms - pmeans[t])[:, :, None])[:, :, 0]
        Ps = Pf + G[t] @ (Ps - pcovs[t]) @ GT[t]
        if t > 0:
            smeans[t - 1], scovs[t - 1] = ms, Ps
    return {'smeans': smeans, 'scovs': scovs, 'init_mean': ms, 'init_cov': Ps, 'lag_one': lag1}


def test_more_steps_than_the_gain_kernel_has_grid_rows():
    """T = 65535 + 6 steps, N = 5 chains (one sweep wave and a ragged one), the smallest tile, every step fully observed
    (Dy = Do = 3, cond NULL) so that the belief stays bounded, lag_one on: the step loop of gp_eks_gain_kernel goes round a
    second time for the first six steps.  The forward filter is pinned elsewhere; here the gain and sweep kernels are held to
    the numpy Rauch-Tung-Striebel recursion over the filtered results of the SAME call (means, covs, pmeans, pcovs, cross of
    the raw entry point), by the file's 1e-8 rule.  That recursion in np.longdouble against float64, on these inputs,
    measured on an MI355X's results: smeans 1.5e-16, scovs 3.8e-16, init_mean 2.5e-16, init_cov 9.6e-16, lag_one
    4.1e-16 of the largest entry -- seven orders inside the rule (the sweep contracts: every step is observed, so rounding
    does not accumulate over the 65541 steps; max |cov| is 0.105, max |mean| 2.7).  The kernels against the float64
    recursion: 2.3e-16, 7.0e-16, 3.6e-16, 1.0e-15, 6.4e-16.  The call is 1.9 s of kernel time (29 us per step of a serial
    loop); the output buffers of the raw call start as NaN, so a step whose gain was never formed shows."""
    c = LONG_HORIZON
    M, D, Do, N, T, Dy = c[:6]
    assert T > 65535 and N == 5 and Do <= 3 and Dy == Do and ec.make_inputs(c)['cond'] is None
    assert grid.leaf_key(M, D, Do)[0] == min(grid.dispatch_heights())
    rc, b = _raw(c)
    assert rc == 0
    assert all(bool(torch.isfinite(v).all()) for v in b.values())
    assert torch.equal(b['info'], torch.zeros_like(b['info']))
    (m0, P0, *_), _ = _args(c)
    host = {k: v.cpu().numpy() for k, v in b.items()}
    ref = rts_numpy(host['means'], host['covs'], host['pmeans'], host['pcovs'], host['cross'], m0.cpu().numpy(),
                    _sym(P0).cpu().numpy())
    errs = {k: sc.rel_err(host[k], ref[k]) for k in ref}
    print('long horizon: ' + '  '.join('%s %.2e' % kv for kv in errs.items()))
    assert all(e < RULE for e in errs.values()), errs
    assert torch.equal(b['smeans'][T - 1], b['means'][T - 1]) and torch.equal(b['scovs'][T - 1], b['covs'][T - 1])


def test_ads_over_more_steps_than_the_gain_kernel_has_grid_rows():
    """the same inputs through GPModel.ads, which runs the same gain and sweep kernels behind the moment-matching filter:
    results of the shapes of eks, finite, info zero.  The call runs with every allocation of the glue filled with NaN
    (tests/gp_surface_poison.py): the gain of a step the loop left out would stay NaN in its slot and reach the smoothed
    results of every earlier step.  Moment matching inside each of the 65541 steps makes this the longer of the two calls."""
    import gp_surface_poison as gsp
    c = LONG_HORIZON
    M, D, Do, N, T, Dy = c[:6]
    args, cond = _args(c)
    gp = _gp(c)
    with gsp.poisoned_allocations(gsp.WORDS['nan']):
        res = gp.ads(*args, cond=cond, lag_one=True)
    assert torch.equal(res.info, torch.zeros(N, dtype=torch.int64, device=DEV))
    vec, mat = (T, N, Do), (T, N, Do, Do)
    shapes = {'smeans': vec, 'scovs': mat, 'means': vec, 'covs': mat, 'pmeans': vec, 'pcovs': mat, 'lag_one': mat,
              'init_mean': (N, Do), 'init_cov': (N, Do, Do), 'loglik': (N,)}
    for k, shape in shapes.items():
        v = getattr(res, k)
        assert tuple(v.shape) == shape and bool(torch.isfinite(v).all()), k
    assert torch.equal(res.smeans[T - 1], res.means[T - 1]) and torch.equal(res.scovs[T - 1], res.covs[T - 1])


def test_python_surface():
    c = ec.case(30, 7, 5)
    M, D, Do, N, T, Dy = c[:6]
    p = ec.make_inputs(c)['p']
    (m0, P0, a, y, var_x, var_y), cond = _args(c)
    from cbfssm.hip.autograd import EksResult
    assert EksResult._fields == ('smeans', 'scovs', 'loglik', 'means', 'covs', 'pmeans', 'pcovs', 'init_mean', 'init_cov',
                                 'lag_one', 'info')
    # no chain, no step: empty tensors of the right shapes, nothing launched
    gp = _model(p, M, D, Do)
    r = gp.eks(m0[:0], P0[:0], a[:, :0], y[:, :0], var_x, var_y, cond=cond[:, :0], lag_one=True)
    assert isinstance(r, EksResult)
    assert r.smeans.shape == r.means.shape == r.pmeans.shape == (T, 0, Do)
    assert r.scovs.shape == r.covs.shape == r.pcovs.shape == r.lag_one.shape == (T, 0, Do, Do)
    assert r.loglik.shape == r.info.shape == (0,) and r.init_mean.shape == (0, Do) and r.init_cov.shape == (0, Do, Do)
    r = gp.eks(m0, P0, a[:0], y[:0], var_x, var_y, cond=cond[:0])
    assert r.smeans.shape == r.means.shape == r.pmeans.shape == (0, N, Do)
    assert r.scovs.shape == r.covs.shape == r.pcovs.shape == (0, N, Do, Do) and r.lag_one is None
    assert r.init_mean.shape == (N, Do) and r.init_cov.shape == (N, Do, Do)
    assert torch.equal(r.loglik, torch.zeros(N, dtype=torch.float64, device=DEV))
    assert torch.equal(r.info, torch.zeros(N, dtype=torch.int64, device=DEV))
    # evaluation only, whatever the leaves and the inputs ask for
    gp = _model(p, M, D, Do, grad=PARAMS)
    req = lambda t: t.clone().requires_grad_()
    out = gp.eks(req(m0), req(P0), req(a), y, req(var_x), req(var_y), cond=cond, lag_one=True)
    assert all(not t.requires_grad and t.grad_fn is None for t in out)
    _check(c, out, 'leaves require grad')
    # full-covariance q(z) and a GP with fewer inputs than outputs: refused
    with pytest.raises(ValueError):
        _model(p, M, D, Do, q_full=True).eks(m0, P0, a, y, var_x, var_y, cond=cond)
    import gp_autograd_cases as gc
    M2, D2, Do2 = ec.ILL_REFUSED
    z = torch.zeros
    with pytest.raises(ValueError):
        _model(gc.make_inputs(M2, D2, Do2, 1)[0], M2, D2, Do2).eks(z(3, Do2, device=DEV), None, None, z(2, 3, 1, device=DEV), None,
                                                                 z(1, device=DEV) + 0.1)
