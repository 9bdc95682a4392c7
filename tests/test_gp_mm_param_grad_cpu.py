"""The references of the leaf gradients of GPModel.moment_match, on the CPU (tests/gp_mm_param_grad_cases.py): the Gram coding
(a) from the five unconstrained leaves, which the GPU tests compare the kernels with, against the explicit-inverse coding
(b), against the numpy adjoint (c) that was written before any kernel, and against central differences of the numpy closed
form of tests/gp_moment_match_cases.py.

(a), (b) and (c) are compared at N_CPU = 7 points per shape (each belief kind at least twice).  Measured here, per gradient
tensor and of its largest entry: (a) against (b) at most 1.7e-10 on the leaves and 1.1e-10 on mean / cov, except the
variance at (257, 6, 3) -- 9.3e-9, cond_2(K) = 9.8e4 --, all inside the 1e-7 rule, so every case keeps the parameters of
gp_autograd_cases.make_inputs; (c) against (a) at most 1.8e-10 (5.3e-9 for that variance).  The smallest largest entry of
a gradient tensor is 1.4e-3 (zeta_var_unc).

Finite differences at (30, 7, 5), per leaf one random unit direction, central, of the numpy closed form's loss: relative
deviation from (a)'s directional derivative over the step sizes,

    h                  1e-2     1e-3     1e-4     1e-5     1e-6
    zeta_pos           2.9e-06  2.9e-08  6.6e-10  6.3e-09  4.8e-08
    zeta_mean          1.0e-12  1.3e-11  1.5e-10  1.3e-10  6.5e-10
    zeta_var_unc       1.2e-07  1.1e-09  4.2e-10  8.1e-10  2.6e-08
    variance_unc       3.8e-06  3.8e-08  4.1e-10  1.7e-10  2.3e-09
    lengthscales_unc   6.3e-05  6.3e-07  6.4e-09  1.2e-10  5.2e-08

-- truncation error c h^2 with c <= 0.63 down to h = 1e-4 (the loss is quadratic in zeta_mean: rounding only), rounding
error of about 1e-14 / h below it.  The test uses h = 1e-3 and h = 1e-4 and asks for 1e-5 and 1e-7: sixteen times what the
scan shows for the worst leaf where truncation dominates, and h^2-consistent with each other."""
import numpy as np
import pytest

import gp_mm_grad_cases as gg
import gp_mm_param_grad_cases as pc
import gp_moment_match_cases as mc
import gp_tile_grid as grid

N_CPU = 7
SHAPES = [r[1:] for r in grid.ROWS] + pc.M_EDGES + pc.SHAPE_EDGES
FLOOR = 1e-4         # no gradient tensor's largest entry may be smaller: the relative rule would be vacuous
NAMES = ['g_' + n for n in pc.PARAMS] + ['g_mean', 'g_cov']


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_gram_coding_against_the_inverse_coding_and_the_numpy_adjoint(shape):
    M, D, Do = shape
    a = pc.reference(M, D, Do, N_CPU)
    b = pc.reference(M, D, Do, N_CPU, coding='inverse')
    c = pc.reference(M, D, Do, N_CPU, coding='numpy')
    cf = mc.reference_closed_form(M, D, Do, N_CPU)
    for k in ('fmean', 'fcov', 'xcov'):
        assert pc.rel_err(a[k], cf[k]) < 1e-9, (shape, k)
    for k in NAMES:
        eb, ec, big = pc.rel_err(a[k], b[k]), pc.rel_err(c[k], a[k]), np.abs(a[k]).max()
        print('%s %s (a) vs (b): %.2e, (c) vs (a): %.2e, largest entry %.2e' % (shape, k, eb, ec, big))
        assert eb < pc.CPU_RULE, (shape, k, eb)
        assert ec < pc.CPU_RULE, (shape, k, ec)
        assert big > FLOOR, (shape, k, big)


@pytest.mark.parametrize('variant', ['fmean', 'fcov', 'xcov', 'nocross'])
def test_partial_losses_agree_between_the_codings(variant):
    """a tensor the loss does not reach is exactly zero in all three; the variance under fmean or xcov alone is the
    difference of two terms of the full loss's size (fmean and xcov depend on it through the jitter only) and is held
    to the full loss's entry"""
    M, D, Do = 30, 7, 5
    a, b, c = (pc.reference(M, D, Do, N_CPU, 'mixed', variant, coding) for coding in ('gram', 'inverse', 'numpy'))
    full = pc.reference(M, D, Do, N_CPU)
    for k in NAMES:
        if not a[k].any():
            assert not b[k].any() and not c[k].any(), (variant, k)
            continue
        scale = np.abs(a[k]).max()
        if k == 'g_variance_unc' and variant in ('fmean', 'xcov'):
            scale = np.abs(full[k]).max()
        else:
            assert scale > FLOOR, (variant, k)
        assert np.abs(a[k] - b[k]).max() < pc.CPU_RULE * scale and np.abs(c[k] - a[k]).max() < pc.CPU_RULE * scale, (variant, k)


def test_period_37_references_weigh_every_belief_by_its_count():
    """the long cases: the reference on 37 distinct beliefs with counted weights equals the one over all points"""
    M, D, Do, npts = 12, 4, 3, 1009
    assert mc.distinct_points(npts) == 37 and pc.counts(npts).sum() == npts
    short = pc.reference(M, D, Do, npts)
    p, mean, cov, W = pc.case_inputs(M, D, Do, npts)
    assert mean.shape[0] == npts and W[0].shape[0] == npts
    long = pc.evaluate(p, mean, cov, W)
    for k in NAMES:
        assert pc.rel_err(short[k], long[k]) < 1e-12, k


def test_without_a_covariance_the_numpy_adjoint_is_that_of_predict():
    M, D, Do = 30, 7, 5
    p, mean, _, _ = mc.make_beliefs(M, D, Do, N_CPU, 'zero')
    W = gg.make_weights(M, D, Do, N_CPU)
    a = pc.evaluate(p, mean, None, W, 'nocross')
    c = pc.numpy_adjoint(p, mean, None, *pc.cotangents(W, 'nocross'))
    assert c['g_cov'] is None
    for k in NAMES[:-1]:
        assert pc.rel_err(c[k], a[k]) < pc.CPU_RULE, k


def _numpy_loss(p, mean, cov, W):
    out = mc.closed_form(p, mean, cov)
    return float((W[0] * out['fmean']).sum() + (W[1] * out['fcov']).sum() + (W[2] * out['xcov']).sum())


def fd_scan(steps):
    """{leaf: {h: relative deviation of the central difference from (a)'s directional derivative}}, one direction per leaf"""
    M, D, Do = 30, 7, 5
    p, mean, cov, W = pc.case_inputs(M, D, Do, N_CPU)
    a = pc.reference(M, D, Do, N_CPU)
    rng = np.random.default_rng(321)
    out = {}
    for name in pc.PARAMS:
        d = rng.standard_normal(np.shape(p[name]))
        d /= np.sqrt((d ** 2).sum())
        exact = (a['g_' + name].reshape(d.shape) * d).sum()
        out[name] = {}
        for h in steps:
            up, dn = dict(p), dict(p)
            up[name], dn[name] = p[name] + h * d, p[name] - h * d
            fd = (_numpy_loss(up, mean, cov, W) - _numpy_loss(dn, mean, cov, W)) / (2.0 * h)
            out[name][h] = abs(fd - exact) / abs(exact)
    return out


def test_finite_differences_of_the_numpy_closed_form_for_each_leaf():
    scan = fd_scan([1e-3, 1e-4])
    for name, s in scan.items():
        print('finite differences %s: %s' % (name, {h: '%.2e' % e for h, e in s.items()}))
        assert s[1e-3] < 1e-5 and s[1e-4] < 1e-7, (name, s)


def test_the_grid_reaches_every_leaf_of_the_layouts():
    """the new kernels are not instantiated per (tile height, DK) -- the point pass per padded input width 8 / 16 / 24, the
    tile pass once -- but the slab they fill and the input adjoint they follow are: the rows reach all 24 leaves, every
    input width of the point pass, and both layouts of the slab"""
    heights = grid.dispatch_heights()
    leaves = {(nb, dk) for nb in heights for dk in (2, 4, 6)}
    assert len(leaves) == 24
    assert {grid.leaf_key(M, D, Do)[:2] for _, M, D, Do in grid.ROWS} == leaves
    assert {(D + 7) // 8 for _, M, D, Do in grid.ROWS} == {1, 2, 3}
    assert grid.long_heights(mc.LONG_CASES) == heights
    from cbfssm.hip import lib
    assert {bool(lib.pack_layout(M, D, Do).rev_stash) for M, D, Do in pc.M_EDGES} == {False, True}
    assert not lib.pack_layout(112, 7, 3).rev_stash and lib.pack_layout(113, 7, 3).rev_stash
