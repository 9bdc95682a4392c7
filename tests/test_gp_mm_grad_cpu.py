"""The references of the input gradients of GPModel.moment_match, on the CPU (tests/gp_mm_grad_cases.py): the Gram coding (a),
which the GPU tests compare the kernel with, against the explicit-inverse coding (b) and against central differences of the
numpy closed form of tests/gp_moment_match_cases.py.

(a) and (b) are compared at N_CPU = 7 points per shape (each belief kind at least twice): (b) holds (M, M, D) pair
differences per point.  Measured here: values of (a) against the numpy closed form at most 1.1e-10 of the largest entry,
gradients of (a) against (b) at most 1.0e-10, both at (257, 6, 3) where cond_2(K) = 9.8e4 (below 2e-11 elsewhere); the
smallest largest entry of a gradient tensor is 0.13.  The two codings share the inverse of K, so this does not probe the
conditioning of K: the finite-difference test stands alone for that.

Finite differences at (30, 7, 5), three random unit directions in (mean, tril cov), central, of the numpy closed form's loss:
relative deviation from (a)'s directional derivative over the step sizes, worst of the three directions,

    h      1e-2     1e-3     1e-4     1e-5     1e-6     1e-7
    err    1.0e-4   1.0e-6   8.3e-9   2.9e-8   7.8e-7   1.2e-5

-- truncation error 1.0 h^2 down to h = 1e-4, rounding error about 3e-13 / h below it.  The test uses h = 1e-3 and h = 1e-4
and asks for 1e-5 and 1e-7: ten times what the scan shows where truncation dominates, and h^2-consistent with each other."""
import numpy as np
import pytest

import gp_mm_grad_cases as gg
import gp_moment_match_cases as mc
import gp_tile_grid as grid
import tile_grid as tg

N_CPU = 7
SHAPES = [r[1:] for r in grid.ROWS] + sorted({c[:3] for c in mc.EDGE_CASES})
FLOOR = 1e-4         # no gradient tensor's largest entry may be smaller: the relative rule would be vacuous


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_gram_coding_against_the_inverse_coding_and_the_closed_form(shape):
    M, D, Do = shape
    a = gg.reference(M, D, Do, N_CPU)
    b = gg.reference(M, D, Do, N_CPU, coding='inverse')
    cf = mc.reference_closed_form(M, D, Do, N_CPU)
    for k in ('fmean', 'fcov', 'xcov'):
        err = gg.rel_err(a[k], cf[k])
        print('%s %s (a) vs numpy closed form: %.2e' % (shape, k, err))
        assert err < 1e-9, (shape, k, err)                       # the bound of test_gp_moment_match_cpu on its references
    for k in ('g_mean', 'g_cov'):
        err = gg.rel_err(a[k], b[k])
        big = np.abs(a[k]).max()
        print('%s %s (a) vs (b): %.2e, largest entry %.2e' % (shape, k, err, big))
        assert err < gg.CPU_RULE, (shape, k, err)
        assert big > FLOOR, (shape, k, big)
    iu = np.triu_indices(D, 1)
    for r in (a, b):
        assert not r['g_cov'][:, iu[0], iu[1]].any(), 'the gradient for cov is exactly zero above the diagonal'


@pytest.mark.parametrize('variant', ['fmean', 'fcov', 'xcov', 'nocross'])
def test_partial_losses_agree_between_the_codings(variant):
    M, D, Do = 30, 7, 5
    a = gg.reference(M, D, Do, N_CPU, 'mixed', variant)
    b = gg.reference(M, D, Do, N_CPU, 'mixed', variant, 'inverse')
    for k in ('g_mean', 'g_cov'):
        assert gg.rel_err(a[k], b[k]) < gg.CPU_RULE and np.abs(a[k]).max() > FLOOR


def _numpy_loss(p, mean, cov, W):
    out = mc.closed_form(p, mean, cov)
    return float((W[0] * out['fmean']).sum() + (W[1] * out['fcov']).sum() + (W[2] * out['xcov']).sum())


def fd_scan(steps):
    """{h: worst relative deviation of the central difference from (a)'s directional derivative over three directions}"""
    M, D, Do = 30, 7, 5
    p, mean, cov, _ = mc.make_beliefs(M, D, Do, N_CPU)
    W = gg.make_weights(M, D, Do, N_CPU)
    a = gg.reference(M, D, Do, N_CPU)
    rng = np.random.default_rng(123)
    out = {h: 0.0 for h in steps}
    for _ in range(3):
        dm, dT = rng.standard_normal(mean.shape), np.tril(rng.standard_normal(cov.shape))
        nrm = np.sqrt((dm ** 2).sum() + (dT ** 2).sum())
        dm, dT = dm / nrm, dT / nrm
        dS = dT + np.transpose(np.tril(dT, -1), (0, 2, 1))               # the symmetric matrix the lower triangle stands for
        exact = (a['g_mean'] * dm).sum() + (a['g_cov'] * dT).sum()
        for h in steps:
            fd = (_numpy_loss(p, mean + h * dm, cov + h * dS, W) - _numpy_loss(p, mean - h * dm, cov - h * dS, W)) / (2.0 * h)
            out[h] = max(out[h], abs(fd - exact) / abs(exact))
    return out


def test_finite_differences_of_the_numpy_closed_form():
    scan = fd_scan([1e-3, 1e-4])
    print('finite differences: %s' % {h: '%.2e' % e for h, e in scan.items()})
    assert scan[1e-3] < 1e-5 and scan[1e-4] < 1e-7


def test_the_grid_reaches_every_compiled_leaf_of_the_adjoint():
    text = tg._read('cbfssm_gp_mm_bwd.hpp')
    heights, dks = grid._instantiated('CBF_GPMMB_INSTANTIATE'), grid._case_values(text, 'launch_gp_mmb_n')
    assert heights == grid.dispatch_heights() and dks == [2, 4, 6]
    leaves = {(nb, dk) for nb in heights for dk in dks}
    assert len(leaves) == 24
    assert {grid.leaf_key(M, D, Do)[:2] for _, M, D, Do in grid.ROWS} == leaves
    # the persistent loop's second trip: one long case per tile height
    assert grid.long_heights(mc.LONG_CASES) == heights
