"""The references of the input gradients of GPModel.adf, on the CPU (tests/gp_adf_grad_cases.py): coding (a), which the GPU
tests compare the kernel with, against coding (b), against the hand-written reverse recursion (c) and against central
differences, on every case the GPU file uses (gp_ekf_cases.ALL_GPU_CASES, 55 cases).

Measured here: gradients of (a) against (b) at most 7.7e-10 of the largest entry (g_P0 at (257, 6, 3)), every other row at
most 1.3e-10; values of (a) against gp_adf_cases.reference_sequential at most 2.3e-10 (rule 1e-9); (c) against (a) at most
1.8e-10 (g_a at (257, 6, 3)).  No case is dropped; the smallest largest entry of a gradient tensor is 0.94.

Finite differences at (30, 7, 5), three random unit directions over all six inputs (P0 in its lower triangle, y only where it
is conditioned on), central, of (a)'s loss: relative deviation from (a)'s directional derivative, worst of the directions,

    h      1e-2     1e-3     1e-4     1e-5     1e-6     1e-7
    err    9.3e-5   9.3e-7   9.3e-9   3.7e-9   4.9e-8   4.3e-7

-- truncation error 0.93 h^2 down to h = 1e-4, rounding error about 4e-14 / h below it.

The test uses h = 1e-3 and h = 1e-4 and asks for 1e-5 and 1e-7: ten times what the scan shows where truncation dominates,
and h^2-consistent with each other."""
import numpy as np
import pytest

import gp_adf_cases as ac
import gp_adf_grad_cases as ag
import gp_ekf_cases as ec
import gp_tile_grid as grid
import tile_grid as tg

FD_BOUNDS = {1e-3: 1e-5, 1e-4: 1e-7}
FLOOR = 1e-6         # a gradient tensor's largest entry, unless it is exactly zero: the relative rule would be vacuous


@pytest.mark.parametrize('c', ag.ALL_CASES, ids=str)
def test_the_two_codings_and_the_reverse_recursion_agree(c):
    a, b = ag.reference(c), ag.reference(c, coding='b')
    seq = ac.reference_sequential(c)
    for k in ('means', 'covs', 'loglik'):
        err = ac.rel_err(a[k], seq[k])
        print('%s %s (a) vs reference_sequential: %.2e' % (c, k, err))
        assert err < 1e-9, (c, k, err)
    r = ag.reverse_numpy(c)
    assert sorted(r) == sorted('g_' + k for k in ag.grad_names(c))
    for name in ag.grad_names(c):
        k = 'g_' + name
        big = np.abs(a[k]).max()
        err, errc = ag.rel_err(b[k], a[k]), ag.rel_err(r[k], a[k])
        print('%s %s (b) vs (a): %.2e, (c) vs (a): %.2e, largest entry %.2e' % (c, k, err, errc, big))
        assert err < ag.CPU_RULE and errc < ag.CPU_RULE, (c, k, err, errc)
        assert big > FLOOR or big == 0.0, (c, k, big)
    if 'P0' in ag.grad_names(c):
        iu = np.triu_indices(c[2], 1)
        for g in (a, b, r):
            assert not g['g_P0'][:, iu[0], iu[1]].any(), 'the gradient for P0 is exactly zero above the diagonal'
    if c[6] == 'zeros':
        for g in (a, b, r):
            assert not g['g_y'].any() and not g['g_var_y'].any()
    cond = ec.make_inputs(c)['cond']
    if cond is not None:
        for g in (a, b, r):
            assert not g['g_y'][cond == 0].any(), 'the gradient for y is exactly zero where cond = 0'


@pytest.mark.parametrize('which', ag.PARTIALS)
def test_partial_losses_agree_between_the_codings(which):
    c = ag.PARTIAL_CASE
    a, b, r = ag.reference(c, which), ag.reference(c, which, 'b'), ag.reverse_numpy(c, which)
    for name in ag.grad_names(c):
        k = 'g_' + name
        assert ag.rel_err(b[k], a[k]) < ag.CPU_RULE and ag.rel_err(r[k], a[k]) < ag.CPU_RULE, (which, k)


def fd_scan(steps):
    """{h: worst relative deviation of the central difference from (a)'s directional derivative over three directions}"""
    c = ag.FD_CASE
    i = ec.make_inputs(c)
    a = ag.reference(c)
    names = ag.grad_names(c)
    used = {k: np.ones(i[k].shape, bool) for k in names}
    used['y'] = np.broadcast_to((i['cond'] != 0)[:, :, None], i['y'].shape)
    used['P0'] = np.broadcast_to(np.tril(np.ones(i['P0'].shape[1:], bool)), i['P0'].shape)
    rng = np.random.default_rng(321)
    out = {h: 0.0 for h in steps}
    for _ in range(3):
        d = {k: np.where(used[k], rng.standard_normal(i[k].shape), 0.0) for k in names}
        nrm = np.sqrt(sum((v ** 2).sum() for v in d.values()))
        d = {k: v / nrm for k, v in d.items()}
        exact = sum((a['g_' + k] * d[k]).sum() for k in names)
        for h in steps:
            up = ag.loss_numpy(c, {k: i[k] + h * d[k] for k in names})
            dn = ag.loss_numpy(c, {k: i[k] - h * d[k] for k in names})
            out[h] = max(out[h], abs((up - dn) / (2.0 * h) - exact) / abs(exact))
    return out


def test_central_differences_of_the_first_coding():
    scan = fd_scan([1e-3, 1e-4])
    print('finite differences: %s' % {h: '%.2e' % e for h, e in scan.items()})
    assert scan[1e-3] < FD_BOUNDS[1e-3] and scan[1e-4] < FD_BOUNDS[1e-4]


def test_the_grid_reaches_every_compiled_leaf_of_the_adjoint():
    text = tg._read('cbfssm_gp_adf_bwd.hpp')
    heights, dks = grid._instantiated('CBF_GPADFB_INSTANTIATE'), grid._case_values(text, 'launch_gp_adfb_n')
    assert heights == grid.dispatch_heights() and dks == [2, 4, 6]
    leaves = {(nb, dk) for nb in heights for dk in dks}
    assert len(leaves) == 24 and leaves == ac.compiled_leaves()
    assert {grid.leaf_key(*c[:3])[:2] for c in ag.ALL_CASES} == leaves
