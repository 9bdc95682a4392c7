"""The references of the GPModel.moment_match tests against each other and against what they must reduce to (no GPU):
the closed form (a) and Gauss-Hermite quadrature through the oracle's GPModel.predict (b), tests/gp_moment_match_cases.py.

  * (a) against (b) on every belief of rank <= 2 that tests/test_gp_moment_match_gpu.py uses: 1e-9 of the largest entry of
    fmean, fcov, xcov, and of the strictly lower triangle of fcov against its own largest entry (measured: 7.2e-13, 5.6e-11,
    3.5e-13, 1.5e-10, all at (257, 6, 3) where cond_2(K) is 9.8e4), so the reference of the GPU tests is an order inside their 1e-8 rule;
  * (a) at S = 0 is the oracle's predict: fmean, diag fcov = fvar, off-diagonal and xcov zero, to 1e-12;
  * (a) at S = eps^2 S0 approaches linearize's first-order model (J = d fmean / d x by autodiff of the oracle):
        xcov - J S                          is O(eps^4): Cov(f, x) = E[grad f] S by Stein's lemma, and E[grad f] = J + O(eps^2)
        off-diagonal of fcov - J S J^T      is O(eps^4) in the same way
    so halving eps must shrink them to at most 1/8 (theory: 1/16; the factor 2 is for the next order).  The diagonal of
    fcov - diag(fvar) - J S J^T is NOT of that order: it contains E[fvar] - fvar(m) = tr(hess fvar . S) / 2 = O(eps^2), which a
    first-order model does not have.  There halving eps gives 1/4 in theory (measured below: 0.25), and the bound is 1/2 by
    the same factor 2;
  * the rows of gp_tile_grid.ROWS reach every compiled (NBLK, DK) leaf of launch_gp_mm_*."""
import numpy as np
import pytest
import torch

import gp_autograd_cases as gc
import gp_linearize_cases as lc
import gp_moment_match_cases as mc
import gp_tile_grid as grid
import tile_grid as tg

# every case of the GPU file whose beliefs are 'mixed' (rank2 every third point), and the rank-one case
MIXED_CASES = [(M, D, Do, mc.N_POINTS) for _, M, D, Do in grid.ROWS] + mc.EDGE_CASES + \
              [mc.VOLIRO_CASE, mc.LONG_CASE, (113, 9, 1, 17), (300, 21, 7, 19), (30, 7, 5, 9)] + mc.LONG_CASES
BOUND = 1e-9


def _compare(tag, ref, quad):
    """`quad` {n: (fmean, fcov, xcov)}: the four figures of the GPU rule on the tensors of those points -- fmean, fcov, xcov
    against their largest entry, the strictly lower triangle of fcov against its own"""
    ns = sorted(quad)
    fm, fc, xc = [np.stack([quad[n][i] for n in ns]) for i in range(3)]
    e = [mc.rel_err(ref['fmean'][ns], fm), mc.rel_err(ref['fcov'][ns], fc), mc.rel_err(ref['xcov'][ns], xc)]
    if fc.shape[-1] > 1:
        e.append(mc.rel_err(mc.lower(ref['fcov'][ns]), mc.lower(fc)))
    print('%s  fmean %.1e  fcov %.1e  xcov %.1e  lower fcov %.1e' % (tag, e[0], e[1], e[2], e[-1]))
    assert max(e) <= BOUND, (tag, e)
    return e


@pytest.mark.parametrize('case', sorted(set(MIXED_CASES)), ids=str)
def test_closed_form_against_quadrature(case):
    ref, quad = mc.reference_closed_form(*case), mc.reference_quadrature(*case)
    kinds = mc.make_beliefs(*case)[3]
    assert sorted(quad) == [n for n in range(mc.distinct_points(case[3])) if kinds[n] == 'rank2'] and quad
    _compare('%s cond %.1e' % (case, ref['cond']), ref, quad)
    assert ref['cond'] < 1e6
    assert ref['cond'] <= 1e5 or case not in mc.LONG_CASES


def test_long_cases_go_round_the_point_group_loop_twice_at_every_tile_height():
    assert mc.LONG_CASES[0] == mc.LONG_CASE
    assert grid.long_heights(mc.LONG_CASES) == sorted(grid.dispatch_heights())
    assert 'const int64_t cap = gp_mm_maxwg(L->NBLK);' in tg._read('cbfssm_gp_mm.hip')
    assert 'case NB: return GpBwdCfg<NB>::MAXWG;' in tg._read('cbfssm_gp_mm.hip')
    for M, D, Do, npts in mc.LONG_CASES:
        k, r = grid.long_k_r(npts, grid.max_workgroups(grid.leaf_key(M, D, Do)[0]))
        assert 1 <= k <= 4 and 1 <= r <= 15, (M, npts, k, r)
        assert M < 113 or D >= 6, (M, D)
        assert mc.distinct_points(npts) == mc.N_POINTS           # the period-37 repetition of distinct beliefs


def test_closed_form_against_quadrature_rank_one():
    M, D, Do, npts = mc.RANK1_CASE
    p, mean, cov, _ = mc.make_beliefs(M, D, Do, npts, 'rank1')
    ref = mc.reference_closed_form(M, D, Do, npts, 'rank1')
    _, gp = gc.oracle_model(p)
    quad = {}
    for n in range(0, npts, 3):
        V = mc.rank2_factor(M, D, Do, n)[:, :1]
        assert np.array_equal(V @ V.T, cov[n])
        quad[n] = mc.quadrature(gp, mean[n], V)
    _compare('rank one', ref, quad)


def test_full_rank_at_two_input_dimensions():
    """D = 2: the quadrature covers a full-rank covariance (through its Cholesky factor)"""
    M, D, Do, npts = 7, 2, 3, 6
    p, mean, cov, _ = mc.make_beliefs(M, D, Do, npts, 'full')
    ref = mc.closed_form(p, mean, cov)
    _, gp = gc.oracle_model(p)
    assert all(np.linalg.matrix_rank(c) == 2 for c in cov) and ref['cond'] < 1e4
    _compare('D = 2', ref, {n: mc.quadrature(gp, mean[n], np.linalg.cholesky(cov[n])) for n in range(npts)})


@pytest.mark.parametrize('case', [(100, 21, 14, 19), (200, 13, 7, 19), (1, 1, 1, 1)], ids=str)
def test_zero_covariance_is_predict(case):
    M, D, Do, npts = case
    p, mean, cov, _ = mc.make_beliefs(M, D, Do, npts, 'zero')
    ref = mc.reference_closed_form(M, D, Do, npts, 'zero')
    _, gp = gc.oracle_model(p)
    with torch.no_grad():
        fmean, fvar = [t.numpy() for t in gp.predict(torch.tensor(mean))]
    scale = max(np.abs(fmean).max(), np.abs(fvar).max())
    assert np.abs(ref['fmean'] - fmean).max() <= 1e-12 * scale
    assert np.abs(mc.diagonal(ref['fcov']) - fvar).max() <= 1e-12 * scale
    if Do > 1:
        assert np.abs(mc.lower(ref['fcov'])).max() <= 1e-12 * scale
    assert not ref['xcov'].any()


def test_small_covariance_approaches_the_first_order_model():
    M, D, Do, npts = 30, 7, 5, 5
    p, X, _, _ = gc.make_inputs(M, D, Do, npts)
    lin = lc.reference_autodiff(M, D, Do, npts)
    J, fvar = lin['dmean'], lin['fvar']
    ls = mc.softplus(p['lengthscales_unc'])
    A = ls[:, None] * np.random.default_rng(5).standard_normal((D, D)) / np.sqrt(D)
    S0 = A @ A.T

    def remainders(eps):
        cov = np.broadcast_to(eps * eps * S0, (npts, D, D)).copy()
        r = mc.closed_form(p, X, cov)
        JS = J @ cov
        rem = r['fcov'] - JS @ np.transpose(J, (0, 2, 1))
        return np.abs(r['xcov'] - JS).max(), np.abs(mc.lower(rem)).max(), np.abs(mc.diagonal(rem) - fvar).max()

    for eps in (0.1, 0.05):
        big, small = remainders(eps), remainders(eps / 2)
        ratios = [s / b for s, b in zip(small, big)]
        print('eps %.3f -> %.3f: xcov %.3f  off-diagonal %.3f  diagonal %.3f' % (eps, eps / 2, *ratios))
        assert ratios[0] <= 0.125 and ratios[1] <= 0.125          # fourth order in eps
        assert ratios[2] <= 0.5                                   # second order: E[fvar] - fvar(m)
        assert min(big) > 1e-6                                    # (far above rounding)


def test_rows_reach_every_compiled_leaf_of_the_launcher():
    text = tg._read('cbfssm_gp_mm.hpp')
    heights, dks = grid._instantiated('CBF_GPMM_INSTANTIATE'), grid._case_values(text, 'launch_gp_mm_n')
    assert heights == grid.dispatch_heights() and dks == [2, 4, 6]
    # the host dispatcher switches over the same heights, and the Makefile builds one unit per height
    host = tg._read('cbfssm_gp_mm.hip')
    assert 'CBF_FOR_EACH_GPBWD_NBLK(CBF_GPMM_DECLARE)' in host and 'launch_gp_mm_nb##NB' in host
    assert 'gpmm_nb$(n).o' in tg._read('Makefile')
    compiled = {(nb, dk) for nb in heights for dk in dks}
    reached = {grid.leaf_key(M, D, Do)[:2] for _, M, D, Do in grid.ROWS}
    assert reached == compiled, sorted(compiled - reached)
    # the kernel has no other compile-time switch: one instantiation per (NBLK, RB = GpBwdCfg<NBLK>::RB, DK)
    assert len(set(tg.re.findall(r'gp_moment_match_kernel<([^>]*)>', text))) == 1
