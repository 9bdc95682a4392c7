"""The CPU references of the GPModel.adf / GPModel.ads tests against each other (no GPU): tests/gp_adf_cases.py says what
(a), (b) and (c) are.  Every figure is printed.

Measured here: (a) against (b) at most 3.8e-10 of the largest entry (pmeans of (257, 6, 3)) over the cases of the GPU file;
the quadrature (c) at 48 against 64 nodes per axis agrees to 3.7e-14 at the cases' own P0 and var_x (nothing is scaled
down), and (c) against (b) to 2.0e-14 at (50, 9, 2), 1.1e-12 at (64, 4, 1) and 3.5e-11 at (113, 6, 2); ADF against the EKF
of gp_ekf_cases on the Sarcos-shaped case 0.44 (means), 0.33 (covs), 0.11 (loglik); gp_ekf_cases.ILL_CANDIDATE (130, 3, 2)
has (a) against (b) at 1.1e-4 and stays out; no filtered or predictive covariance has a negative eigenvalue."""
import numpy as np
import pytest

import gp_adf_cases as ac
import gp_tile_grid as grid

AGREE, QUAD_CONVERGED, QUAD_RULE = 1e-9, 1e-10, 1e-8
GPU_CASES = list(dict.fromkeys(ac.ALL_GPU_CASES + ac.ADS_CASES + [ac.FAIL_CASE, ac.SARCOS_CASE, ac.case(200, 13, 7)]
                               + [ac.case(M, D, Do) for M, D, Do in ac.CHAIN_GROUP_SHAPES]))


@pytest.mark.parametrize('c', GPU_CASES, ids=str)
def test_the_two_closed_form_references_agree(c):
    a, b = ac.reference_joint(c), ac.reference_sequential(c)
    errs = ac.agreement(a, b)
    print(c, ' '.join('%s %.2e' % kv for kv in errs.items()))
    assert all(e <= AGREE for e in errs.values()), (c, errs)
    for k in ('covs', 'pcovs'):
        lo, scale = ac.min_eig(b[k])
        print(c, k, 'min eig %.3e  max |P| %.3e' % (lo, scale))
        assert lo >= -1e-12 * scale, (c, k, lo, scale)


def test_the_ill_conditioned_candidate_stays_out():
    """gp_ekf_cases.ILL_CANDIDATE (130, 3, 2) is outside the 1e-9 rule between (a) and (b), as it is for ekf: printed, not
    part of the GPU file"""
    c = ac.ec.ILL_CANDIDATE
    assert c not in GPU_CASES
    errs = ac.agreement(ac.reference_joint(c), ac.reference_sequential(c))
    print(c, ' '.join('%s %.2e' % kv for kv in errs.items()))


@pytest.mark.parametrize('c', ac.QUAD_CASES, ids=str)
def test_the_quadrature_confirms_the_closed_form(c):
    """(c) has converged at the cases' own P0 and var_x (48 against 64 nodes per axis), then (c) against (b)"""
    q48, q64 = (ac.reference_quadrature(c, n) for n in ac.QUAD_NODES)
    conv = ac.agreement(q48, q64)
    print(c, '48 / 64 nodes  ', ' '.join('%s %.2e' % kv for kv in conv.items()))
    assert all(e <= QUAD_CONVERGED for e in conv.values()), (c, conv)
    errs = ac.agreement(q64, ac.reference_sequential(c))
    print(c, '(c) against (b)', ' '.join('%s %.2e' % kv for kv in errs.items()))
    assert all(e <= QUAD_RULE for e in errs.values()), (c, errs)


def test_one_step_is_one_closed_form_call_and_the_update():
    c = ac.case(30, 7, 5, T=1, mask='ones')
    M, D, Do, N, T, Dy = c[:6]
    i, b = ac.make_inputs(c), ac.reference_sequential(c)
    S = np.zeros((N, D, D))
    S[:, :Do, :Do] = i['P0']
    r = ac.mc.closed_form(i['p'], np.concatenate([i['m0'], i['a'][0]], 1), S)
    Cx = r['xcov'][:, :, :Do]
    m = i['m0'] + r['fmean']
    P = i['P0'] + Cx + Cx.transpose(0, 2, 1) + r['fcov'] + np.diag(i['var_x'])
    assert np.array_equal(b['pmeans'][0], m) and np.array_equal(b['pcovs'][0], P)
    assert np.array_equal(b['cross'][0], i['P0'] + Cx)
    ll = np.zeros(N)
    ac._update(c, i, 0, m, P, ll, True)                                  # the joint update on (b)'s prediction
    for k, v in (('means', m[None]), ('covs', P[None]), ('loglik', ll)):
        assert ac.rel_err(b[k], v) <= 1e-12, k


def test_the_first_step_from_a_point_belief_is_predict():
    import torch
    c = ac.case(30, 7, 5, T=1, mask='zeros', with_vx=False, with_P0=False)
    i, b = ac.make_inputs(c), ac.reference_sequential(c)
    _, gp = ac.gc.oracle_model(i['p'])
    with torch.no_grad():
        f, fv = gp.predict(torch.tensor(np.concatenate([i['m0'], i['a'][0]], 1)))
    assert ac.rel_err(b['pmeans'][0], i['m0'] + f.numpy()) <= 1e-12
    assert ac.rel_err(b['pcovs'][0], np.einsum('nd,de->nde', fv.numpy(), np.eye(c[2]))) <= 1e-12
    assert not b['cross'].any()


@pytest.mark.parametrize('c', [ac.case(30, 7, 5, mask='zeros'), ac.case(250, 6, 2, N=18, T=4, Dy=1, mask='zeros')], ids=str)
def test_nothing_conditioned_has_zero_loglik(c):
    for ref in (ac.reference_joint(c), ac.reference_sequential(c)):
        assert not ref['loglik'].any()
        assert np.array_equal(ref['means'], ref['pmeans']) and np.array_equal(ref['covs'], ref['pcovs'])


def test_adf_is_not_the_ekf():
    """the guard that the tests can tell the two filters apart"""
    c = ac.SARCOS_CASE
    adf, ekf = ac.reference_sequential(c), ac.ec.reference_joint(c)
    for k in ('means', 'covs', 'loglik'):
        d = ac.rel_err(adf[k], ekf[k])
        print(c, k, 'ADF against EKF %.2f' % d)
        assert d > 1e-2, (k, d)


def test_the_smoother_of_an_unconditioned_filter_is_the_filter():
    c = ac.case(30, 7, 5, mask='zeros')
    f, s = ac.reference_sequential(c), ac.reference_rts(c)
    assert ac.rel_err(s['smeans'], f['means']) <= 1e-10 and ac.rel_err(s['scovs'], f['covs']) <= 1e-10
    assert ac.rel_err(s['init_mean'], f['m0']) <= 1e-10 and ac.rel_err(s['init_cov'], f['P0']) <= 1e-10


def test_the_sweeps_over_the_two_forward_references_agree():
    for c in ac.ADS_CASES:
        a, b = ac.rts(ac.reference_joint(c)), ac.reference_rts(c)
        errs = {k: ac.rel_err(a[k], b[k]) for k in b}
        print(c, ' '.join('%s %.2e' % kv for kv in errs.items()))
        assert all(e <= AGREE for e in errs.values()), (c, errs)


def test_the_grid_reaches_every_compiled_leaf():
    """the kept grid rows reach all 24 (NBLK, DK) leaves of the ADF launcher, read from cbfssm_gp_adf.hpp and gpadf_nb*.hip"""
    leaves = ac.compiled_leaves()
    assert len(leaves) == 24 and leaves == {(nb, dk) for nb in grid.dispatch_heights() for dk in (2, 4, 6)}
    assert len(grid.ROWS) - len(ac.GRID_ROWS) <= 2
    reached = {grid.leaf_key(M, D, Do)[:2] for _, M, D, Do in ac.GRID_ROWS}
    assert reached == leaves, leaves - reached


def test_the_python_surface_exists():
    from cbfssm.hip import autograd as ag
    from cbfssm.model import gp_tf
    assert ag.AdfResult._fields == ('means', 'covs', 'loglik', 'pmeans', 'pcovs', 'cross', 'info')
    assert callable(ag.gp_adf_eval) and callable(ag.gp_ads_eval)
    assert callable(gp_tf.GPModel.adf) and callable(gp_tf.GPModel.ads)
