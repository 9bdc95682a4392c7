"""GPModel.eks without a GPU: the two CPU references of tests/gp_eks_cases.py -- (a) the Rauch-Tung-Striebel recursion,
(b) the dense joint Gaussian of the whole chain conditioned on all observations at once, with no backward recursion --
agree to 1e-9 of the largest entry of every tensor on EVERY case the GPU tests use, ten times inside the 1e-8 rule of
tests/test_gp_eks_gpu.py; the forward recursion they share reproduces gp_ekf_cases.reference_joint to 1e-12; every P-_t is
positive definite; and P-_0 of the altered chain of the failure case is not.

Measured here, (a) against (b): at most 2.0e-11 (smeans), 1.2e-11 (scovs), 6.1e-12 (lag_one), all at (30, 7, 5), T = 40 under
the random mask; at most 2.5e-14 elsewhere.  min eig P- >= 0.05, cond P- <= 2.0e3.  The smallest eigenvalue of a smoothed
covariance over its largest entry is >= 0 up to rounding, and exactly 0 only for the initial covariance when P0 is None."""
import numpy as np
import pytest

import gp_ekf_cases as ec
import gp_eks_cases as sc

FLOOR = 1e-9


@pytest.mark.parametrize('c', sc.ALL_GPU_CASES, ids=str)
def test_the_two_references_agree(c):
    f, ref = sc.forward(c), ec.reference_joint(c)
    for k in ('means', 'covs', 'loglik'):
        assert sc.rel_err(f[k], ref[k]) <= 1e-12, (c, k)
    ag = sc.agreement(c)
    eig = np.linalg.eigvalsh(f['pcovs'])
    a = sc.reference_rts(c)
    lo = min(float(np.linalg.eigvalsh(a[k]).min() / np.abs(a[k]).max()) if np.abs(a[k]).max() > 0 else 0.0
             for k in ('scovs', 'init_cov'))
    print('%s (a) against (b): %s  min eig P- %.2e  cond P- %.2e  min eig Ps / max %.2e'
          % (c, {k: '%.1e' % v for k, v in ag.items()}, eig.min(), (eig[..., -1] / eig[..., 0]).max(), lo))
    assert all(np.isfinite(v) and v <= FLOOR for v in ag.values()), (c, ag)
    assert eig.min() > 0.0, (c, eig.min())                  # every P-_t is positive definite: the factorisation exists
    assert lo >= -1e-12, (c, lo)
    assert all(np.all(np.isfinite(a[k])) for k in sc.KEYS)
    if not c[8]:                                            # P0 None: the smoothed initial covariance is exactly zero
        assert np.all(a['init_cov'] == 0.0) and np.all(sc.reference_dense(c)['init_cov'] == 0.0)


def test_the_failure_case_is_not_positive_definite_in_one_chain_only():
    f = sc.forward_failing()
    eig = np.linalg.eigvalsh(f['pcovs'][0])
    print('min eig of P-_0 per chain:', np.array2string(eig[:, 0], precision=3))
    assert eig[sc.FAIL_CHAIN, 0] < 0.0
    assert np.all(np.delete(eig[:, 0], sc.FAIL_CHAIN) > 0.0)
    assert np.all(np.isfinite(f['means'])) and np.all(np.isfinite(f['covs']))
