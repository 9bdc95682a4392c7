"""The differentiable GPModel.ekf without a GPU: the two CPU references of tests/gp_ekf_grad_cases.py against each other on
every case the GPU file uses, and the proof from the launcher's source text that the grid rows reach every compiled
(NBLK, DK) leaf of the new backward launcher (launch_gp_ekf_bwd_n, csrc/cbfssm_gp_ekf_bwd.hpp).

Rule: every gradient tensor of (b) within 1e-7 of the largest entry of (a)'s tensor, ten times inside the GPU rule (the
margin gp_ekf_cases.ILL_KEEP uses); a gradient that is exactly zero in (a) (y and var_y under the 'zeros' mask) must be
exactly zero in (b).  The forward values are held to gp_ekf_cases' 1e-9.  Measured: at most 2.3e-10 over the 55 cases
(var_y after forty steps); the file takes about ten seconds."""
import re

import numpy as np
import pytest

import gp_ekf_cases as ec
import gp_ekf_grad_cases as egc
import gp_filter_fullq_grid as fg
import gp_tile_grid as gg
import tile_grid as tg


@pytest.mark.parametrize('c', egc.ALL_CASES, ids=str)
def test_the_two_references_agree(c):
    a, b = egc.reference(c), egc.reference(c, coding='b')
    for k in ('means', 'covs', 'loglik'):
        assert egc.rel_err(b[k], a[k]) < 1e-9, (c, k)
    worst = {}
    for k in egc.grad_names(c) + list(egc.PARAMS):
        ga, gb = a['g_' + k], b['g_' + k]
        assert ga.shape == gb.shape and np.all(np.isfinite(ga)) and np.all(np.isfinite(gb)), (c, k)
        worst[k] = egc.rel_err(gb, ga)
        print('%s %-16s max|ref| %.3e  (b) against (a) %.2e' % (c, k, np.abs(ga).max(), worst[k]))
    assert all(e < egc.CPU_RULE for e in worst.values()), (c, worst)


@pytest.mark.parametrize('which', egc.PARTIALS)
def test_the_two_references_agree_on_partial_cotangents(which):
    c = egc.PARTIAL_CASE
    a, b = egc.reference(c, which), egc.reference(c, which, 'b')
    for k in egc.grad_names(c) + list(egc.PARAMS):
        assert egc.rel_err(b['g_' + k], a['g_' + k]) < egc.CPU_RULE, (which, k)


def test_reference_conventions():
    """P0's gradient is that of the lower triangle; y has no gradient where cond = 0; nothing conditioned: none for var_y"""
    c = ec.case(30, 7, 5)
    r = egc.reference(c)
    assert np.all(np.triu(r['g_P0'], 1) == 0.0) and np.abs(np.tril(r['g_P0'], -1)).max() > 0.0
    cond = ec.make_inputs(c)['cond']
    assert np.all(r['g_y'][cond == 0] == 0.0) and np.all(np.isnan(ec.make_inputs(c)['y'][cond == 0]))
    z = egc.reference(ec.case(30, 7, 5, mask='zeros'))
    assert np.all(z['g_y'] == 0.0) and np.all(z['g_var_y'] == 0.0)


# ---- every (NBLK, DK) leaf of the backward launcher is reached by a grid row
def _compiled():
    text = tg._read('cbfssm_gp_ekf_bwd.hpp')
    heights = gg._instantiated('CBF_GPEKFBWD_INSTANTIATE')
    dks = gg._case_values(text, 'launch_gp_ekf_bwd_n')
    assert heights and dks
    return text, heights, dks


def test_every_leaf_of_the_backward_launcher_is_reached_by_a_grid_row():
    text, heights, dks = _compiled()
    # every DK case goes to one kernel launcher, which takes the wave layout and stash mode from GpBwdCfg<NBLK>
    body = gg._body(text, 'launch_gp_ekf_bwd_n')
    assert sorted(int(v) for v in re.findall(r'launch_gp_ekf_bwd_k<NBLK, (\d+)>', body)) == sorted(dks)
    assert 'gp_ekf_bwd_kernel<NBLK, C::RB, DK, C::STASH>' in gg._body(text, 'launch_gp_ekf_bwd_k')
    # the host dispatcher switches over the heights that are instantiated
    host = tg._read('cbfssm_gp_ekf_bwd.hip')
    assert re.search(r'#define X\(NB\) case NB: return launch_gp_ekf_bwd_nb##NB\([^\n]*\n\s*CBF_FOR_EACH_GPBWD_NBLK\(X\)', host)
    assert sorted(heights) == sorted(gg.dispatch_heights())
    compiled = {(nb, dk) for nb in heights for dk in dks}
    got = {(nb, dk) for nb, dk, _ in fg.reached()}
    assert compiled - got == set(), sorted(compiled - got)
    # and the forward under grad takes the same leaves of launch_gp_ekf_n
    fwd = tg._read('cbfssm_gp_ekf.hpp')
    assert {(nb, dk) for nb in gg._instantiated('CBF_GPEKF_INSTANTIATE') for dk in gg._case_values(fwd, 'launch_gp_ekf_n')} \
        == compiled
    assert 'gp_ekf_kernel<NBLK, C::RB, DK, true, true>' in gg._body(fwd, 'launch_gp_ekf_k')
