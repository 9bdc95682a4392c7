"""The coverage proof of the GP-surface tile grid (tests/gp_tile_grid.py), without a GPU: the table reaches every compiled
leaf of gp_predict_bwd_kernel, gp_rollout_bwd_kernel and gp_rollout_kernel, every trim of the rollout's seven-row-block
tile at every input width and both edges of every tile height -- and on every row the two CPU codings of the reference
agree 100 times closer than the rules of tests/test_gp_tile_grid_gpu.py, so that those rules measure the kernels."""
import numpy as np
import pytest

import gp_autograd_cases as gc
import gp_rollout_cases as rc
import gp_tile_grid as gg

HEIGHTS = gg.dispatch_heights()


def _reached():
    out = {}
    for name, M, D, Do in gg.ROWS:
        out.setdefault(gg.leaf_key(M, D, Do), []).append(name)
    return out


def test_launcher_families_list_the_same_leaves():
    """batch adjoint, rollout, rollout adjoint: one tree, three times, and the heights the host dispatchers switch over"""
    fam = gg.compiled_families()
    assert set(fam) == {'predict_bwd', 'rollout', 'rollout_bwd'}
    assert len(HEIGHTS) >= 8 and len(set(HEIGHTS)) == len(HEIGHTS)
    for key, (heights, dks) in fam.items():
        assert heights == sorted(HEIGHTS), key
        assert dks == [2, 4, 6], key
    assert len(gg.compiled_leaves()) == 3 * len(HEIGHTS)
    trim_height, kts = gg.compiled_trims()
    assert trim_height == 7 and kts == [-1, 0, 1, 2, 3]
    assert len(gg.compiled_rollout_leaves()) == 3 * (len(HEIGHTS) - 1) + 3 * 5


def test_rows_are_named_once_and_within_the_limits():
    assert len(set(gg.ROW_IDS)) == len(gg.ROWS)
    for name, M, D, Do in gg.ROWS:
        assert 1 <= Do <= min(D, 16) and D <= 24 and 1 <= M <= 320, name
        assert M < 113 or D != 4, name                      # (see the module docstring: conditioning)
        nb, dk, kt = gg.leaf_key(M, D, Do)
        assert dk == gg.input_steps(D) and 16 * nb >= M, name
        assert name.startswith('nb%d_' % nb) and name.endswith('_dk%d' % dk), name
        if '_kt' in name:
            assert '_kt%d_' % kt in name, name
    assert gg.N_CHAINS > 16 and gg.N_CHAINS % 16 != 0 and gg.N_POINTS > 32 and gg.N_POINTS % 16 != 0


def test_every_compiled_leaf_is_reached():
    got = {(nb, dk) for nb, dk, _ in _reached()}
    missing = sorted(gg.compiled_leaves() - got)
    assert not missing, 'no row of gp_tile_grid.ROWS reaches (NBLK, DK) %s' % (missing,)
    missing = sorted(gg.compiled_rollout_leaves() - set(_reached()))
    assert not missing, 'no row of gp_tile_grid.ROWS reaches the rollout leaf (NBLK, DK, KT) %s' % (missing,)
    # and no row reaches something the source text does not list (the parser and the host agree)
    assert set(_reached()) <= gg.compiled_rollout_leaves()


def test_every_width_and_trim_at_the_trimmed_height():
    trim_height, kts = gg.compiled_trims()
    got = {(dk, kt) for nb, dk, kt in _reached() if nb == trim_height}
    want = {(dk, kt) for dk in gg.compiled_families()['rollout'][1] for kt in kts}
    assert len(want) == 15 and got == want, sorted(want - got)


def test_first_and_exact_fill_of_every_tile_height():
    Ms = {M for _, M, _, _ in gg.ROWS}
    prev = 0
    for nb in sorted(HEIGHTS):
        assert 16 * prev + 1 in Ms, 'first M of tile height %d' % nb
        assert 16 * nb in Ms, 'exact fill of tile height %d' % nb
        prev = nb


def test_input_and_output_widths():
    assert {D for _, _, D, _ in gg.ROWS} >= {8, 9, 16, 17, 24}
    assert {Do for _, _, _, Do in gg.ROWS} >= {1, 8, 9, 16}
    one_block = [(D, Do) for _, M, D, Do in gg.ROWS if M <= 16 and Do == 16]
    assert any(D > Do for D, Do in one_block), 'Do = 16 on a one-wave workgroup with auxiliary inputs'
    assert any(D == Do for D, Do in one_block), 'Do = 16 on a one-wave workgroup without auxiliary inputs'


def test_long_rows_go_round_the_persistent_loop_twice():
    caps = set()
    for M, D, Do, npts in gg.LONG_ROWS:
        nb, _, _ = gg.leaf_key(M, D, Do)
        blocks, cap = (npts + 15) // 16, gg.max_workgroups(nb)
        assert cap < blocks <= 2 * cap, (M, npts, blocks, cap)
        assert npts % 16 != 0
        caps.add((cap, nb > 7))
    assert {c for c, _ in caps} >= {1024, 256} and sum(stash for _, stash in caps) >= 1
    assert len([1 for M, _, _, _ in gg.LONG_ROWS if M > 112]) >= 2
    # one long row at every tile height, all three caps; the rows after the first three by the rule npts = 16 (cap + k) + r
    assert gg.long_heights(gg.LONG_ROWS) == sorted(gg.dispatch_heights())
    assert {c for c, _ in caps} == {1024, 512, 256}
    assert gg.LONG_ROWS[:3] == [(130, 6, 4, 4149), (300, 6, 4, 4101), (12, 4, 3, 16405)]
    for M, D, Do, npts in gg.LONG_ROWS[3:]:
        k, r = gg.long_k_r(npts, gg.max_workgroups(gg.leaf_key(M, D, Do)[0]))
        assert 1 <= k <= 4 and 1 <= r <= 15, (M, npts, k, r)
        assert M < 113 or D >= 6, (M, D)


def test_chain_group_rows_are_one_stash_height_and_one_below():
    nbs = sorted(gg.leaf_key(*gg.ROW_BY_NAME[n][1:])[0] for n in gg.CHAIN_GROUP_ROWS)
    assert len(nbs) == 2 and nbs[0] <= 7 < nbs[1]


def _agree(name, x, r, tol):
    scale = np.abs(r).max()
    err = np.abs(x - r).max() / scale
    print('%-34s max|ref| %.3e  codings differ by %.2e of it' % (name, scale, err))
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(r)) and scale > 0.0 and err < tol, (name, err)


def _check_zeta_rows(ref, M):
    lo, hi = gg.last_data_block(M)
    for k in gc.PARAMS:
        if k.startswith('zeta'):
            assert np.any(ref['g_' + k].reshape(M, -1)[lo:hi] != 0.0), k


@pytest.mark.parametrize('name', gg.ROW_IDS)
def test_reference_alone_stays_inside_the_tolerances(name):
    """Oracle and second coding agree 100 times inside the rules (gradients 1e-8 of the tensor's largest entry,
    trajectories 1e-10 of max |traj|, entropy 1e-11 relative), K_mm is well conditioned (cond < 1e6: the regime the 1e-6
    gradient rule is stated for) and every gradient carries signal, the rows of the last data row block included."""
    row = gg.ROW_BY_NAME[name]
    _, M, D, Do = row
    cond = gg.kmm_condition(M, D, Do)
    print('cond_2(K_mm + jitter I) %.3e' % cond)
    assert cond < 1e6, cond
    case = gg.rollout_case(row)
    ref, sec = rc.reference(case), rc.evaluate(case, 'second')
    _agree('traj', sec['traj'], ref['traj'], 1e-10)
    assert abs(sec['entropy'] - ref['entropy']) < 1e-11 * abs(ref['entropy'])
    names = ('h0',) + (('a',) if D > Do else ()) + (('var_add',) if case[6] else ()) + gc.PARAMS
    assert ref['g_a'].shape == (gg.N_STEPS, gg.N_CHAINS, D - Do)
    for k in names:
        _agree('rollout: ' + k, sec['g_' + k], ref['g_' + k], 1e-8)
    _check_zeta_rows(ref, M)
    pcase = gg.predict_case(row)
    pref, psec = gg.predict_reference(pcase), gg.evaluate_predict(pcase, 'second')
    for k in ('X',) + gc.PARAMS:
        _agree('predict: ' + k, psec['g_' + k], pref['g_' + k], 1e-8)
    _check_zeta_rows(pref, M)


@pytest.mark.parametrize('case', gg.LONG_ROWS, ids=str)
def test_long_row_reference_alone_stays_inside_the_tolerances(case):
    cond = gg.kmm_condition(*case[:3])
    print('cond_2(K_mm + jitter I) %.3e' % cond)
    assert cond < 1e6, cond
    assert cond <= 1e5 or case in gg.LONG_ROWS[:3], cond       # (the bound the rows of ROWS keep)
    pref, psec = gg.predict_reference(case), gg.evaluate_predict(case, 'second')
    for k in ('X',) + gc.PARAMS:
        _agree('predict: ' + k, psec['g_' + k], pref['g_' + k], 1e-8)
    _check_zeta_rows(pref, case[0])
