"""The coverage proof of the tile grid (tests/tile_grid.py), without a GPU: the table reaches every compiled leaf of the
time-loop kernels, every trim and output width of the seven-row-block tiles, both edges of every tile height and both sides
of the adjoint's LDS-or-streamed switch -- and on every row the two CPU references agree with each other, so that the
tolerances of tests/test_tile_grid_gpu.py measure the kernels and not the reference.

The oracle-agreement part runs on every row of the table (a fraction of a second each), not only on M <= 112."""
import numpy as np
import pytest

from cbfssm import synthetic as syn
import tile_grid as tg

HEIGHTS = sorted({nb for nb, _, _ in tg.compiled_leaves()})
ALL_TRIMS = {-1, 0, 1, 2, 3}


def _reached():
    out = {}
    for name, kw in tg.CASES:
        for key in tg.leaf_keys(kw):
            out.setdefault(key, []).append(name)
    return out


def _rows(pred):
    return [name for name, kw in tg.CASES if pred(tg.workload(kw))]


def _nblk(name):
    return next(iter(tg.leaf_keys(tg.CASE_KW[name])))[0]


def test_launcher_families_list_the_same_leaves():
    """float64 passes, float64 adjoint, float64 input-gradient adjoint, float32 passes, float32 adjoint: one tree, five times"""
    fam = tg.compiled_families()
    assert set(fam) == {'pass', 'rev', 'revin', 'pass32', 'rev32'}
    heights, dks = fam['pass']
    assert len(heights) >= 8 and {dk for dk, _ in dks} >= {2, 4, 6} and {md for _, md in dks} == {'fwd', 'bwd'}
    for key, (h, d) in fam.items():
        assert sorted(h) == sorted(heights) and d == dks, key


def test_rows_are_small_ragged_and_carry_backward_signal():
    from oracle import cbfssm_oracle as orc
    assert len(set(tg.CASE_IDS)) == len(tg.CASES)
    for name, kw in tg.CASES:
        w = tg.workload(kw)
        assert 6 <= w.T <= 12 and w.B in (2, 3) and w.N % 16 != 0 and w.N < 32, name
        for run in (0, 1):
            assert orc.window_schedule(w.T, w.recog_len, run)[0].any(), (name, 'backward run %d never resamples' % run)
        assert w.loss_factors[1] != 0.0, name
        assert w.dim_out_b >= 1 and w.D <= 24 and w.dim_x <= 16, name
        assert {key[1] for key in tg.leaf_keys(kw)} == {tg.input_steps(w.D)}, name


def test_every_compiled_leaf_is_reached():
    got = {(nb, dk, mode) for nb, dk, _, _, mode in _reached()}
    missing = sorted(tg.compiled_leaves() - got)
    assert not missing, 'no row of tile_grid.CASES reaches (NBLK, DK, mode) %s' % (missing,)


def test_seven_row_blocks_every_trim_and_output_width():
    reached = _reached()
    for mode in ('fwd', 'bwd'):
        by_dk = {}
        for nb, dk, kt, kd, md in reached:
            if nb == 7 and md == mode:
                by_dk.setdefault(dk, set()).add(kt)
        assert by_dk[6] == ALL_TRIMS, (mode, by_dk)
        assert any(kts == ALL_TRIMS for dk, kts in by_dk.items() if dk != 6), (mode, by_dk)
        assert {kd for nb, _, _, kd, md in reached if nb == 7 and md == mode} == {2, 4}, mode
    # a backward GP with nine outputs on a trimmed tile: the first Do on the KD = 4 side
    assert _rows(lambda w: 96 < w.M <= 112 and w.dim_out_b == 9)


def test_first_and_exact_fill_of_every_tile_height():
    Ms = {tg.workload(kw).M for _, kw in tg.CASES}
    prev = 0
    for nb in HEIGHTS:
        assert 16 * prev + 1 in Ms, 'first M of tile height %d' % nb
        assert 16 * nb in Ms, 'exact fill of tile height %d' % nb
        prev = nb
    assert 320 in Ms and 96 in Ms


def test_input_widths_and_state_dimensions():
    assert {tg.workload(kw).D for _, kw in tg.CASES} >= {8, 9, 16, 17, 24}
    assert _rows(lambda w: w.dim_x == 16)
    assert _rows(lambda w: w.dim_y == w.dim_x - 1)


def test_both_sides_of_the_adjoints_lds_switch_at_seven_row_blocks():
    """DK = 2: by shape.  DK = 4, 6: the K^-1 image fits at every M of the height, so a row of that width is in
    NO_BLDS_CASES (run once more with the image streamed); when a later geometry makes it overflow, this says so."""
    seven = [(name, tg.workload(kw)) for name, kw in tg.CASES if 64 < kw['M'] <= 112]
    for dk in (2, 4, 6):
        sides = {tg.kinv_in_lds(7, dk, w.M) for _, w in seven if tg.input_steps(w.D) == dk}
        forced = [n for n, w in seven if n in tg.NO_BLDS_CASES and tg.input_steps(w.D) == dk and tg.kinv_in_lds(7, dk, w.M)]
        assert True in sides, dk
        assert False in sides or forced, dk
    assert tg.kinv_in_lds(7, 2, 108) and not tg.kinv_in_lds(7, 2, 109)
    assert tg.kinv_in_lds(7, 4, 112) and tg.kinv_in_lds(7, 6, 112)


def _today_kinv_in_lds(nblk, dk, M):
    """kinv_in_lds as it stood before it took `ig` (RevInGeom<DK, false>), kept to pin the default"""
    rb = 2 if nblk > 7 else 1
    waves = (nblk + rb - 1) // rb
    jb = (4 * dk + 1 + 15) // 16
    psl, ecs = (272, 16) if jb == 2 else (max(jb, 2) * 256, 0)
    base = 2 * 4 * dk * 17 + 2 * (16 * nblk) * 17 + 2 * 16 * 17 + waves * psl + 64 + waves * ecs
    return base + nblk * ((M + 3) // 4) * 64 <= 163840 // 8


def _height_range(nb):
    return range(16 * ([0] + HEIGHTS)[HEIGHTS.index(nb)] + 1, 16 * nb + 1)


def test_lds_switch_default_is_unchanged_and_the_input_gradient_geometry_differs_where_splitj_was_on():
    for nb in HEIGHTS:
        for dk in (2, 4, 6):
            for M in range(1, 16 * nb + 1):
                assert tg.kinv_in_lds(nb, dk, M) == tg.kinv_in_lds(nb, dk, M, ig=False) == _today_kinv_in_lds(nb, dk, M)
                if dk == 2:         # JB = 1: one 16-row block of input rows, nothing to split, IG changes nothing
                    assert tg.kinv_in_lds(nb, dk, M, ig=True) == tg.kinv_in_lds(nb, dk, M), (nb, dk, M)
    # DK 4, 6 (JB = 2) without SPLITJ: 7 * (512 - 272 - 16) more doubles of partial tiles at seven row blocks, and the
    # image that fits at every M of the height by default leaves the LDS after M = 104
    for dk in (4, 6):
        assert tg.kinv_in_lds(7, dk, 104, ig=True) and not tg.kinv_in_lds(7, dk, 105, ig=True) and tg.kinv_in_lds(7, dk, 112)


def test_every_leaf_of_the_input_gradient_family_is_reached():
    """launch_revin_n: 8 heights x 3 DK x 2 directions, each in two K^-1 placements = 96 kernels.  The BLDS = true
    kernels of the heights >= 10 cannot be launched (the image never fits next to the tiles); the grid reaches every
    other one: the rows by shape, the streamed kernels of heights 1, 2, 4 through IG_NO_BLDS_CASES."""
    heights, dks = tg.compiled_families()['revin']
    leaves = {(nb, dk, mode) for nb in heights for dk, mode in dks}
    assert len(leaves) == 48 and leaves <= tg.compiled_leaves()
    got = {key[:3] for _, kw in tg.CASES for key in tg.revin_leaf_keys(kw)}
    missing = sorted(leaves - got)
    assert not missing, 'no row of tile_grid.CASES reaches (NBLK, DK, mode) %s of the input-gradient family' % (missing,)
    launchable = {(nb, dk, mode, blds) for nb, dk, mode in leaves for blds in (False, True)
                  if not blds or any(tg.kinv_in_lds(nb, dk, M, ig=True) for M in _height_range(nb))}
    never = {(nb, dk, mode, True) for nb, dk, mode in leaves if nb >= 10}
    assert len(launchable) == 72 and launchable == {(nb, dk, mode, b) for nb, dk, mode in leaves for b in (False, True)} - never
    reached = {key for _, kw in tg.CASES for key in tg.revin_leaf_keys(kw)}
    reached |= {key for n in tg.IG_NO_BLDS_CASES for key in tg.revin_leaf_keys(tg.CASE_KW[n], no_blds=True)}
    assert reached == launchable, sorted(launchable - reached)


def test_input_gradient_family_both_placements_at_seven_row_blocks_by_shape():
    seven = [(name, kw) for name, kw in tg.CASES if 64 < kw['M'] <= 112]
    for dk in (2, 4, 6):
        for mode in ('fwd', 'bwd'):
            sides = {blds for _, kw in seven for nb, k, md, blds in tg.revin_leaf_keys(kw) if (nb, k, md) == (7, dk, mode)}
            assert sides == {True, False}, (dk, mode, sides)
    # the hand-checked table of the rows: (DK, M in LDS, M streamed)
    for dk, lds, streamed in ((6, (65, 97, 103), (106, 112)), (4, (80,), (105,)), (2, (96, 100, 101, 108), (109,))):
        Ms = {kw['M'] for _, kw in seven if tg.input_steps(tg.workload(kw).D) == dk}
        assert Ms == set(lds) | set(streamed), (dk, sorted(Ms))
        assert all(tg.kinv_in_lds(7, dk, M, ig=True) for M in lds) and not any(tg.kinv_in_lds(7, dk, M, ig=True) for M in streamed)
    # the thresholds themselves: M = 108 | 109 at DK 2, 104 | 105 at DK 4 and 6
    for dk, last in ((2, 108), (4, 104), (6, 104)):
        assert [M for M in _height_range(7) if tg.kinv_in_lds(7, dk, M, ig=True)] == list(range(65, last + 1)), dk


def test_input_gradient_family_placement_is_fixed_at_the_other_heights():
    """always LDS at heights 1, 2, 4; never at heights >= 10 -- whatever M and DK"""
    for nb in HEIGHTS:
        if nb == 7:
            continue
        for dk in (2, 4, 6):
            sides = {tg.kinv_in_lds(nb, dk, M, ig=True) for M in _height_range(nb)}
            assert sides == {nb < 7}, (nb, dk, sides)


def test_input_gradient_sub_tables_cover_what_they_are_for():
    assert {(_nblk(n), tg.input_steps(tg.workload(tg.CASE_KW[n]).D)) for n in tg.IG_NO_BLDS_CASES} == \
        {(nb, dk) for nb in (1, 2, 4) for dk in (2, 4, 6)}
    assert sorted(_nblk(n) for n in tg.IG_STASH_CHUNK_CASES) == [13, 16, 20]
    assert sorted(_nblk(n) for n in tg.IG_HALF_CASES) == HEIGHTS
    assert {tg.input_steps(tg.workload(tg.CASE_KW[n]).D) for n in tg.IG_HALF_CASES} == {2, 4, 6}
    assert all(_nblk(n) > 10 for n in tg.IG_PRSSM_CASES) and tg.IG_PRSSM_CASES
    for n in tg.IG_STASH_CHUNK_CASES:       # enough steps and segments for several time-chunked launches
        assert tg.CASE_KW[n]['T'] >= 6


def test_sub_tables_cover_what_they_are_for():
    assert sorted(_nblk(n) for n in tg.GRAD_NOCOND_CASES) == HEIGHTS
    assert {_nblk(n) for n in tg.HALF_CASES} >= {nb for nb in HEIGHTS if nb > 7}
    kts = {(key[1], key[2]) for n in tg.HALF_CASES for key in tg.leaf_keys(tg.CASE_KW[n])}
    assert kts >= {(6, 1), (6, 2), (2, 1), (2, 2)}


@pytest.mark.parametrize('name', tg.CASE_IDS)
def test_reference_alone_stays_inside_the_tolerances(name):
    """numpy oracle and autograd restatement agree on the loss to 1e-10, every gradient is finite and not identically zero
    (the rows of the last data row block included), and both K_mm are well conditioned: cond < 1e6, the regime the 1e-6
    gradient rule is stated for."""
    from oracle import cbfssm_oracle as orc
    from oracle import cbfssm_torch_ref as tref
    w, cfg, p, u, y, noise = tg.setup(tg.CASE_KW[name])
    for g in 'fb':
        cond = syn.kmm_condition(p, g)
        assert cond < 1e6, (g, cond)
    for condition in ((True, False) if name in tg.GRAD_NOCOND_CASES else (True,)):
        ref = orc.elbo_step(cfg, p, u, y, noise, condition)
        scal, grads = tref.loss_and_grads(cfg, p, u, y, noise, condition)
        assert np.isfinite(ref['loss'])
        assert scal['loss'] == pytest.approx(ref['loss'], rel=1e-10)
        lo, hi = tg.last_data_block(w.M)
        for k in syn.PARAM_NAMES:
            assert np.all(np.isfinite(grads[k])), k
            assert np.any(grads[k] != 0.0), k
            if 'zeta' in k:
                assert np.any(grads[k][lo:hi] != 0.0), k
