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
    """float64 passes, float64 adjoint, float32 passes, float32 adjoint: one tree, four times"""
    fam = tg.compiled_families()
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
