"""The case table of tests/prepare_cases.py meets its conditions, the float64 restatement of the prepare kernel's algorithm
stays inside every rule that tests/test_prepare_gpu.py applies to the kernel (with the margins noted below), and the
image re-indexing helpers are bijections that round-trip.  No GPU."""
import numpy as np
import pytest

import prepare_cases as pc

IDS = [pc.run_id(r) for r in pc.RUNS]


def test_table_covers_every_edge():
    Ms = [c[0] for c in pc.CASES]
    assert Ms == [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97, 112, 113, 140, 141, 160, 161, 209, 257, 320]
    assert {1, 3, 4, 5, 8, 9, 16, 17, 21, 24} <= {c[1] for c in pc.CASES}
    assert {1, 4, 14, 15, 16} <= {c[2] for c in pc.CASES}
    lays = [pc.layout(*c) for c in pc.CASES]
    assert {l['DK'] for l in lays} == {2, 4, 6} and {l['JB'] for l in lays} == {1, 2}
    assert {l['NBLK'] for l in lays} == set(pc.NBLKS)
    # the ones row of ZT in the second JB block, and both sides of the LDS / global switch
    assert any(c[1] == 16 and pc.layout(*c)['JB'] == 2 for c in pc.CASES)
    assert any(l['work'][1] == 0 for l in lays) and any(l['work'][1] > 0 for l in lays)
    assert pc.layout(140, 21, 14)['work'][1] == 0 and pc.layout(141, 24, 16)['work'][1] == 141 * 141
    # every M except 1 has both sets
    assert len(pc.RUNS) == 2 * len(pc.CASES) - 1 and ((1, 1, 1), 'ill') not in pc.RUNS


def test_layout_restatement_matches_the_library():
    from cbfssm.hip import lib
    for M, D, Do in pc.CASES + ((33, 5, 4), (141, 6, 1), (140, 8, 4), (141, 9, 5)):
        mine, theirs = pc.layout(M, D, Do), lib.pack_layout(M, D, Do)
        for name in pc.SECTIONS:
            assert mine[name][0] == getattr(theirs, name), (M, D, Do, name)
        for name in ('total', 'M', 'D', 'Do', 'NBLK', 'DK', 'Mp', 'Dp', 'KS', 'JB'):
            assert mine[name] == getattr(theirs, name), (M, D, Do, name)
        # sections do not overlap and end inside the pack
        spans = sorted(mine[n] for n in pc.SECTIONS)
        for (o0, n0), (o1, _) in zip(spans, spans[1:]):
            assert o0 + n0 <= o1
        assert spans[-1][0] + spans[-1][1] <= mine['total']


@pytest.mark.parametrize('run', pc.RUNS, ids=IDS)
def test_parameter_sets_sit_in_their_condition_window(run):
    (M, D, Do), kind = run
    p = pc.params(M, D, Do, kind)
    cond = pc.condition(M, D, Do, kind)
    if kind == 'well':
        assert 1.0 <= cond <= pc.WELL_MAX < pc.REFINE_COND / 3.9
    else:
        assert pc.ILL_MIN <= cond <= pc.ILL_MAX and pc.ILL_MIN > pc.REFINE_COND
    assert p['jitter'] == 1e-8 and p['var'].shape == (1,) and 0.5 <= p['var'][0] <= 2.0
    if M * Do > 1:
        assert p['zvar'].min() == 1e-3 and p['zvar'].max() == 1.0                   # three decades
    if D > 1:
        assert len(set(p['ls'])) == D                                                # non-uniform per dimension
    if Do > 1:
        assert np.ptp(p['zmean'].mean(axis=0)) > 0.5
    assert np.all(p['zvar'] > 0) and np.all(p['ls'] > 0)


def test_zeta_var_spans_three_decades_along_the_table():
    lo = min(pc.params(*c, k)['zvar'].min() for c, k in pc.RUNS)
    hi = max(pc.params(*c, k)['zvar'].max() for c, k in pc.RUNS)
    assert hi / lo >= 1e3


@pytest.mark.parametrize('run', pc.RUNS, ids=IDS)
def test_restatement_stays_inside_every_rule(run):
    """Margins of the float64 restatement: the Cholesky backward bound at <= 0.25 of the rule, the right residual of the
    unrefined factor at <= 0.05, K^-1 = G G^T at <= 0.06; the refined factor at <= 0.5 of the 1.0 eps rule where the
    unrefined one, from M = 17 on, sits above 1.3 in the left residual -- which is what makes that rule a test of the
    Newton step."""
    (M, D, Do), kind = run
    p, e, r = pc.params(M, D, Do, kind), pc.emulate(M, D, Do, kind), pc.reference(M, D, Do, kind)
    ill = kind == 'ill'
    assert e['refined'] == ill
    A = e['Kmm'] + p['jitter'] * np.eye(M)
    got = pc.factor_ratios(M, e['L'], e['Linvt'], e['Kinv'], A, ill)
    assert got['L'] <= 0.25 and got['Kinv'] <= 0.06, got
    if ill:
        assert got['G_left'] <= 0.5 and got['G_right'] <= 0.5 and got['maxnorm'] <= 0.5, got
        before = pc.g_residuals(e['L'], e['G0'])
        if M >= 17:
            assert before['left'] >= 1.3, before
    else:
        assert got['G_right'] <= 0.05, got
    # the restatement against the longdouble reference: its own floors are finite, the scalars agree to what the
    # condition number allows, and the reference factor reproduces its matrix to longdouble rounding
    fl = pc.floors(M, D, Do, kind)
    assert all(np.isfinite(v) for v in fl.values())
    cond = e['cond']
    assert fl['Kmm'] <= 64 * pc.EPS * max(1.0, float(np.sum((p['Z'] / p['ls']) ** 2, axis=1).max()))
    assert fl['logdet'] <= 1e-12 * max(1.0, abs(float(r['logdet']))) + 4 * pc.EPS * cond         # a pivot: cond eps relative
    assert fl['klz'] <= 1e-12 * abs(float(r['klz'])) + 40 * pc.EPS * cond * abs(float(r['klz']))
    Ll = r['L']
    res = np.abs(Ll @ Ll.T - (r['Kmm'] + pc.LD(p['jitter']) * np.eye(M, dtype=pc.LD))).max()
    assert float(res) <= (M + 4) * float(np.finfo(pc.LD).eps) * float(np.abs(r['Kmm']).max()) * 4
    assert float(np.abs(r['W'] @ Ll - np.eye(M, dtype=pc.LD)).max()) <= 1e-4 * pc.EPS * cond


@pytest.mark.parametrize('case', pc.CASES, ids=['M%d-D%d-Do%d' % c for c in pc.CASES])
def test_image_helpers_round_trip(case):
    M, D, Do = case
    lay = pc.layout(M, D, Do)
    rng = np.random.default_rng(M)
    dense = dict(Bp=(M, M), Wp=(M, M), WTp=(M, M), Zp=(M, D), muA=(M, Do), s2A=(M, Do), muB=(M, Do), s2B=(M, Do),
                 ZT=(M, D + 1))
    for name, shape in dense.items():
        row, col, rows, cols = pc.image_map(name, lay)
        assert row.size == lay[name][1] == rows * cols                               # the image IS the padded matrix,
        assert np.unique(row * cols + col).size == rows * cols                       # every entry exactly once
        assert row.max() == rows - 1 and col.max() == cols - 1
        x = rng.standard_normal(shape)
        img = pc.to_image(name, lay, x)
        back = pc.from_image(name, lay, img)
        assert not np.isnan(back).any()
        assert np.array_equal(back[:shape[0], :shape[1]], x)
        back[:shape[0], :shape[1]] = 0.0
        assert not back.any()                                                        # padding is zero
        assert np.array_equal(pc.to_image(name, lay, pc.from_image(name, lay, img)), img)


def test_expected_images_place_the_ones_row_and_the_triangles():
    for M, D, Do in ((17, 8, 16), (32, 16, 4), (64, 24, 16)):
        lay = pc.layout(M, D, Do)
        p = pc.params(M, D, Do, 'well')
        e = pc.emulate(M, D, Do, 'well')
        img = pc.expected_images(lay, p, e)
        zt = pc.from_image('ZT', lay, img['ZT'])
        assert np.array_equal(zt[:M, D], np.ones(M)) and not zt[M:].any() and not zt[:, D + 1:].any()
        assert np.array_equal(zt[:M, :D], e['Zs'])
        w, wt = pc.from_image('Wp', lay, img['Wp']), pc.from_image('WTp', lay, img['WTp'])
        assert np.array_equal(w, wt.T) and not np.triu(w, 1).any()
        assert np.array_equal(w[:M, :M], e['Linvt'].T)


def test_failing_minor_matrices_fail_where_they_should():
    for M, ks in ((100, (1, 2, 32, 33, 64, 65)), (200, (141, 200))):
        for k in ks:
            A = pc.failing_minor(M, k)
            assert np.array_equal(A, A.T)
            _, piv, info = pc.eliminate(A)
            assert info == k and abs(piv[k - 1] + 1.0) <= 1e-12 and np.all(piv[:k - 1] > 0.5)
            assert pc.cholesky_ld(A)[1] == k
