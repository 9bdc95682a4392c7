"""prepare_kernel (csrc/cbfssm_api.hip) through ctypes at its own M edges: every section of the pack against the
np.longdouble reference, the componentwise bounds and the bitwise re-indexing rules of tests/prepare_cases.py, for a
well-conditioned set (no Newton step on G) and an ill-conditioned one (Newton step) per M; then the other entry points
that launch the same kernel -- cbfssm_gp_prepare2_f64, cbfssm_kmm_chol_f64, cbfssm_cholesky_f64 -- and cbfssm_rbf_k_f64.

The pack is an own buffer of layout.total + 64 doubles that starts as NaN with a sentinel tail: a section the kernel
does not fully write keeps a NaN, a write between or behind the sections disturbs a NaN gap or the tail.

Every rule prints achieved / rule before it is asserted (pytest -s shows the table of profiles/prepare/README.md)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import prepare_cases as pc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD, SENT = 64, -7.25e33
IDS = [pc.run_id(r) for r in pc.RUNS]
EPS = pc.EPS


def _lib():
    from cbfssm.hip import lib
    return lib, lib.load()


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64, order='C')).to(DEV)          # (a copy: the case arrays are read-only)


def _ptr(t):
    assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _fresh(n):
    buf = torch.full((n + GUARD,), float('nan'), dtype=torch.float64, device=DEV)
    buf[n:] = SENT
    return buf


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _inputs(p):
    return [_dev(p[k]) for k in ('Z', 'ls', 'var', 'zmean', 'zvar')]


def _prepare(M, D, Do, p, buf=None):
    """cbfssm_gp_prepare_f64 into `buf` (a fresh NaN buffer if None) -> (buffer on the device, library layout)"""
    lib, l = _lib()
    lay = lib.pack_layout(M, D, Do)
    if buf is None:
        buf = _fresh(lay.total)
    args = _inputs(p)
    lib.check(l.cbfssm_gp_prepare_f64(C.byref(lay), *[_ptr(a) for a in args], C.c_double(p['jitter']), _ptr(buf), _stream()),
              'gp_prepare')
    torch.cuda.synchronize()
    return buf, lay


@functools.lru_cache(maxsize=4)
def _single(M, D, Do, kind):
    """the pack of one single prepare into a fresh buffer, on the host (shared by the tests that compare against it)"""
    buf, _ = _prepare(M, D, Do, pc.params(M, D, Do, kind))
    out = buf.cpu().numpy()
    out.setflags(write=False)
    return out


def _section(host, lay, name, shape=None):
    o, n = lay[name]
    v = host[o:o + n]
    return v.reshape(shape) if shape else v


def _report(tag, **ratios):
    print('%-24s %s' % (tag, '  '.join('%s=%.3g' % kv for kv in ratios.items())))


# ---------------------------------------------------------------------------------------------------------------------
# every case, both parameter sets, through cbfssm_gp_prepare_f64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('run', pc.RUNS, ids=IDS)
def test_every_pack_section(run):
    (M, D, Do), kind = run
    ill = kind == 'ill'
    p, ref, fl = pc.params(M, D, Do, kind), pc.reference(M, D, Do, kind), pc.floors(M, D, Do, kind)
    lay = pc.layout(M, D, Do)
    buf, liblay = _prepare(M, D, Do, p)
    assert liblay.total == lay['total'] and all(getattr(liblay, n) == lay[n][0] for n in pc.SECTIONS)
    host = buf.cpu().numpy()
    tag = pc.run_id(run)

    exact = {}                                         # the rules without a tolerance: name -> holds

    # ---- whole pack: sentinel tail, no NaN in any section but `work`, the gaps between the sections untouched
    exact['sentinel tail'] = bool(np.all(host[lay['total']:] == SENT))
    covered = np.zeros(lay['total'], dtype=bool)
    for name in pc.SECTIONS:
        o, n = lay[name]
        covered[o:o + n] = True
        if name != 'work':
            exact['no NaN in ' + name] = not np.isnan(host[o:o + n]).any()
    exact['gaps untouched'] = bool(np.isnan(host[:lay['total']][~covered]).all())

    sec = {n: _section(host, lay, n, (M, M)) for n in ('Kmm', 'L', 'Kinv', 'Linvt')}
    sec['Zs'] = _section(host, lay, 'Zs', (M, D))
    scal = _section(host, lay, 'scal')
    Kmm, L, Kinv, G = sec['Kmm'], sec['L'], sec['Kinv'], sec['Linvt']

    # ---- Zs, invl: IEEE division, bit for bit
    exact['Zs bitwise'] = _same_bits(sec['Zs'], p['Z'] / p['ls'])
    invl = np.zeros(lay['Dp'])
    invl[:D] = 1.0 / p['ls']
    exact['invl bitwise'] = _same_bits(_section(host, lay, 'invl'), invl)

    # ---- Kmm against the longdouble K: per entry within max(1e-300, 20 x the CPU floor); symmetric; no jitter on the
    # diagonal (1e-8 is far above the tolerance)
    kerr = float(np.abs(Kmm.astype(pc.LD) - ref['Kmm']).max())
    ratios = dict(Kmm=kerr / pc.floor_tol(fl['Kmm']))
    exact['Kmm symmetric'] = np.array_equal(Kmm, Kmm.T)

    # ---- L, Linvt, Kinv
    exact['L upper zero'] = _same_bits(np.triu(L, 1), np.zeros((M, M)))
    exact['Linvt lower zero'] = _same_bits(np.tril(G, -1), np.zeros((M, M)))
    exact['Kinv symmetric'] = np.array_equal(Kinv, Kinv.T)
    ratios.update(pc.factor_ratios(M, L, G, Kinv, Kmm + p['jitter'] * np.eye(M), ill))

    # ---- scal
    exact['SIGMA2 bitwise'] = _same_bits(scal[pc.SIGMA2], p['var'][0])
    exact['JITTER bitwise'] = _same_bits(scal[pc.JIT], np.float64(p['jitter']))
    exact['INFO zero'] = scal[pc.INFO] == 0.0
    exact['scal 6..15 zero'] = _same_bits(scal[6:], np.zeros(pc.SCAL_COUNT - 6))
    cond = pc.cond_from(Kmm, Kinv, p['jitter'])
    ratios['cond'] = float(abs(pc.LD(scal[pc.COND]) - cond) / cond) / (4 * M * EPS)
    exact['branch'] = bool(scal[pc.COND] > pc.REFINE_COND) == ill                      # the branch the kernel took
    ratios['logdet'] = float(abs(pc.LD(scal[pc.LOGDET]) - ref['logdet'])) / pc.scalar_tol(fl['logdet'], ref['logdet'])
    ratios['klz'] = float(abs(pc.LD(scal[pc.KLZ]) - ref['klz'])) / pc.scalar_tol(fl['klz'], ref['klz'])

    # ---- images: bit for bit the re-indexed dense sections and inputs, padding exactly zero, ZT row D exactly one
    for name, want in pc.expected_images(lay, p, sec).items():
        exact[name + ' image bitwise'] = _same_bits(_section(host, lay, name), want)
    zt = pc.from_image('ZT', lay, _section(host, lay, 'ZT'))
    exact['ZT ones row'] = np.array_equal(zt[:M, D], np.ones(M)) and not zt[M:, D].any()
    cz = _section(host, lay, 'cz')
    exact['cz padding'] = bool(np.all(cz[M:] == -1e30))
    zs = sec['Zs'].astype(pc.LD)
    half, logv = pc.LD(0.5) * np.sum(zs * zs, axis=1), np.log(pc.LD(p['var'][0]))
    # (relative to the two terms, so that a row where they cancel is not asked for more than their rounding)
    ratios['cz'] = pc._ratio(np.abs(cz[:M].astype(pc.LD) - (logv - half)), 4 * EPS * (half + abs(logv)))
    _report(tag, **ratios)
    broken = [k for k, v in exact.items() if not v]
    if broken:
        print('%-24s NOT EXACT: %s' % (tag, ', '.join(broken)))
    assert not broken and all(v <= 1.0 for v in ratios.values()), (broken, ratios)

    # ---- a repeat call writes the same bits (the refinement's scratch in Kinv and Bp is rebuilt)
    _prepare(M, D, Do, p, buf)
    again = buf.cpu().numpy()
    assert _same_bits(again, host)

    # ---- ill first, then well, into one buffer: nothing of the first prepare survives
    if not ill and M > 1:
        both = _prepare(M, D, Do, pc.params(M, D, Do, 'ill'))[0]
        assert (both[lay['scal'][0] + pc.COND] > pc.REFINE_COND).item()
        _prepare(M, D, Do, p, both)
        assert _same_bits(both.cpu().numpy(), host)


# ---------------------------------------------------------------------------------------------------------------------
# cbfssm_gp_prepare2_f64: each pack bitwise what its single prepare writes
# ---------------------------------------------------------------------------------------------------------------------
PAIRS = (((33, 5, 4), (140, 21, 14)), ((141, 6, 1), (320, 24, 16)),
         ((140, 8, 4), (141, 9, 5)), ((141, 9, 5), (140, 8, 4)))      # the last two: exactly one M beyond the LDS form


@pytest.mark.parametrize('pair', PAIRS, ids=['%d+%d' % (a[0], b[0]) for a, b in PAIRS])
def test_prepare2_equals_two_single_prepares(pair):
    lib, l = _lib()
    kinds = ('well', 'ill')
    lays = [lib.pack_layout(*c) for c in pair]
    ps = [pc.params(*c, k) for c, k in zip(pair, kinds)]
    bufs = [_fresh(lay.total) for lay in lays]
    ins = [_inputs(p) for p in ps]
    args = []
    for lay, a, buf in zip(lays, ins, bufs):
        args += [C.byref(lay)] + [_ptr(x) for x in a] + [_ptr(buf)]
    lib.check(l.cbfssm_gp_prepare2_f64(*args, C.c_double(pc.JITTER), _stream()), 'gp_prepare2')
    torch.cuda.synchronize()
    for c, k, buf, lay in zip(pair, kinds, bufs, lays):
        got = buf.cpu().numpy()
        assert np.all(got[lay.total:] == SENT)
        assert (got[lay.scal + pc.COND] > pc.REFINE_COND) == (k == 'ill') and got[lay.scal + pc.INFO] == 0.0
        assert _same_bits(got, _single(*c, k)), (c, k)


# ---------------------------------------------------------------------------------------------------------------------
# cbfssm_kmm_chol_f64
# ---------------------------------------------------------------------------------------------------------------------
def _kmm_chol(Z, ls, var, jitter=pc.JITTER):
    lib, l = _lib()
    M, D = Z.shape
    nwork = M * D + M * (M + 1)
    Kmm, L, info, work = _fresh(M * M), _fresh(M * M), _fresh(1), _fresh(nwork)
    zd, ld, vd = _dev(Z), _dev(ls), _dev(var)
    lib.check(l.cbfssm_kmm_chol_f64(M, D, _ptr(zd), _ptr(ld), _ptr(vd), C.c_double(jitter), _ptr(Kmm), _ptr(L), _ptr(info),
                                    _ptr(work), _stream()), 'kmm_chol')
    torch.cuda.synchronize()
    out = []
    for t, n in ((Kmm, M * M), (L, M * M), (info, 1), (work, nwork)):
        h = t.cpu().numpy()
        assert np.all(h[n:] == SENT)
        out.append(h[:n])
    return out[0].reshape(M, M), out[1].reshape(M, M), out[2][0]


@pytest.mark.parametrize('case', ((32, 16, 4), (140, 21, 14), (141, 24, 16)), ids=lambda c: 'M%d' % c[0])
@pytest.mark.parametrize('kind', pc.KINDS)
def test_kmm_chol_equals_the_pack_sections(case, kind):
    M, D, Do = case
    p, lay = pc.params(M, D, Do, kind), pc.layout(M, D, Do)
    Kmm, L, info = _kmm_chol(p['Z'], p['ls'], p['var'])
    pack = _single(M, D, Do, kind)
    assert info == 0.0
    assert _same_bits(Kmm, _section(pack, lay, 'Kmm', (M, M)))
    assert _same_bits(L, _section(pack, lay, 'L', (M, M)))


@pytest.mark.parametrize('M', (17, 141))
@pytest.mark.parametrize('D', (25, 64))
def test_kmm_chol_beyond_the_pack_input_dimension(M, D):
    Z, ls, var = pc.kmm_inputs(M, D)
    ref = pc.kernel_ld(Z, Z, ls, var[0])
    floor = max(float(np.abs(pc.kernel_f64(Z, ls, var[0]) - ref).max()),
                float(np.abs(pc.kernel_f64(Z[:, ::-1], ls[::-1], var[0]) - ref).max()))
    Kmm, L, info = _kmm_chol(Z, ls, var)
    ratios = dict(Kmm=float(np.abs(Kmm.astype(pc.LD) - ref).max()) / pc.floor_tol(floor),
                  L=pc.chol_backward(L, Kmm + pc.JITTER * np.eye(M)))
    _report('kmm_chol M%d D%d' % (M, D), **ratios)
    assert info == 0.0 and np.array_equal(Kmm, Kmm.T) and not np.triu(L, 1).any()
    assert all(v <= 1.0 for v in ratios.values()), ratios


def test_kmm_chol_reports_the_row_of_a_nan():
    for (M, D), r in (((100, 5), 40), ((200, 9), 150), ((33, 3), 0), ((141, 4), 140)):
        Z, ls, var = pc.kmm_inputs(M, D)
        Z = Z.copy()
        Z[r, D // 2] = np.nan
        _, _, info = _kmm_chol(Z, ls, var)
        assert info == r + 1, (M, r, info)


# ---------------------------------------------------------------------------------------------------------------------
# cbfssm_cholesky_f64
# ---------------------------------------------------------------------------------------------------------------------
def _cholesky(A, jitter):
    lib, l = _lib()
    M = A.shape[0]
    L, info, work = _fresh(M * M), _fresh(1), _fresh(M * (M + 1))
    ad = _dev(A)
    lib.check(l.cbfssm_cholesky_f64(M, _ptr(ad), C.c_double(jitter), _ptr(L), _ptr(info), _ptr(work), _stream()), 'cholesky')
    torch.cuda.synchronize()
    Lh, ih, wh = L.cpu().numpy(), info.cpu().numpy(), work.cpu().numpy()
    assert np.all(Lh[M * M:] == SENT) and np.all(ih[1:] == SENT) and np.all(wh[M * (M + 1):] == SENT)
    return Lh[:M * M].reshape(M, M), ih[0]


@pytest.mark.parametrize('M', (1, 33, 140, 141, 320))
def test_cholesky_of_a_given_matrix(M):
    A = pc.spd_matrix(M)
    for jitter in (0.0, 1e-3):
        L, info = _cholesky(A, jitter)
        assert info == 0.0 and not np.isnan(L).any() and not np.triu(L, 1).any()
        ratio = pc.chol_backward(L, A + jitter * np.eye(M))
        _report('cholesky M%d j%g' % (M, jitter), L=ratio)
        assert ratio <= 1.0


@pytest.mark.parametrize('M,k', [(100, k) for k in (1, 2, 32, 33, 64, 65)] + [(200, 141), (200, 200)])
def test_cholesky_names_the_first_failing_minor(M, k):
    _, info = _cholesky(pc.failing_minor(M, k), 0.0)
    assert info == k


# ---------------------------------------------------------------------------------------------------------------------
# cbfssm_rbf_k_f64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', ((1, 1, 1), (17, 300, 64)), ids=lambda s: '%dx%dx%d' % s)
def test_rbf_k_against_longdouble(shape):
    lib, l = _lib()
    n, m, D = shape
    rng = np.random.default_rng(n + m + D)
    X, X2 = rng.uniform(-2.0, 2.0, (n, D)), rng.uniform(-2.0, 2.0, (m, D))
    ls = (1.5 + np.arange(D) / D + rng.uniform(0.0, 0.3, D)) * np.sqrt(D)
    var = np.array([1.37])
    ref = pc.kernel_ld(X, X2, ls, var[0])

    def f64(a, b, s):
        a, b = a / s, b / s
        return var[0] * np.exp(-0.5 * (-2.0 * (a @ b.T) + np.sum(a * a, axis=1)[:, None] + np.sum(b * b, axis=1)[None, :]))
    floor = max(float(np.abs(f64(X, X2, ls) - ref).max()), float(np.abs(f64(X[:, ::-1], X2[:, ::-1], ls[::-1]) - ref).max()))
    out = _fresh(n * m)
    xd, x2d, ld, vd = _dev(X), _dev(X2), _dev(ls), _dev(var)
    lib.check(l.cbfssm_rbf_k_f64(n, m, D, _ptr(xd), _ptr(x2d), _ptr(ld), _ptr(vd), _ptr(out), _stream()), 'rbf_k')
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[n * m:] == SENT)
    ratio = float(np.abs(got[:n * m].reshape(n, m).astype(pc.LD) - ref).max()) / pc.floor_tol(floor)
    _report('rbf_k %dx%dx%d' % shape, K=ratio)
    assert ratio <= 1.0
