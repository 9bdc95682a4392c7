"""Case table, np.longdouble reference and float64 CPU floor for the prepare kernel (csrc/cbfssm_api.hip, prepare_kernel).
No GPU and no library call in here: tests/test_prepare_cpu.py checks the table and the rules on the CPU,
tests/test_prepare_gpu.py runs the kernel against them.

The table walks the kernel's own M edges -- the 32-column panel, the 16-row MFMA tile, the switch of the working matrix
from LDS to global memory at M = 140 / 141 -- with D, Do varied along it.  Every M but 1 comes with two parameter sets:
  well  infinity-norm condition of K + jitter I  <= 1.9e6   (a quarter of the 7.5e6 refinement threshold: no Newton step)
  ill   condition in [3e7, 1e10]                            (clustered inducing inputs, long lengthscales: Newton step)
so the branch the kernel takes is unambiguous.  The lengthscale scale of a set is found by bisection on the condition
number and rounded to three digits.

Reference (np.longdouble): K from the reference's expansion -2 x.x' + |x|^2 + |x'|^2 on Z / ls (gp_tf.py:33-49), a column
Cholesky of K + jitter I (gp_tf.py:52-65), log det and the prior KL (gp_tf.py:163-172).
CPU floor: `emulate` restates the kernel's algorithm in float64 numpy -- unblocked bordered elimination of
[[K + jitter I, I], [I, .]], L and G = L^-T scaled by sqrt(piv) at the end, K^-1 = G G^T, one Newton step W <- W + W (I - L W)
with the residual in longdouble.  Its distance from the longdouble reference is the floor of a tensor."""
import functools

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
JITTER = 1e-8
REFINE_COND = 7.5e6
WELL_MAX = 1.9e6
ILL_MIN, ILL_MAX = 3e7, 1e10
NBLKS = (1, 2, 4, 7, 10, 13, 16, 20)
LDS_MAX_M = 140
SCAL_COUNT = 16
SIGMA2, LOGDET, KLZ, INFO, COND, JIT = 0, 1, 2, 3, 4, 5

#        M    D  Do
CASES = ((1, 1, 1), (2, 3, 4), (15, 4, 14), (16, 5, 15), (17, 8, 16), (31, 9, 1), (32, 16, 4), (33, 17, 14),
         (63, 21, 15), (64, 24, 16), (65, 3, 4), (97, 5, 1), (112, 16, 16), (113, 9, 15), (140, 21, 14), (141, 24, 16),
         (160, 4, 4), (161, 17, 1), (209, 8, 14), (257, 16, 15), (320, 24, 16))
KINDS = ('well', 'ill')
RUNS = tuple((c, k) for c in CASES for k in KINDS if not (c[0] == 1 and k == 'ill'))
_ILL_TARGETS = (6e7, 5e8, 4e9)


def run_id(run):
    (M, D, Do), kind = run
    return 'M%d-D%d-Do%d-%s' % (M, D, Do, kind)


# ---------------------------------------------------------------------------------------------------------------------
# layout of a pack (include/cbfssm_hip.h, restated) and the image index maps
# ---------------------------------------------------------------------------------------------------------------------
SECTIONS = ('Bp', 'Zp', 'cz', 'muA', 's2A', 'invl', 'scal', 'Kmm', 'L', 'Kinv', 'Linvt', 'Zs', 'muB', 's2B', 'ZT', 'work',
            'Wp', 'WTp')


def layout(M, D, Do):
    """offsets and sizes (in doubles) of the sections of a pack: {'name': (offset, size)}, plus the integer fields"""
    nblk = next(v for v in NBLKS if 16 * v >= M)
    dk = 2 if D <= 8 else (4 if D <= 16 else 6)
    mp, ks, jb = 16 * nblk, 4 * nblk, (4 * dk + 1 + 15) // 16
    sizes = dict(Bp=nblk * ks * 64, Zp=nblk * dk * 64, cz=mp, muA=nblk * 256, s2A=nblk * 256, invl=4 * dk, scal=SCAL_COUNT,
                 Kmm=M * M, L=M * M, Kinv=M * M, Linvt=M * M, Zs=M * D, muB=nblk * 256, s2B=nblk * 256, ZT=nblk * jb * 256,
                 work=M * (M | 1) if M > LDS_MAX_M else 0, Wp=nblk * ks * 64, WTp=nblk * ks * 64)
    out, o = {}, 0
    for name in SECTIONS:
        out[name] = (o, sizes[name])
        o += (sizes[name] + 63) // 64 * 64
    out.update(total=o, M=M, D=D, Do=Do, NBLK=nblk, DK=dk, Mp=mp, Dp=4 * dk, KS=ks, JB=jb)
    return out


def _amap(nblk, ksteps):
    """A-operand image [rb][s][64]: element i holds A[row 16 rb + (l & 15)][col 4 s + (l >> 4)]"""
    i = np.arange(nblk * ksteps * 64)
    l, s, rb = i & 63, (i >> 6) % ksteps, (i >> 6) // ksteps
    return 16 * rb + (l & 15), 4 * s + (l >> 4)


def _bmap(nblk):
    """B-operand image [rb][r][64] of muA / s2A: element i holds X[m = 16 rb + 4 r + (l >> 4)][d = l & 15]"""
    i = np.arange(nblk * 256)
    l, r, rb = i & 63, (i >> 6) & 3, i >> 8
    return 16 * rb + 4 * r + (l >> 4), l & 15


def _ztmap(nblk, jb):
    """ZT [rb][jb][s][64]: element i holds ZT[j = 16 jb + (l & 15)][m = 16 rb + 4 s + (l >> 4)], stored as (m, j) of Z~"""
    i = np.arange(nblk * jb * 256)
    l, s, b, rb = i & 63, (i >> 6) & 3, (i >> 8) % jb, (i >> 8) // jb
    return 16 * rb + 4 * s + (l >> 4), 16 * b + (l & 15)


def image_map(name, lay):
    """(row, col, rows, cols) of an image section: image[i] = padded[row[i], col[i]], padded of shape (rows, cols)"""
    nb, mp = lay['NBLK'], lay['Mp']
    if name in ('Bp', 'Wp', 'WTp'):
        return _amap(nb, lay['KS']) + (mp, mp)
    if name == 'Zp':
        return _amap(nb, lay['DK']) + (mp, lay['Dp'])
    if name in ('muA', 's2A'):
        return _bmap(nb) + (mp, 16)
    if name in ('muB', 's2B'):
        return _amap(nb, 4) + (mp, 16)
    if name == 'ZT':
        return _ztmap(nb, lay['JB']) + (mp, 16 * lay['JB'])
    raise KeyError(name)


def to_image(name, lay, dense, pad=0.0):
    """dense (r, c) -> the section's image; entries outside `dense` are `pad`"""
    row, col, rows, cols = image_map(name, lay)
    full = np.full((rows, cols), pad, dtype=np.float64)
    full[:dense.shape[0], :dense.shape[1]] = dense
    return full[row, col]


def from_image(name, lay, image):
    """the section's image -> padded dense (rows, cols); every padded entry is hit exactly once (see the CPU test)"""
    row, col, rows, cols = image_map(name, lay)
    full = np.full((rows, cols), np.nan)
    full[row, col] = image
    return full


def expected_images(lay, p, dense):
    """every image section from the inputs and the pack's own dense sections ({'Kinv', 'Linvt', 'Zs'}), bit for bit"""
    M, D = lay['M'], lay['D']
    G = dense['Linvt']
    zt = np.zeros((lay['Mp'], 16 * lay['JB']))
    zt[:M, :D] = dense['Zs']
    zt[:M, D] = 1.0
    return dict(Bp=to_image('Bp', lay, dense['Kinv']), Wp=to_image('Wp', lay, np.tril(G.T)), WTp=to_image('WTp', lay, np.triu(G)),
                Zp=to_image('Zp', lay, dense['Zs']), muA=to_image('muA', lay, p['zmean']), s2A=to_image('s2A', lay, p['zvar']),
                muB=to_image('muB', lay, p['zmean']), s2B=to_image('s2B', lay, p['zvar']), ZT=to_image('ZT', lay, zt))


# ---------------------------------------------------------------------------------------------------------------------
# parameter sets
# ---------------------------------------------------------------------------------------------------------------------
def kernel_f64(Z, ls, var):
    Zs = Z / ls
    Xs = np.sum(Zs * Zs, axis=1)
    return var * np.exp(-0.5 * (-2.0 * (Zs @ Zs.T) + (Xs[:, None] + Xs[None, :])))      # the kernel's order: symmetric


def cond_inf(K, jitter=JITTER):
    A = K + jitter * np.eye(K.shape[0])
    return float(np.abs(A).sum(axis=1).max() * np.abs(np.linalg.inv(A)).sum(axis=1).max())


def _round3(x):
    return float('%.3g' % x)


@functools.lru_cache(maxsize=None)
def params(M, D, Do, kind):
    """Z (M, D), ls (D), var (1), zmean (M, Do), zvar (M, Do): constrained values, float64"""
    idx = [c[0] for c in CASES].index(M) if M in [c[0] for c in CASES] else M
    rng = np.random.default_rng(1000 * M + 10 * D + (1 if kind == 'ill' else 0))
    shape = 0.7 + 0.6 * (np.arange(D) + rng.uniform(0.0, 0.5, D)) / max(D, 2)         # non-uniform per dimension
    if kind == 'well':
        Z = rng.uniform(-2.0, 2.0, (M, D))
        var = np.array([rng.uniform(0.5, 1.5)])
        target = 2e5
    else:
        Z = rng.uniform(-1.0, 1.0, D) + 0.3 * rng.standard_normal((M, D))            # one cluster
        var = np.array([2.0 if M == 2 else rng.uniform(0.5, 1.5)])
        target = min(_ILL_TARGETS[idx % 3], 0.3 * M * var[0] / JITTER)
    # cond grows with the lengthscale scale s (K -> var 1 1^T): bisection on log s, then three digits
    lo, hi = np.log(1e-2), np.log(1e4)
    if M > 1:
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            if cond_inf(kernel_f64(Z, np.exp(mid) * shape, var[0])) < target:
                lo = mid
            else:
                hi = mid
        s = _round3(np.exp(0.5 * (lo + hi)))
    else:
        s = 1.3
    ls = s * shape
    zmean = rng.standard_normal((M, Do)) * (1.0 + 0.3 * np.arange(Do)) + 0.5 * np.arange(Do) - 1.0
    zvar = 10.0 ** rng.uniform(-3.0, 0.0, (M, Do))                                    # three decades
    zvar.flat[0] = 1e-3
    zvar.flat[-1] = 1.0 if M * Do > 1 else 1e-3
    out = dict(Z=Z, ls=ls, var=var, zmean=zmean, zvar=zvar, jitter=JITTER)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def condition(M, D, Do, kind):
    p = params(M, D, Do, kind)
    return cond_inf(kernel_f64(p['Z'], p['ls'], p['var'][0]), p['jitter'])


# ---------------------------------------------------------------------------------------------------------------------
# np.longdouble reference
# ---------------------------------------------------------------------------------------------------------------------
def kernel_ld(X, X2, ls, var):
    a, b = X.astype(LD) / ls.astype(LD), X2.astype(LD) / ls.astype(LD)
    d2 = LD(-2) * (a @ b.T) + np.sum(a * a, axis=1)[:, None] + np.sum(b * b, axis=1)[None, :]
    return LD(var) * np.exp(LD(-0.5) * d2)


def cholesky_ld(A):
    """column Cholesky in longdouble; (L, info): info = first leading minor that is not positive definite, else 0"""
    A = A.astype(LD)
    M = A.shape[0]
    L = np.zeros((M, M), dtype=LD)
    for j in range(M):
        col = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not col[0] > 0:
            return L, j + 1
        L[j, j] = np.sqrt(col[0])
        L[j + 1:, j] = col[1:] / L[j, j]
    return L, 0


def lower_inverse_ld(L):
    M = L.shape[0]
    W = np.zeros((M, M), dtype=LD)
    for i in range(M):
        r = -(L[i, :i] @ W[:i, :])
        r[i] += LD(1)
        W[i, :] = r / L[i, i]
    return W


@functools.lru_cache(maxsize=None)
def reference(M, D, Do, kind):
    p = params(M, D, Do, kind)
    K = kernel_ld(p['Z'], p['Z'], p['ls'], p['var'][0])
    L, info = cholesky_ld(K + LD(p['jitter']) * np.eye(M, dtype=LD))
    assert info == 0
    W = lower_inverse_ld(L)
    logdet = LD(2) * np.sum(np.log(np.diag(L)))
    mu, s2 = p['zmean'].astype(LD), p['zvar'].astype(LD)
    kdiag = np.sum(W * W, axis=0)                                   # diag K^-1 = column norms of L^-1
    a = W @ mu
    kl = LD(0.5) * (np.sum(kdiag[:, None] * s2) + np.sum(a * a) - LD(M * Do) + LD(Do) * logdet - np.sum(np.log(s2)))
    out = dict(Kmm=K, L=L, W=W, logdet=logdet, klz=kl)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# float64 restatement of the kernel's algorithm
# ---------------------------------------------------------------------------------------------------------------------
def eliminate(A):
    """unblocked bordered elimination of [[A, I], [I, .]] in one M x M working matrix (lower + diagonal: A; strict upper: 0):
    -> (W, piv, info); column j of the lower part is L[:, j] sqrt(piv_j), row i of the strict upper part L^-T[i, :] sqrt(piv)"""
    M = A.shape[0]
    W = np.tril(A).astype(np.float64)
    piv = np.zeros(M)
    info = 0
    low = np.tril(np.ones((M, M), dtype=bool))
    with np.errstate(all='ignore'):
        for j in range(M):
            p = W[j, j]
            piv[j] = p
            if not p > 0.0 and info == 0:
                info = j + 1
            if j + 1 == M:
                break
            w = (1.0 / p) * W[j + 1:, j]
            c = W[:, j].copy()
            c[j] = 1.0
            upd = np.outer(c, w)
            upd[j + 1:] *= low[j + 1:, j + 1:]                       # a lower row is updated up to its diagonal only
            W[:, j + 1:] -= upd
    return W, piv, info


def scale_factor(W, piv):
    """L (lower) and G = L^-T (upper) from the working matrix"""
    sp = np.sqrt(piv)
    S = W / sp[None, :]
    L = np.tril(S, -1) + np.diag(sp)
    G = np.triu(S, 1) + np.diag(1.0 / sp)
    return L, G


def newton_step(L, G):
    """W <- W + W (I - L W), W = G^T, the residual accumulated in longdouble and rounded once"""
    Wm = G.T
    R = (np.eye(L.shape[0], dtype=LD) - L.astype(LD) @ Wm.astype(LD)).astype(np.float64)
    return (Wm + Wm @ np.tril(R)).T


@functools.lru_cache(maxsize=None)
def emulate(M, D, Do, kind):
    p = params(M, D, Do, kind)
    Zs = p['Z'] / p['ls']
    K = kernel_f64(p['Z'], p['ls'], p['var'][0])
    Wk, piv, info = eliminate(K + p['jitter'] * np.eye(M))
    assert info == 0
    L, G0 = scale_factor(Wk, piv)
    Kinv = G0 @ G0.T
    cond = (np.abs(K).sum(axis=1) + p['jitter']).max() * np.abs(Kinv).sum(axis=1).max()
    G = G0
    if cond > REFINE_COND:
        G = np.triu(newton_step(L, G0))
        Kinv = G @ G.T
    logdet = float(np.sum(np.log(piv)))
    mu, s2 = p['zmean'], p['zvar']
    kl = 0.5 * (np.sum(np.diag(Kinv)[:, None] * s2) + np.sum(mu * (Kinv @ mu)) - np.sum(np.log(s2)) + Do * (logdet - M))
    return dict(Zs=Zs, Kmm=K, L=L, G0=G0, Linvt=G, Kinv=Kinv, cond=float(cond), logdet=logdet, klz=float(kl),
                refined=bool(cond > REFINE_COND))


@functools.lru_cache(maxsize=None)
def floors(M, D, Do, kind):
    """largest distance of the float64 restatement from the longdouble reference, per tensor"""
    e, r = emulate(M, D, Do, kind), reference(M, D, Do, kind)
    p = params(M, D, Do, kind)
    rev = kernel_f64(p['Z'][:, ::-1], p['ls'][::-1], p['var'][0])     # the same expansion, the dimensions summed in reverse
    return dict(Kmm=float(max(np.abs(e['Kmm'] - r['Kmm']).max(), np.abs(rev - r['Kmm']).max())), logdet=float(abs(e['logdet'] - r['logdet'])),
                klz=float(abs(e['klz'] - r['klz'])))


def floor_tol(floor):
    return max(1e-300, 20.0 * floor)


def scalar_tol(floor, ref):
    return max(1e-12 * abs(float(ref)), 20.0 * floor)


# ---------------------------------------------------------------------------------------------------------------------
# rules: every one returns achieved / rule (<= 1 passes), products in longdouble
# ---------------------------------------------------------------------------------------------------------------------
def _ratio(err, bound):
    """max over entries of err / bound; an entry with bound 0 must have err 0"""
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    if np.any((bound == 0) & (err != 0)) or not np.all(np.isfinite(err)):
        return float('inf')
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def chol_backward(L, A):
    """|L L^T - A| <= (M + 4) eps |L||L|^T componentwise (Higham's bound for any summation order, plus the final scaling)"""
    Ll = L.astype(LD)
    M = L.shape[0]
    return _ratio(np.abs(Ll @ Ll.T - A.astype(LD)), LD((M + 4) * EPS) * (np.abs(Ll) @ np.abs(Ll).T))


def g_residuals(L, G):
    """W = G^T against L, componentwise and in units of eps: right = max |L W - I| / (eps |L||W|), left = max |W L - I| /
    (eps |W||L|); maxnorm = max|W L - I| / (4 eps max|W| max|L|), the suite's older rule"""
    Ll, Wl = L.astype(LD), G.T.astype(LD)
    I = np.eye(L.shape[0], dtype=LD)
    aL, aW = np.abs(Ll), np.abs(Wl)
    left = np.abs(Wl @ Ll - I)
    return dict(right=_ratio(np.abs(Ll @ Wl - I), LD(EPS) * (aL @ aW)), left=_ratio(left, LD(EPS) * (aW @ aL)),
                maxnorm=float(left.max() / (4 * EPS * aW.max() * aL.max())) if np.all(np.isfinite(left)) else float('inf'))


def kinv_product(Kinv, G):
    """|Kinv - G G^T| <= (M + 4) eps |G||G|^T componentwise, G G^T in longdouble from the given G"""
    Gl = G.astype(LD)
    M = G.shape[0]
    return _ratio(np.abs(Kinv.astype(LD) - Gl @ Gl.T), LD((M + 4) * EPS) * (np.abs(Gl) @ np.abs(Gl).T))


def cond_from(Kmm, Kinv, jitter):
    """row sums of |K| (+ jitter) and |K^-1| in longdouble"""
    a = np.abs(Kmm.astype(LD)).sum(axis=1) + LD(jitter)
    return a.max() * np.abs(Kinv.astype(LD)).sum(axis=1).max()


def factor_ratios(M, L, G, Kinv, A, ill):
    """achieved / rule of the factor sections of one pack (or of the restatement):
      L        |L L^T - A| <= (M + 4) eps |L||L|^T
      Kinv     |Kinv - G G^T| <= (M + 4) eps |G||G|^T
      well     G_right: |L W - I| <= (M + 4) eps |L||W|
      ill      G_left, G_right: |W L - I|, |L W - I| <= 1.0 eps |W||L|, |L||W| (a correctly rounded inverse gives 0.5; the
               factor 2 covers the Newton step's second-order terms), and the older max-norm rule"""
    g = g_residuals(L, G)
    out = dict(L=chol_backward(L, A), Kinv=kinv_product(Kinv, G))
    if ill:
        out.update(G_left=g['left'], G_right=g['right'], maxnorm=g['maxnorm'])
    else:
        out['G_right'] = g['right'] / (M + 4)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# inputs of the stand-alone entry points
# ---------------------------------------------------------------------------------------------------------------------
def spd_matrix(M, seed=0):
    """B B^T + I with a slowly decaying B: symmetric, safely positive definite"""
    rng = np.random.default_rng(7000 + 13 * M + seed)
    B = rng.standard_normal((M, M)) / np.sqrt(M)
    A = B @ B.T + np.eye(M)
    return 0.5 * (A + A.T)


def failing_minor(M, k, seed=0):
    """spd_matrix with mat[k-1, k-1] lowered so that the k-th pivot of the elimination is -1 (jitter 0)"""
    A = spd_matrix(M, seed).copy()
    L, _ = cholesky_ld(A[:k, :k])
    pk = float(L[k - 1, k - 1] ** 2)                                # the k-th pivot of the unchanged matrix
    A[k - 1, k - 1] -= pk + 1.0
    return A


def kmm_inputs(M, D, seed=0):
    """a well-conditioned (Z, ls, var) for D beyond the pack's 24"""
    rng = np.random.default_rng(9000 + 100 * M + D + seed)
    Z = rng.uniform(-2.0, 2.0, (M, D))
    ls = (1.5 + np.arange(D) / D + rng.uniform(0.0, 0.3, D)) * np.sqrt(D)
    return Z, ls, np.array([rng.uniform(0.5, 1.5)])
