"""Shared by the train-tail tests (csrc/cbfssm_tail.hip): the cases, the slab / image packers of the ABI, and a reference
that owes nothing to the kernel's algebra.

The reference is reverse-mode autodiff, on the CPU in float64, of ONE scalar per GP, built from the raw parameters through
softplus + 1e-10, the RBF kernel on Z / ls, cholesky(K + jitter I) and its inverse:

    F = <B, K^-1> + <C, Z/ls> - <glx, log ls> + gsig s^2 + glogsig log s^2 + <gMu, mu> + <gS2, zvar> + klw KL

with C = gZ[:, :D] - (Z/ls) o gZ[:, D] held constant and KL the prior KL of gp_tf.py:163-172 (diagonal q(z)), its
full-covariance form (sum_d S_d in place of diag(sum_d zvar), `fullq`), or PR-SSM's jitter-free prior (prssm.py:81-82,
`nojit`).  The noise terms <gvx, var_x> + <gvy + tail, var_y> are `noise_grads`.  It never forms T, G2, the trace identity
or Ws.  The cotangents B, gZ, gMu, ... are what a reduced adjoint slab carries (Slab<> in csrc/cbfssm_adjoint.hpp); B is
NOT symmetric, so that only a correct symmetrisation of the g_mode 1 / 2 images passes.

Conditioning: Z is uniform in [-3, 3]^D and lengthscales_unc = lsv + U(0, 0.2) with lsv chosen per case so that
cond_2(K + jitter I) lies in the case's window (1e1 .. 1e4; one deliberately ill-conditioned case at 1e5 .. 1e7): with
K ~ I the Hadamard product with K_mm would switch the whole RBF chain off.

Float64 floor of a case and tensor (`floors`): |train._gp_adjoint on CPU tensors - this reference| / max|reference|, with a
stand-in pack whose Kinv, Kmm, Zs and jitter come from the reference (Kinv: its K + jitter I inverted by a second float64
route, `second_inverse`) -- what a correct float64 evaluation of the tail's formulation loses, not a number that comes from
the kernel under test.  The GPU tolerance is max(1e-12, 20 x floor)."""
import collections
import ctypes as C
import functools

import numpy as np
import torch

JITTER = 1e-8
GP_PARAMS = ('zeta_pos', 'zeta_mean', 'zeta_var_unc', 'variance_unc', 'lengthscales_unc')
TILE_HEIGHTS = (1, 2, 4, 7, 10, 13, 16, 20)        # row blocks; layout.NBLK is the tile height, not ceil(M / 16)
TOL_FACTOR, TOL_MIN = 20.0, 1e-12

Case = collections.namedtuple('Case', 'M D Do lsv cond_lo cond_hi')

# The smallest M at which each index rule changes (1; 16 | 17; 33: four-block tile with an empty block; 48 | 49: the
# max(M, 48) scratch edge; 112: last size with the matrix section in the slab; 113: first stash size; 161: first g_mode 2
# height; 208 | 209; 320), across D in {1, 9, 16, 17, 24, 32} (two / four / six k-steps of the input dimension and the
# second column tile of tail_gemm<2>) and Do in {1, 7, 16}.  No pack layout exists above D = 24 (cbfssm_gp_pack_layout), so the
# D = 32 rows have no slab and are skipped: the tail's own limit of D <= 32 cannot be reached through the ABI.
CASES = [
    Case(1, 1, 1, 1.0, 1.0, 1.0),                  # K_mm is the scalar s^2: the window is cond = 1
    Case(16, 1, 1, -2.5, 1e1, 1e4),
    Case(16, 9, 7, 4.5, 1e1, 1e4),
    Case(17, 16, 16, 6.0, 1e1, 1e4),
    Case(33, 17, 7, 5.5, 1e1, 1e4),
    Case(48, 24, 16, 6.5, 1e1, 1e4),
    Case(49, 9, 1, 3.3, 1e1, 1e4),
    Case(49, 32, 16, 5.5, 1e1, 1e4),
    Case(112, 24, 7, 5.6, 1e1, 1e4),
    Case(113, 9, 7, 2.8, 1e1, 1e4),
    Case(161, 17, 16, 4.3, 1e1, 1e4),
    Case(208, 16, 1, 3.8, 1e1, 1e4),
    Case(208, 32, 7, 5.5, 1e1, 1e4),
    Case(209, 24, 16, 5.2, 1e1, 1e4),
    Case(320, 9, 16, 2.4, 1e1, 1e4),
    Case(320, 17, 7, 3.9, 1e1, 1e4),
    Case(100, 9, 7, 12.0, 1e5, 1e7),                # ill-conditioned: the jitter terms carry a visible share of g_var
]


def case_id(c):
    return 'M%d-D%d-Do%d' % (c.M, c.D, c.Do)


def layout_of(M, D, Do):
    """the library's pack layout (host arithmetic), or None where it has none or no adjoint slab for it"""
    from cbfssm.hip import lib as _l
    lay = _l.PackLayout()
    if _l.load().cbfssm_gp_pack_layout(int(M), int(D), int(Do), C.byref(lay)) != 0 or lay.rev_slab <= 0:
        return None
    return lay


def runnable():
    return [c for c in CASES if layout_of(c.M, c.D, c.Do) is not None]


def two_gp(c):
    """the two-GP model (cbfssm_train_tail_f64 / _g_f64) takes the case as gp_f: dim_x = Do, dim_u = D - Do >= 0, and gp_b needs
    an unobserved state dimension"""
    return c.D >= c.Do >= 2


def g_mode_of(lay):
    """what the float32 adjoint leaves at this tile height: the full G below 13 row blocks, G + G^T's lower blocks from there"""
    return 2 if lay.NBLK >= 13 else 1


# ---- the layouts the ABI takes ---------------------------------------------------------------------------------------
def pack_c(dense, nrb, ncb):
    """dense (16 nrb, 16 ncb) -> MFMA accumulator image [rb][cb][r][lane]: the inverse of train._unpack_c"""
    assert dense.shape == (16 * nrb, 16 * ncb)
    return dense.reshape(nrb, 4, 4, ncb, 16).permute(0, 3, 1, 2, 4).reshape(-1).contiguous()


def pad_nan(a, rows, cols):
    out = torch.full((rows, cols), float('nan'), dtype=torch.float64)
    out[:a.shape[0], :a.shape[1]] = a
    return out


def matrix_image(mat, nblk, mode=0):
    """C-layout image [NBLK][NBLK][4][64] of an (M, M) matrix, NaN in every padding element.  mode 2: the lower-triangular
    16 x 16 blocks of mat + mat^T with the diagonal blocks of mat itself, and NaN in the whole upper block triangle"""
    M = mat.shape[0]
    if mode == 2:
        blk = torch.arange(M) // 16
        low, dia = blk[:, None] > blk[None, :], blk[:, None] == blk[None, :]
        nan = torch.full_like(mat, float('nan'))
        mat = torch.where(low, mat + mat.T, torch.where(dia, mat, nan))
    return pack_c(pad_nan(mat, 16 * nblk, 16 * nblk), nblk, nblk)


def dense_ld(mat, ld):
    """(M, M) -> row-major [M][ld] with NaN behind every row"""
    return pad_nan(mat, mat.shape[0], ld).reshape(-1).contiguous()


def slab_offsets(lay, with_matrix):
    nb, jb = lay.NBLK, lay.JB
    o = {'gMu': 0, 'gS2': nb * 256, 'gB': 2 * nb * 256}
    o['gZ'] = o['gB'] + (nb * nb * 256 if with_matrix else 0)
    o['small'] = o['gZ'] + nb * jb * 256
    o['end'] = o['small'] + 192
    return o


def pack_slab(t, lay, matrix=None, with_matrix=None):
    """the reduced slab of one GP, layout->rev_slab doubles (Slab<> in csrc/cbfssm_adjoint.hpp):
    [gMu | gS2 | matrix section (absent at the stash tile heights) | gZ, D + 1 columns | small], NaN wherever the tail has no
    business reading.  matrix: the section's image (matrix_image), needed exactly where the slab has the section"""
    nb, jb, M, D, Do = lay.NBLK, lay.JB, lay.M, lay.D, lay.Do
    with_matrix = (not lay.rev_stash) if with_matrix is None else with_matrix
    o = slab_offsets(lay, with_matrix)
    assert o['end'] <= lay.rev_slab and with_matrix == (not lay.rev_stash)
    slab = torch.full((int(lay.rev_slab),), float('nan'), dtype=torch.float64)
    slab[o['gMu']:o['gS2']] = pack_c(pad_nan(t['gMu'], 16 * nb, 16), nb, 1)
    slab[o['gS2']:o['gB']] = pack_c(pad_nan(t['gS2'], 16 * nb, 16), nb, 1)
    if with_matrix:
        assert matrix is not None and matrix.numel() == nb * nb * 256
        slab[o['gB']:o['gZ']] = matrix
    else:
        assert matrix is None
    slab[o['gZ']:o['small']] = pack_c(pad_nan(t['gZ'], 16 * nb, 16 * jb), nb, jb)
    s = o['small']
    slab[s:s + Do] = t['gvx']
    slab[s + 16:s + 16 + Do] = t['gvy']
    slab[s + 32:s + 32 + D] = t['glx']
    slab[s + 96], slab[s + 97] = t['gsig'], t['glogsig']
    return slab


def unpack_slab(slab, lay, with_matrix=None):
    """the inverse of pack_slab on the real entries (train._unpack_c for the images); matrix: the section's (M, M) or None"""
    from cbfssm.hip.train import _unpack_c
    nb, jb, M, D, Do = lay.NBLK, lay.JB, lay.M, lay.D, lay.Do
    with_matrix = (not lay.rev_stash) if with_matrix is None else with_matrix
    o = slab_offsets(lay, with_matrix)
    s = o['small']
    out = {'gMu': _unpack_c(slab[o['gMu']:o['gS2']], nb, 1)[:M, :Do], 'gS2': _unpack_c(slab[o['gS2']:o['gB']], nb, 1)[:M, :Do],
           'gZ': _unpack_c(slab[o['gZ']:o['small']], nb, jb)[:M, :D + 1], 'gvx': slab[s:s + Do], 'gvy': slab[s + 16:s + 16 + Do],
           'glx': slab[s + 32:s + 32 + D], 'gsig': slab[s + 96], 'glogsig': slab[s + 97],
           'matrix': _unpack_c(slab[o['gB']:o['gZ']], nb, nb)[:M, :M] if with_matrix else None}
    return out


def tail_block(t, dim_y):
    """[loglik, kl_x, entropy, d loss / d var_y [dim_y]]: the tail reads the last dim_y entries only"""
    return torch.cat([torch.full((3,), float('nan'), dtype=torch.float64), t['tail_vy'][:dim_y]])


# ---- inputs ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def build(M, D, Do, lsv, seed=0, shared=False):
    """raw parameters and cotangents of one GP, drawn in this order (torch float64 on the CPU).  shared: PR-SSM's one
    lengthscale for all input dimensions (prssm.py:40): the first entry of lengthscales_unc, D times"""
    rng = np.random.default_rng(100000 * seed + 1000 * M + 10 * D + Do)
    f = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    t = {'zeta_pos': f(rng.uniform(-3.0, 3.0, (M, D))),
         'zeta_mean': f(0.5 * rng.standard_normal((M, Do))),
         'zeta_var_unc': f(rng.uniform(-3.0, -1.0, (M, Do))),
         'variance_unc': f(rng.uniform(-0.5, 0.5, (1,))),
         'lengthscales_unc': f(lsv + rng.uniform(0.0, 0.2, (D,))),
         'var_x_unc': f(rng.uniform(-3.0, -1.0, (Do,))),
         'var_y_unc': f(rng.uniform(-2.0, 0.0, (Do,))),
         'gMu': f(rng.standard_normal((M, Do))),
         'gS2': f(rng.standard_normal((M, Do))),
         'B': f(rng.standard_normal((M, M)) / np.sqrt(M)),
         'gZ': f(rng.standard_normal((M, D + 1))),
         'gvx': f(rng.standard_normal(Do)), 'gvy': f(rng.standard_normal(Do)), 'glx': f(rng.standard_normal(D)),
         'gsig': f(rng.standard_normal()), 'glogsig': f(rng.standard_normal()),
         'tail_vy': f(rng.standard_normal(Do))}
    q = np.tril(0.3 * rng.standard_normal((Do, M, M)) / np.sqrt(M), -1)
    q[:, np.arange(M), np.arange(M)] = rng.uniform(0.2, 0.5, (Do, M))
    t['q_sqrt'] = f(q)
    t['Ssum'] = torch.einsum('dij,dkj->ik', t['q_sqrt'], t['q_sqrt'])
    if shared:
        t['lengthscales_unc'] = t['lengthscales_unc'][:1].expand(D).clone()
    return t


def build_case(c, seed=0, shared=False):
    return build(c.M, c.D, c.Do, c.lsv, seed, shared)


# ---- the reference ---------------------------------------------------------------------------------------------------
def _sp(x):
    return torch.nn.functional.softplus(x) + 1e-10


def kernel_parts(th):
    """ls, s^2, zvar, Z / ls, K_mm (without jitter) from the raw parameters (tf_transform.py:19-21, gp_tf.py:33-49).
    The squared distance is the model's own expression, -2 x.x' + |x|^2 + |x'|^2 without a clamp (gp_tf.py:33-38), which is
    the function the train step differentiates and what the library's prepare evaluates.  It is not the same float64 number as
    sum (x - x')^2: the two differ by eps |z~|^2, which K^-1 multiplies by cond -- 1e-11 of every gradient tensor at M16-D1-Do1
    (lengthscale 0.08, |z~| up to 37, cond 1.8e3; measured on the GPU against the difference form), below 3 eps cond in every
    other case (|z~| <= 1.3).  The tail takes K_mm, K^-1 and z~ from the pack; how K_mm is rounded is not its business."""
    ls, var, zvar = _sp(th['lengthscales_unc']), _sp(th['variance_unc']), _sp(th['zeta_var_unc'])
    Zs = th['zeta_pos'] / ls
    Xs = (Zs * Zs).sum(1)
    K = var * torch.exp(-0.5 * (-2.0 * (Zs @ Zs.T) + Xs[:, None] + Xs[None, :]))
    return ls, var, zvar, Zs, K


def objective(t, th, klw=1.0, kl='jitter', data=True, Cz=None):
    """F of the module docstring for one GP.  kl: 'jitter' (gp_tf.py:163-172), 'nojit' (prssm.py:81-82) or 'fullq'.
    Cz: the constant C, for callers that move the parameters (finite differences); None: C at th itself, detached"""
    ls, var, zvar, Zs, K = kernel_parts(th)
    mu = th['zeta_mean']
    M, Do = mu.shape
    D = Zs.shape[1]
    L = torch.linalg.cholesky(K + JITTER * torch.eye(M, dtype=torch.float64))
    Kinv = torch.cholesky_inverse(L)
    F = torch.zeros((), dtype=torch.float64)
    if data:
        if Cz is None:
            Cz = t['gZ'][:, :D] - Zs.detach() * t['gZ'][:, D:]
        F = F + (t['B'] * Kinv).sum() + (Cz * Zs).sum() - (t['glx'] * torch.log(ls)).sum() + t['gsig'] * var.sum() \
            + t['glogsig'] * torch.log(var).sum() + (t['gMu'] * mu).sum()
        if kl != 'fullq':                                   # (full q(z): the factors' adjoint is not the tail's)
            F = F + (t['gS2'] * zvar).sum()
    if klw != 0.0:
        if kl == 'nojit':
            Lk = torch.linalg.cholesky(K)
            Kk = torch.cholesky_inverse(Lk)
        else:
            Lk, Kk = L, Kinv
        logdet = 2.0 * torch.log(torch.diagonal(Lk)).sum()
        quad = (mu * (Kk @ mu)).sum()
        if kl == 'fullq':
            tr = (Kk * t['Ssum']).sum()
            ent = 2.0 * torch.log(torch.diagonal(t['q_sqrt'], dim1=1, dim2=2)).sum()
        else:
            tr = (torch.diagonal(Kk) * zvar.sum(1)).sum()
            ent = torch.log(zvar).sum()
        F = F + klw * 0.5 * (tr + quad - M * Do + Do * logdet - ent)
    return F


def leaves(t, grad=True):
    return {k: t[k].clone().requires_grad_(grad) for k in GP_PARAMS}


Ref = collections.namedtuple('Ref', 'cond K Kinv Zs parts')


@functools.lru_cache(maxsize=None)
def reference(M, D, Do, lsv, seed=0, shared=False):
    """cond_2(K + jitter I), the reference's own K_mm / K^-1 / Z/ls, and the gradient of each linear part of F:
    parts['data' | 'jitter' | 'nojit' | 'fullq'][name], so that d F / d theta = data + klw * <kl part>"""
    t = build(M, D, Do, lsv, seed, shared)
    parts = {}
    for key, kw in (('data', dict(klw=0.0)), ('jitter', dict(data=False)), ('nojit', dict(data=False, kl='nojit')),
                    ('fullq', dict(data=False, kl='fullq'))):
        th = leaves(t)
        g = torch.autograd.grad(objective(t, th, **kw), [th[k] for k in GP_PARAMS], allow_unused=True)
        parts[key] = {k: (torch.zeros_like(t[k]) if gi is None else gi) for k, gi in zip(GP_PARAMS, g)}
    with torch.no_grad():
        ls, var, zvar, Zs, K = kernel_parts(leaves(t, False))
        Kj = K + JITTER * torch.eye(M, dtype=torch.float64)
        Kinv = torch.cholesky_inverse(torch.linalg.cholesky(Kj))
        cond = float(torch.linalg.cond(Kj))
    return Ref(cond, K, Kinv, Zs, parts)


def reference_case(c, seed=0, shared=False):
    return reference(c.M, c.D, c.Do, c.lsv, seed, shared)


def expected(ref, t, klw=1.0, kl='jitter', data=True, shared=False):
    """d F / d (the five raw tensors) for one entry point's switches.  shared: the one lengthscale's gradient, the sum over
    the input dimensions of those of its D copies"""
    out = {}
    for k in GP_PARAMS:
        g = klw * ref.parts[kl][k]
        if data:
            g = g + ref.parts['data'][k]
        if kl == 'fullq' and k == 'zeta_var_unc':
            g = torch.zeros_like(g)
        if shared and k == 'lengthscales_unc':
            g = g.sum().reshape(1)
        out[k] = g
    return out


def noise_grads(gvx, gvy, vx_unc, vy_unc):
    """d (<gvx, var_x> + <gvy, var_y>) / d (var_x_unc, var_y_unc) through softplus + 1e-10"""
    a, b = vx_unc.clone().requires_grad_(), vy_unc.clone().requires_grad_()
    ga, gb = torch.autograd.grad((gvx * _sp(a)).sum() + (gvy * _sp(b)).sum(), [a, b])
    return ga, gb


def g_image_matrix(ref, t):
    """what g_mode 1 / 2 hand the tail: G = K^-1 B K^-1 from the reference's own inverse"""
    return ref.Kinv @ t['B'] @ ref.Kinv


# ---- the float64 floor of the tail's formulation ---------------------------------------------------------------------
class StandInPack:
    """what train._gp_adjoint reads of a GPPack, filled from the reference"""

    def __init__(self, lay, Kmm, Kinv, Zs, jitter):
        from cbfssm.hip import lib as _l
        self.layout, self.M, self.D = lay, lay.M, lay.D
        self.Kmm, self.Kinv, self._Zs = Kmm, Kinv, Zs
        self.scal = torch.zeros(_l.SCAL_COUNT, dtype=torch.float64)
        self.scal[_l.SCAL_JITTER] = jitter

    def section(self, name, shape):
        assert name == 'Zs'
        return self._Zs.reshape(shape)


def second_inverse(Kj):
    """(K + jitter I)^-1 by LU with partial pivoting: a second correct float64 route to the inverse, with a factorisation of
    its own.  An evaluation of the tail's formulation starts from K_mm and inverts it itself (the library's prepare does), so
    the stand-in's K^-1 is the reference's matrix inverted again, not the bits autodiff saw: with those the floor of zeta_mean
    (gMu + K^-1 mu) would be an exact 0 and its tolerance 1e-12 at any cond, which no second inversion, good to about cond eps,
    can meet.  (A second route through the SAME Cholesky factor, L^-T L^-1 by triangular solves, agrees with cholesky_inverse to
    1e-15 at cond 1e6: it shares the rounding of L and says nothing about it.)"""
    return torch.linalg.inv(Kj)


@functools.lru_cache(maxsize=None)
def floors(M, D, Do, lsv, seed=0, shared=False):
    """{name: floor} over the two priors _gp_adjoint knows (jitter, nojit), each |restatement - reference| / max|reference|"""
    from cbfssm.hip.train import _gp_adjoint, gp_unc_grads
    t, ref, lay = build(M, D, Do, lsv, seed, shared), reference(M, D, Do, lsv, seed, shared), layout_of(M, D, Do)
    raw = {k: t[k] for k in GP_PARAMS}
    if shared:
        raw['lengthscales_unc'] = raw['lengthscales_unc'][:1]
    with torch.no_grad():
        ls, var, zvar, Zs, K = kernel_parts(leaves(t, False))
        pack = StandInPack(lay, ref.K, second_inverse(ref.K + JITTER * torch.eye(M, dtype=torch.float64)), ref.Zs, JITTER)
        klpack = StandInPack(lay, ref.K, second_inverse(ref.K), ref.Zs, 0.0)
        img = matrix_image(t['B'], lay.NBLK)
        slab = pack_slab(t, lay, None if lay.rev_stash else img)
        out = {k: 0.0 for k in GP_PARAMS}
        for kl, kp in (('jitter', None), ('nojit', klpack)):
            gz, gmu, gs2, gvar, gls, _ = _gp_adjoint(pack, slab, t['zeta_pos'], ls, var, t['zeta_mean'], zvar, Do,
                                                     not lay.rev_stash, img if lay.rev_stash else None, kp)
            got = gp_unc_grads('', raw, gz, gmu, gs2, gvar, gls, shared_ls=shared)
            want = expected(ref, t, 1.0, kl, shared=shared)
            for k in GP_PARAMS:
                out[k] = max(out[k], rel_err(got[k], want[k]))
    return out


def floors_case(c, seed=0, shared=False):
    return floors(c.M, c.D, c.Do, c.lsv, seed, shared)


def rel_err(got, want):
    """max |got - want| / max |want|; a reference that is zero everywhere asks for exact zeros"""
    got, want = torch.as_tensor(got).reshape(-1), torch.as_tensor(want).reshape(-1)
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    if not (err == err):
        return float('inf')
    if scale == 0.0:
        return 0.0 if err == 0.0 else float('inf')
    return err / scale


def tolerance(floor):
    return max(TOL_MIN, TOL_FACTOR * floor)
