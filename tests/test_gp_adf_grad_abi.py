"""Host-side checks of the entry points of the input adjoint of GPModel.adf (no GPU): the two symbols are declared, exported
and bound with the documented order of arguments, the count is 64-bit and what the header says at every tile height, and bad
arguments are refused on the host before anything is launched -- with the output buffers untouched.  The limits are those of
cbfssm_gp_adf_f64."""
import ctypes as C
import os
import re

from cbfssm.hip import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT, CALL = 'cbfssm_gp_adf_bwd_work_elems', 'cbfssm_gp_adf_bwd_f64'
SENTINEL = -7.25
ORDER = ['pack', 'm0', 'P0', 'a', 'y', 'cond', 'var_x', 'var_y', 'Dy', 'means', 'covs', 'pmeans', 'pcovs', 'info', 'gmeans',
         'gcovs', 'gloglik', 'N', 'T', 'gm0', 'gP0', 'ga', 'gy', 'gvar_x', 'gvar_y', 'work', 'stream']
OUT = ('gm0', 'gP0', 'ga', 'gy', 'gvar_x', 'gvar_y', 'work')
REQUIRED = ('pack', 'm0', 'a', 'y', 'var_y', 'means', 'covs', 'pmeans', 'pcovs', 'info', 'gm0', 'ga', 'gy', 'gvar_y', 'work')


def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, 'include', 'cbfssm_hip.h')).read()
    declared = set(re.findall(r'\b(cbfssm_[a-z0-9_]+)\s*\(', text))
    so = C.CDLL(lib.LIB_PATH)
    for name in (COUNT, CALL):
        assert name in declared and name in lib.SYMBOLS and hasattr(so, name), name
    l = lib.load()
    fn, count = getattr(l, CALL), getattr(l, COUNT)
    assert fn.restype is C.c_int and count.restype is C.c_int64 and len(count.argtypes) == 2
    assert len(fn.argtypes) == 1 + len(ORDER) == 28
    ints = {1 + ORDER.index('Dy'): C.c_int, 1 + ORDER.index('N'): C.c_int64, 1 + ORDER.index('T'): C.c_int64}
    assert all(t is ints.get(i, C.c_void_p) for i, t in enumerate(fn.argtypes) if i)
    decl = re.search(r'int %s\(([^;]*)\);' % CALL, text).group(1)
    assert [re.findall(r'\w+', part)[-1] for part in decl.split(',')] == ['layout'] + ORDER
    # the count's declaration says which reference call sites the pair stands for
    assert re.search(r'%s\([^;]*;\s*/\* gp_tf\.py:132-161, cbfssm\.py:199-221 \*/' % COUNT, text)


def _waves(nblk):
    return (nblk + 1) // 2 if nblk > 7 else nblk


def test_the_count_is_64_bit_sized_by_the_launch_and_refuses_a_bad_layout():
    l = lib.load()
    count = getattr(l, COUNT)
    shapes = (((1, 1, 1), 1), ((24, 8, 8), 2), ((50, 9, 2), 4), ((100, 21, 14), 7), ((113, 9, 1), 10), ((180, 12, 3), 13),
              ((250, 12, 6), 16), ((320, 24, 16), 20))
    for (M, D, Do), nblk in shapes:
        lay = lib.pack_layout(M, D, Do)
        assert lay.NBLK == nblk
        dp, mp, lt = 4 * lay.DK, 16 * nblk, 16 * lay.DK * lay.DK
        fwd = 16 * 16 * nblk + Do * nblk * nblk * 256
        # per workgroup: the chain phase's scratch (cbfssm_gp_moment_match_bwd_work_elems' per workgroup), the staged x, S,
        # gfmean, gfcov, gxcov, the results gmean, gcov, the lanes' rows of Pb- and entries of mb-, and the 32 variance sums
        point = _waves(nblk) * lt + (nblk // 2 + 1) * mp + 4 * 16 * dp + 7 * lt + 4 * dp
        block = 2 * point + 2 * (16 * dp + 16 * lt) + 256 + 4096 + 256 * dp + 4096 + 256 + 32
        assert count(C.byref(lay), 0) == fwd == l.cbfssm_gp_adf_work_elems(C.byref(lay))
        for N, groups in ((1, 1), (16, 1), (17, 2), (5120, 320)):
            assert count(C.byref(lay), N) == fwd + groups * block, (M, N)
    big = lib.pack_layout(320, 24, 16)
    assert count(C.byref(big), 2 ** 30) > 2 ** 41                   # 64-bit arithmetic: no wrap at 32 bits
    good = lib.pack_layout(100, 21, 14)
    assert count(None, 1) == -1 and count(C.byref(good), -1) == -1
    for field, value in (('M', 0), ('M', 321), ('D', 25), ('Do', 17), ('NBLK', 3), ('D', 13)):         # (D = 13 < Do = 14)
        lay = lib.pack_layout(100, 21, 14)
        setattr(lay, field, value)
        assert count(C.byref(lay), 16) == -1, (field, value)


class _Buffers:
    """host arrays behind every pointer of the call, filled with a sentinel"""

    def __init__(self, Do=14, Dy=7, N=3, T=2, Da=7):
        mat, vec = T * N * Do * Do, T * N * Do
        sizes = {'pack': 4, 'm0': N * Do, 'P0': N * Do * Do, 'a': T * N * Da, 'y': T * N * Dy, 'cond': T * N, 'var_x': Do,
                 'var_y': Dy, 'means': vec, 'covs': mat, 'pmeans': vec, 'pcovs': mat, 'info': N, 'gmeans': vec, 'gcovs': mat,
                 'gloglik': N, 'gm0': N * Do, 'gP0': N * Do * Do, 'ga': T * N * Da, 'gy': T * N * Dy, 'gvar_x': Do,
                 'gvar_y': Dy, 'work': 16}
        self.arr = {k: (C.c_double * max(n, 1))(*([SENTINEL] * max(n, 1))) for k, n in sizes.items()}
        self.Dy, self.N, self.T = Dy, N, T

    def args(self, null=(), **over):
        p = {k: (None if k in null else C.cast(v, C.c_void_p)) for k, v in self.arr.items()}
        p.update(Dy=self.Dy, N=self.N, T=self.T, stream=None)
        p.update(over)
        return [p[k] for k in ORDER]

    def untouched(self):
        return all(x == SENTINEL for k in OUT for x in self.arr[k])


def test_the_adjoint_refuses_bad_arguments_without_a_device():
    l = lib.load()
    call = getattr(l, CALL)
    good = lib.pack_layout(100, 21, 14)
    b = _Buffers()
    # a NULL layout, every required pointer, a negative size: -1 with a message
    assert call(None, *b.args()) == -1 and l.cbfssm_last_error().decode()
    for name in REQUIRED:
        assert call(C.byref(good), *b.args(null=(name,))) == -1 and l.cbfssm_last_error().decode(), name
    for over in ({'N': -1}, {'T': -1}, {'Dy': -1}):
        assert call(C.byref(good), *b.args(**over)) == -1 and l.cbfssm_last_error().decode(), over
    # all three cotangents NULL; gP0 is NULL exactly when P0 is, gvar_x exactly when var_x is
    assert call(C.byref(good), *b.args(null=('gmeans', 'gcovs', 'gloglik'))) == -1 and 'cotangent' in l.cbfssm_last_error().decode()
    for name in ('P0', 'gP0', 'var_x', 'gvar_x'):
        assert call(C.byref(good), *b.args(null=(name,))) == -1 and l.cbfssm_last_error().decode(), name
    # the limits: -3 with a message, before any launch and before any pointer is looked at
    for over in ({'Dy': 0}, {'Dy': 15}, {'N': 2 ** 30 + 1}, {'T': 2 ** 24 + 1}):
        assert call(C.byref(good), *b.args(**over)) == -3 and l.cbfssm_last_error().decode(), over
    for field, value in (('M', 321), ('M', 0), ('D', 25), ('D', 13), ('Do', 17), ('NBLK', 3)):
        lay = lib.pack_layout(100, 21, 14)
        setattr(lay, field, value)
        assert call(C.byref(lay), *b.args()) == -3 and l.cbfssm_last_error().decode(), (field, value)
        assert call(C.byref(lay), *b.args(null=REQUIRED + ('gmeans', 'gcovs', 'gloglik'))) == -3
    assert call(C.byref(good), *b.args(null=REQUIRED, Dy=0)) == -3
    # a and ga may be NULL only where the GP takes the state alone
    alone = lib.pack_layout(30, 5, 5)
    assert call(C.byref(alone), *_Buffers(Do=5, Dy=2, Da=0).args(null=('a', 'ga'), N=0)) == 0
    # nothing to do: no launch at N = 0 or T = 0; the optional arguments may be NULL in matching pairs, two cotangents too
    assert call(C.byref(good), *b.args(N=0)) == 0
    assert call(C.byref(good), *b.args(T=0)) == 0
    assert call(C.byref(good), *b.args(T=0, null=('P0', 'gP0', 'var_x', 'gvar_x', 'cond', 'gcovs', 'gloglik'))) == 0
    assert b.untouched()
