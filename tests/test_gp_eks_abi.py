"""Host-side checks of the GPModel.eks entry points (no GPU): the two symbols are declared, exported and bound, the
declarations say where the recursion comes from, the count is 64-bit, and bad arguments are refused on the host before
anything is launched -- with the output buffers untouched.  The limits and refusals are those of cbfssm_gp_ekf_f64."""
import ctypes as C
import os
import re

from cbfssm.hip import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT = 'cbfssm_gp_eks_work_elems'
CALL = 'cbfssm_gp_eks_f64'
SENTINEL = -7.25
# after the layout: pack, m0, P0, a, y, cond, var_x, var_y | Dy, N, T | means, covs, loglik, pmeans, pcovs, cross, smeans,
# scovs, sm_init, sP_init, lag1, info, work, stream
ORDER = ['pack', 'm0', 'P0', 'a', 'y', 'cond', 'var_x', 'var_y', 'Dy', 'N', 'T', 'means', 'covs', 'loglik', 'pmeans', 'pcovs',
         'cross', 'smeans', 'scovs', 'sm_init', 'sP_init', 'lag1', 'info', 'work', 'stream']
OUTPUTS = ('means', 'covs', 'loglik', 'pmeans', 'pcovs', 'cross', 'smeans', 'scovs', 'sm_init', 'sP_init', 'lag1', 'info', 'work')
REQUIRED = ('pack', 'm0', 'a', 'y', 'var_y') + tuple(k for k in OUTPUTS if k != 'lag1')
OPTIONAL = ('P0', 'cond', 'var_x', 'lag1')


def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, 'include', 'cbfssm_hip.h')).read()
    declared = set(re.findall(r'\b(cbfssm_[a-z0-9_]+)\s*\(', text))
    so = C.CDLL(lib.LIB_PATH)
    for name in (COUNT, CALL):
        assert name in declared and name in lib.SYMBOLS and hasattr(so, name), name
    l = lib.load()
    assert getattr(l, CALL).restype is C.c_int and getattr(l, COUNT).restype is C.c_int64
    assert len(getattr(l, CALL).argtypes) == 1 + len(ORDER) == 26
    # the declaration names its arguments in this order
    decl = re.search(r'int %s\(([^;]*)\);' % CALL, text).group(1)
    names = [re.findall(r'\w+', part)[-1] for part in decl.split(',')]
    assert names == ['layout'] + ORDER, names
    # the declarations say where the recursion comes from
    for name in (COUNT, CALL):
        assert re.search(r'%s\([^;]*;\s*/\* gp_tf\.py:132-161, cbfssm\.py:199-221,245-251 \*/' % name, text), name


def test_the_count_is_64_bit_and_refuses_a_bad_layout():
    l = lib.load()
    count = getattr(l, COUNT)
    for (M, D, Do), nblk in (((1, 1, 1), 1), ((100, 21, 14), 7), ((113, 9, 1), 10), ((320, 24, 16), 20)):
        lay = lib.pack_layout(M, D, Do)
        assert lay.NBLK == nblk
        assert count(C.byref(lay)) == 16 * 16 * nblk == l.cbfssm_gp_ekf_work_elems(C.byref(lay))
    assert count(None) == -1
    for field, value in (('M', 0), ('M', 321), ('D', 25), ('Do', 17), ('NBLK', 3), ('D', 13)):   # (D = 13 < Do = 14)
        lay = lib.pack_layout(100, 21, 14)
        setattr(lay, field, value)
        assert count(C.byref(lay)) == -1, (field, value)


class _Buffers:
    """host arrays behind every pointer of the call, the outputs filled with a sentinel"""

    def __init__(self, Do=14, Dy=7, N=3, T=2, Da=7):
        mat = T * N * Do * Do
        sizes = {'pack': 4, 'm0': N * Do, 'P0': N * Do * Do, 'a': T * N * Da, 'y': T * N * Dy, 'cond': T * N, 'var_x': Do,
                 'var_y': Dy, 'means': T * N * Do, 'covs': mat, 'loglik': N, 'pmeans': T * N * Do, 'pcovs': mat, 'cross': mat,
                 'smeans': T * N * Do, 'scovs': mat, 'sm_init': N * Do, 'sP_init': N * Do * Do, 'lag1': mat, 'info': N,
                 'work': 16}
        self.arr = {k: (C.c_double * n)(*([SENTINEL] * n)) for k, n in sizes.items()}
        self.Dy, self.N, self.T = Dy, N, T

    def args(self, null=(), **over):
        p = {k: (None if k in null else C.cast(v, C.c_void_p)) for k, v in self.arr.items()}
        p.update(Dy=self.Dy, N=self.N, T=self.T, stream=None)
        p.update(over)
        return [p[k] for k in ORDER]

    def untouched(self):
        return all(x == SENTINEL for k in OUTPUTS for x in self.arr[k])


def test_bad_arguments_are_refused_without_a_device():
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
    # the limits: -3 with a message, before any launch
    for over in ({'Dy': 0}, {'Dy': 15}, {'N': 2 ** 30 + 1}, {'T': 2 ** 24 + 1}):
        assert call(C.byref(good), *b.args(**over)) == -3 and l.cbfssm_last_error().decode(), over
    for field, value in (('M', 321), ('M', 0), ('D', 25), ('D', 13), ('Do', 17), ('NBLK', 3)):   # M = 321; D < Do
        lay = lib.pack_layout(100, 21, 14)
        setattr(lay, field, value)
        assert call(C.byref(lay), *b.args()) == -3 and l.cbfssm_last_error().decode(), (field, value)
    # a limit violation is reported even when pointers are missing too (nothing is looked at before the limits)
    assert call(C.byref(good), *b.args(null=REQUIRED, Dy=0)) == -3
    # a may be NULL only where the GP takes the state alone
    alone = lib.pack_layout(30, 5, 5)
    assert call(C.byref(alone), *_Buffers(Do=5, Dy=2, Da=0).args(null=('a',), N=0)) == 0
    # nothing to do: no launch at N = 0 or T = 0; whatever is optional, lag1 among it, may be NULL
    assert call(C.byref(good), *b.args(N=0)) == 0
    assert call(C.byref(good), *b.args(T=0, null=OPTIONAL)) == 0
    assert b.untouched()
    # the refusals are those of cbfssm_gp_ekf_f64: the same code for the same bad sizes
    ekf = l.cbfssm_gp_ekf_f64
    for over in ({'Dy': 0}, {'N': -1}, {'T': 2 ** 24 + 1}):
        a = b.args(**over)
        assert call(C.byref(good), *a) == ekf(C.byref(good), *a[:14], a[ORDER.index('work')], None), over
