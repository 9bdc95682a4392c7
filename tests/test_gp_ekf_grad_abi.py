"""Host-side checks of the entry points of the differentiable GPModel.ekf (no GPU): the four symbols are declared, exported
and bound, the declarations say what they stand for, the counts are 64-bit, and bad arguments are refused on the host
before anything is launched -- with the output buffers untouched.  The limits are those of cbfssm_gp_ekf_f64, plus a layout
that has an adjoint slab."""
import ctypes as C
import os
import re

from cbfssm.hip import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAVE, GROUPS, WORK, BWD = ('cbfssm_gp_ekf_save_f64', 'cbfssm_gp_ekf_bwd_workgroups', 'cbfssm_gp_ekf_bwd_work_elems',
                           'cbfssm_gp_ekf_bwd_f64')
SENTINEL = -7.25
SAVE_ORDER = ['pack', 'm0', 'P0', 'a', 'y', 'cond', 'var_x', 'var_y', 'Dy', 'N', 'T', 'means', 'covs', 'loglik', 'pmeans',
              'pcovs', 'cross', 'jac', 'work', 'stream']
BWD_ORDER = ['pack', 'm0', 'P0', 'a', 'y', 'cond', 'var_x', 'var_y', 'Dy', 'means', 'covs', 'pmeans', 'pcovs', 'cross', 'jac',
             'gmeans', 'gcovs', 'gloglik', 'N', 'T', 'gm0', 'gP0', 'ga', 'gy', 'gpart', 'work', 'gB_image', 'stream']
SAVE_OUT = ('means', 'covs', 'loglik', 'pmeans', 'pcovs', 'cross', 'jac', 'work')
BWD_OUT = ('gm0', 'gP0', 'ga', 'gy', 'gpart', 'work', 'gB_image')
SAVE_REQUIRED = ('pack', 'm0', 'a', 'y', 'var_y') + SAVE_OUT
BWD_REQUIRED = ('pack', 'm0', 'a', 'y', 'var_y', 'means', 'covs', 'pmeans', 'pcovs', 'cross', 'jac', 'gm0', 'ga', 'gy', 'gpart',
                'work')
BWD_OPTIONAL = ('P0', 'cond', 'var_x', 'gmeans', 'gcovs', 'gloglik', 'gP0', 'gB_image')


def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, 'include', 'cbfssm_hip.h')).read()
    declared = set(re.findall(r'\b(cbfssm_[a-z0-9_]+)\s*\(', text))
    so = C.CDLL(lib.LIB_PATH)
    for name in (SAVE, GROUPS, WORK, BWD):
        assert name in declared and name in lib.SYMBOLS and hasattr(so, name), name
    l = lib.load()
    assert getattr(l, SAVE).restype is C.c_int and getattr(l, BWD).restype is C.c_int
    assert getattr(l, GROUPS).restype is C.c_int64 and getattr(l, WORK).restype is C.c_int64
    assert len(getattr(l, SAVE).argtypes) == 1 + len(SAVE_ORDER) == 21
    assert len(getattr(l, BWD).argtypes) == 1 + len(BWD_ORDER) == 29
    for name, order in ((SAVE, SAVE_ORDER), (BWD, BWD_ORDER)):
        decl = re.search(r'int %s\(([^;]*)\);' % name, text).group(1)
        names = [re.findall(r'\w+', part)[-1] for part in decl.split(',')]
        assert names == ['layout'] + order, names
    # the declarations say which reference call sites they stand for
    assert re.search(r'%s\([^;]*;\s*/\* gp_tf\.py:132-161, cbfssm\.py:199-221,245-251 \*/' % SAVE, text)
    for name in (GROUPS, WORK, BWD):
        assert re.search(r'%s\([^;]*;\s*/\* tf\.gradients of ' % name, text), name


def test_the_counts_are_64_bit_and_refuse_a_bad_layout():
    l = lib.load()
    groups, work = getattr(l, GROUPS), getattr(l, WORK)
    for (M, D, Do), nblk in (((1, 1, 1), 1), ((100, 21, 14), 7), ((113, 9, 1), 10), ((320, 24, 16), 20)):
        lay = lib.pack_layout(M, D, Do)
        assert lay.NBLK == nblk
        assert groups(C.byref(lay), 33) == 3 and groups(C.byref(lay), 0) == 0
        fixed = 16 * 16 * nblk + 2 * 3 * 4096                       # alpha, the lanes' rows of the covariance adjoint, Jh
        if lay.rev_stash:                                           # + the operand images of T + 1 slots per workgroup
            slots = 3 * (5 + 1)
            assert work(C.byref(lay), 33, 5) == fixed + 2 * slots * nblk * 256 + l.cbfssm_stash_contract_work_elems(C.byref(lay), slots)
        else:
            assert work(C.byref(lay), 33, 5) == fixed
    big = lib.pack_layout(320, 24, 16)
    assert work(C.byref(big), 2 ** 30, 2 ** 20) > 2 ** 56              # 64-bit arithmetic: no wrap at 32 bits
    assert groups(None, 1) == -1 and work(None, 1, 1) == -1
    good = lib.pack_layout(100, 21, 14)
    assert groups(C.byref(good), -1) == -1 and groups(C.byref(good), 2 ** 30 + 1) == -1
    assert work(C.byref(good), 1, -1) == -1 and work(C.byref(good), 1, 2 ** 24 + 1) == -1
    for field, value in (('M', 0), ('M', 321), ('D', 25), ('Do', 17), ('NBLK', 3), ('D', 13), ('rev_slab', 0), ('rev_stash', 1),
                         ('gp_form', 7)):                               # (D = 13 < Do = 14)
        lay = lib.pack_layout(100, 21, 14)
        setattr(lay, field, value)
        assert groups(C.byref(lay), 16) == -1 and work(C.byref(lay), 16, 2) == -1, (field, value)


class _Buffers:
    """host arrays behind every pointer of the two calls, filled with a sentinel"""

    def __init__(self, Do=14, Dy=7, N=3, T=2, Da=7):
        mat, vec = T * N * Do * Do, T * N * Do
        sizes = {'pack': 4, 'm0': N * Do, 'P0': N * Do * Do, 'a': T * N * Da, 'y': T * N * Dy, 'cond': T * N, 'var_x': Do,
                 'var_y': Dy, 'means': vec, 'covs': mat, 'loglik': N, 'pmeans': vec, 'pcovs': mat, 'cross': mat, 'jac': mat,
                 'gmeans': vec, 'gcovs': mat, 'gloglik': N, 'gm0': N * Do, 'gP0': N * Do * Do, 'ga': T * N * Da,
                 'gy': T * N * Dy, 'gpart': 16, 'work': 16, 'gB_image': 16}
        self.arr = {k: (C.c_double * n)(*([SENTINEL] * n)) for k, n in sizes.items()}
        self.Dy, self.N, self.T = Dy, N, T

    def args(self, order, null=(), **over):
        p = {k: (None if k in null else C.cast(v, C.c_void_p)) for k, v in self.arr.items()}
        p.update(Dy=self.Dy, N=self.N, T=self.T, stream=None)
        p.update(over)
        return [p[k] for k in order]

    def untouched(self, outputs):
        return all(x == SENTINEL for k in outputs for x in self.arr[k])


def _refusals(call, order, required, outputs):
    l = lib.load()
    good = lib.pack_layout(100, 21, 14)
    b = _Buffers()
    # a NULL layout, every required pointer, a negative size: -1 with a message
    assert call(None, *b.args(order)) == -1 and l.cbfssm_last_error().decode()
    for name in required:
        assert call(C.byref(good), *b.args(order, null=(name,))) == -1 and l.cbfssm_last_error().decode(), name
    for over in ({'N': -1}, {'T': -1}, {'Dy': -1}):
        assert call(C.byref(good), *b.args(order, **over)) == -1 and l.cbfssm_last_error().decode(), over
    # the limits: -3 with a message, before any launch -- Dy out of range, sizes, D < Do, a refused layout
    for over in ({'Dy': 0}, {'Dy': 15}, {'N': 2 ** 30 + 1}, {'T': 2 ** 24 + 1}):
        assert call(C.byref(good), *b.args(order, **over)) == -3 and l.cbfssm_last_error().decode(), over
    for field, value in (('M', 321), ('M', 0), ('D', 25), ('D', 13), ('Do', 17), ('NBLK', 3)):
        lay = lib.pack_layout(100, 21, 14)
        setattr(lay, field, value)
        assert call(C.byref(lay), *b.args(order)) == -3 and l.cbfssm_last_error().decode(), (field, value)
    assert call(C.byref(good), *b.args(order, null=required, Dy=0)) == -3
    # a may be NULL only where the GP takes the state alone
    alone = lib.pack_layout(30, 5, 5)
    assert call(C.byref(alone), *_Buffers(Do=5, Dy=2, Da=0).args(order, null=('a', 'ga'), N=0)) == 0
    # nothing to do: no launch at N = 0 or T = 0
    assert call(C.byref(good), *b.args(order, N=0)) == 0
    assert call(C.byref(good), *b.args(order, T=0)) == 0
    assert b.untouched(outputs)
    return b


def test_the_forward_under_grad_refuses_bad_arguments_without_a_device():
    l = lib.load()
    b = _refusals(getattr(l, SAVE), SAVE_ORDER, SAVE_REQUIRED, SAVE_OUT)
    good = lib.pack_layout(100, 21, 14)
    assert getattr(l, SAVE)(C.byref(good), *b.args(SAVE_ORDER, T=0, null=('P0', 'cond', 'var_x'))) == 0


def test_the_adjoint_refuses_bad_arguments_without_a_device():
    l = lib.load()
    call = getattr(l, BWD)
    b = _refusals(call, BWD_ORDER, BWD_REQUIRED, BWD_OUT)
    good = lib.pack_layout(100, 21, 14)
    assert call(C.byref(good), *b.args(BWD_ORDER, T=0, null=BWD_OPTIONAL)) == 0
    # a layout without an adjoint: -3
    for field, value in (('rev_slab', 0), ('rev_stash', 1), ('gp_form', 7)):
        lay = lib.pack_layout(100, 21, 14)
        setattr(lay, field, value)
        assert call(C.byref(lay), *b.args(BWD_ORDER)) == -3 and l.cbfssm_last_error().decode(), (field, value)
    # a stash height needs the image of the K^-1 adjoint
    tall = lib.pack_layout(113, 9, 1)
    bt = _Buffers(Do=1, Dy=1, Da=8)
    assert tall.rev_stash == 1
    assert call(C.byref(tall), *bt.args(BWD_ORDER, null=('gB_image',))) == -1 and l.cbfssm_last_error().decode()
    assert b.untouched(BWD_OUT) and bt.untouched(BWD_OUT)
