"""Host-side checks of the GPModel.linearize entry points (no GPU): the two symbols are declared, exported and bound, the
count is 64-bit, and bad arguments are refused on the host before anything is launched."""
import ctypes as C
import os
import re

from cbfssm.hip import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT = 'cbfssm_gp_linearize_work_elems'
CALL = 'cbfssm_gp_linearize_f64'
NULLS = [None] * 6                        # fmean, fvar, dmean, dvar, work, stream


def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, 'include', 'cbfssm_hip.h')).read()
    declared = set(re.findall(r'\b(cbfssm_[a-z0-9_]+)\s*\(', text))
    so = C.CDLL(lib.LIB_PATH)
    for name in (COUNT, CALL):
        assert name in declared and name in lib.SYMBOLS and hasattr(so, name), name
    assert getattr(lib.load(), CALL).restype is C.c_int
    # the header says where the function comes from
    assert re.search(r'tf\.gradients\(fmean\[:, d\], Xnew\)[^;]*gp_tf\.py:132-161', text, re.S)


def test_the_count_is_64_bit():
    l = lib.load()
    assert getattr(l, COUNT).restype is C.c_int64
    for (M, D, Do), nblk in (((1, 1, 1), 1), ((100, 21, 14), 7), ((113, 9, 1), 10), ((320, 24, 16), 20)):
        lay = lib.pack_layout(M, D, Do)
        assert lay.NBLK == nblk
        assert getattr(l, COUNT)(C.byref(lay)) == 16 * 16 * nblk            # alpha = K^-1 mu, [16][16 NBLK]


def _broken(field, value):
    lay = lib.pack_layout(100, 21, 14)
    setattr(lay, field, value)
    return lay


def test_bad_arguments_are_refused_without_a_device():
    l = lib.load()
    count, call = getattr(l, COUNT), getattr(l, CALL)
    good = lib.pack_layout(100, 21, 14)
    for lay in (_broken('M', 0), _broken('M', 321), _broken('D', 25), _broken('Do', 17), _broken('NBLK', 3)):
        assert count(C.byref(lay)) == -1
        assert call(C.byref(lay), None, None, 41, *NULLS) == -3 and l.cbfssm_last_error().decode()
    assert count(None) == -1
    # NULL pointers and a negative count: -1, with a message, before any launch
    assert call(None, None, None, 41, *NULLS) == -1
    assert call(C.byref(good), None, None, 41, *NULLS) == -1 and l.cbfssm_last_error().decode()
    assert call(C.byref(good), None, None, -1, *NULLS) == -1 and l.cbfssm_last_error().decode()
    # nothing to do: no launch, no pointer is looked at beyond the NULL checks
    buf = (C.c_double * 4)()
    p = C.cast(buf, C.c_void_p)
    assert call(C.byref(good), p, p, -1, None, None, p, None, p, None) == -1
    assert call(C.byref(good), p, p, 0, None, None, None, None, p, None) == -1        # dmean is required
    assert call(C.byref(good), p, p, 0, None, None, p, None, None, None) == -1        # work is required
    assert call(C.byref(good), p, p, 0, None, None, p, None, p, None) == 0            # npts = 0: returns before any launch
