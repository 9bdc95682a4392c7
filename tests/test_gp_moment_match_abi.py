"""Host-side checks of the GPModel.moment_match entry points (no GPU): the two symbols are declared, exported and bound, the
count is 64-bit, and bad arguments are refused on the host before anything is launched."""
import ctypes as C
import os
import re

from cbfssm.hip import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT = 'cbfssm_gp_moment_match_work_elems'
CALL = 'cbfssm_gp_moment_match_f64'


def _buf():
    buf = (C.c_double * 4)()
    return buf, C.cast(buf, C.c_void_p)


def _call(l, lay, npts, pack=True, mean=True, cov=True, fmean=True, fcov=True, xcov=True, info=True, work=True):
    """the call with a (never dereferenced) pointer where the flag is true and NULL where it is false"""
    keep, p = _buf()
    ptr = lambda on: p if on else None
    return getattr(l, CALL)(C.byref(lay) if lay is not None else None, ptr(pack), ptr(mean), ptr(cov), npts, ptr(fmean),
                            ptr(fcov), ptr(xcov), ptr(info), ptr(work), None)


def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, 'include', 'cbfssm_hip.h')).read()
    declared = set(re.findall(r'\b(cbfssm_[a-z0-9_]+)\s*\(', text))
    so = C.CDLL(lib.LIB_PATH)
    for name in (COUNT, CALL):
        assert name in declared and name in lib.SYMBOLS and hasattr(so, name), name
    assert getattr(lib.load(), CALL).restype is C.c_int
    assert len(getattr(lib.load(), CALL).argtypes) == 11
    # the header says where the function comes from
    assert re.search(r'gp_tf\.py:132-161[^;]*moment matching', text, re.S)
    assert re.search(r'cbfssm_gp_moment_match_f64: pack prepared', text)


def test_the_count_is_64_bit():
    l = lib.load()
    assert getattr(l, COUNT).restype is C.c_int64
    for (M, D, Do), nblk in (((1, 1, 1), 1), ((100, 21, 14), 7), ((113, 9, 1), 10), ((320, 24, 16), 20)):
        lay = lib.pack_layout(M, D, Do)
        assert lay.NBLK == nblk
        # alpha = K^-1 mu, [16][16 NBLK], and the W_d tiles [Do][NBLK][NBLK][256]
        assert getattr(l, COUNT)(C.byref(lay)) == 16 * 16 * nblk + Do * nblk * nblk * 256
    assert getattr(l, COUNT)(None) == -1


def _broken(field, value):
    lay = lib.pack_layout(100, 21, 14)
    setattr(lay, field, value)
    return lay


def test_limits_are_refused_before_any_launch():
    l = lib.load()
    for lay in (_broken('M', 321), _broken('D', 25), _broken('Do', 17), _broken('M', 0), _broken('NBLK', 3)):
        assert getattr(l, COUNT)(C.byref(lay)) == -1
        assert _call(l, lay, 41) == -3 and l.cbfssm_last_error().decode()
        # (before any pointer is looked at)
        assert _call(l, lay, 41, pack=False, mean=False, fmean=False, fcov=False, info=False, work=False) == -3


def test_null_pointers_and_a_negative_count_are_refused():
    l = lib.load()
    good = lib.pack_layout(100, 21, 14)
    assert _call(l, None, 41) == -1
    for name in ('pack', 'mean', 'fmean', 'fcov', 'info', 'work'):
        assert _call(l, good, 41, **{name: False}) == -1 and l.cbfssm_last_error().decode(), name
        assert _call(l, good, 0, **{name: False}) == -1, name
    assert _call(l, good, -1) == -1 and l.cbfssm_last_error().decode()
    # nothing to do: returns before any launch (no device is needed); cov and xcov may be NULL
    assert _call(l, good, 0) == 0
    assert _call(l, good, 0, cov=False, xcov=False) == 0
