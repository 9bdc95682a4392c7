"""Host-side checks of the entry points of the input adjoint of GPModel.moment_match (no GPU): the two symbols are declared,
exported and bound, the count is 64-bit and what the header says at every tile height, and bad arguments are refused on the
host before anything is launched."""
import ctypes as C
import os
import re

from cbfssm.hip import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT = 'cbfssm_gp_moment_match_bwd_work_elems'
CALL = 'cbfssm_gp_moment_match_bwd_f64'
ARGS = ('pack', 'mean', 'cov', 'gfmean', 'gfcov', 'gxcov', 'gmean', 'gcov', 'info', 'work')


def _call(l, lay, npts, **off):
    """the call with a (never dereferenced) pointer for every argument but those named false, which are NULL"""
    buf = (C.c_double * 4)()
    p = C.cast(buf, C.c_void_p)
    a = {k: (p if off.get(k, True) else None) for k in ARGS}
    return getattr(l, CALL)(C.byref(lay) if lay is not None else None, a['pack'], a['mean'], a['cov'], npts, a['gfmean'],
                            a['gfcov'], a['gxcov'], a['gmean'], a['gcov'], a['info'], a['work'], None)


def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, 'include', 'cbfssm_hip.h')).read()
    declared = set(re.findall(r'\b(cbfssm_[a-z0-9_]+)\s*\(', text))
    so = C.CDLL(lib.LIB_PATH)
    for name in (COUNT, CALL):
        assert name in declared and name in lib.SYMBOLS and hasattr(so, name), name
        # each declaration says where the function comes from, as its forward does
        assert re.search(r'\b%s\(.{0,120}?/\* gp_tf\.py:132-161 \*/' % name, text, re.S), name
    fn = getattr(lib.load(), CALL)
    assert fn.restype is C.c_int and len(fn.argtypes) == 13
    assert fn.argtypes[4] is C.c_int64 and all(t is C.c_void_p for i, t in enumerate(fn.argtypes) if i not in (0, 4))


def _waves(nblk):
    return (nblk + 1) // 2 if nblk > 7 else nblk


def _cap(nblk):
    return 1024 if nblk <= 2 else (512 if nblk <= 7 else 256)


def test_the_count_is_64_bit_and_as_documented_at_every_tile_height():
    l = lib.load()
    assert getattr(l, COUNT).restype is C.c_int64
    shapes = (((1, 1, 1), 1), ((24, 8, 8), 2), ((50, 9, 2), 4), ((100, 21, 14), 7), ((113, 9, 1), 10), ((180, 12, 3), 13),
              ((250, 12, 6), 16), ((320, 24, 16), 20))
    for (M, D, Do), nblk in shapes:
        lay = lib.pack_layout(M, D, Do)
        assert lay.NBLK == nblk
        dp, mp, lt = 4 * lay.DK, 16 * nblk, 16 * lay.DK * lay.DK
        # the forward's sections, then per workgroup and point of the pair: the waves' G_half slots, the row sums [o][row],
        # H / AH / Yh / Hb [16][DP], seven DP x DP matrices and four vectors
        point = _waves(nblk) * lt + (nblk // 2 + 1) * mp + 4 * 16 * dp + 7 * lt + 4 * dp
        assert getattr(l, COUNT)(C.byref(lay)) == 16 * 16 * nblk + Do * nblk * nblk * 256 + _cap(nblk) * 2 * point
        assert getattr(l, COUNT)(C.byref(lay)) > l.cbfssm_gp_moment_match_work_elems(C.byref(lay))
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
        assert _call(l, lay, 41, **{k: False for k in ARGS}) == -3


def test_null_pointers_and_a_negative_count_are_refused():
    l = lib.load()
    good = lib.pack_layout(100, 21, 14)
    assert _call(l, None, 41) == -1
    for name in ('pack', 'mean', 'gmean', 'work'):
        assert _call(l, good, 41, **{name: False}) == -1 and l.cbfssm_last_error().decode(), name
        assert _call(l, good, 0, **{name: False}) == -1, name
    assert _call(l, good, -1) == -1 and l.cbfssm_last_error().decode()
    # not all three cotangents may be NULL; gcov is NULL exactly when cov is
    assert _call(l, good, 41, gfmean=False, gfcov=False, gxcov=False) == -1 and 'cotangent' in l.cbfssm_last_error().decode()
    assert _call(l, good, 41, cov=False) == -1 and _call(l, good, 41, gcov=False) == -1
    # nothing to do: returns before any launch (no device is needed); info, one or two cotangents, cov with gcov may be NULL
    assert _call(l, good, 0) == 0
    assert _call(l, good, 0, info=False, gfcov=False, gxcov=False) == 0
    assert _call(l, good, 0, cov=False, gcov=False, gfmean=False) == 0
