"""Host-side checks of the entry points of the model adjoint of GPModel.moment_match (no GPU): the two symbols are declared,
exported and bound, the count is 64-bit and what the header and DESIGN 3.2o say at the grid rows, and bad arguments are
refused on the host before anything is launched."""
import ctypes as C
import os
import re

import gp_tile_grid as grid
from cbfssm.hip import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT = 'cbfssm_gp_moment_match_params_bwd_work_elems'
CALL = 'cbfssm_gp_moment_match_params_bwd_f64'
ARGS = ('pack', 'cflat', 'mean', 'cov', 'gfmean', 'gfcov', 'gxcov', 'gmean', 'gcov', 'xcov', 'red_slab', 'gB_dense', 'work')


def _call(l, lay, npts, **off):
    """the call with a (never dereferenced) pointer for every argument but those named false, which are NULL; gB_dense
    follows the layout unless it is named"""
    buf = (C.c_double * 4)()
    p = C.cast(buf, C.c_void_p)
    a = {k: (p if off.get(k, True) else None) for k in ARGS}
    if 'gB_dense' not in off and (lay is None or not lay.rev_stash):
        a['gB_dense'] = None
    return getattr(l, CALL)(C.byref(lay) if lay is not None else None, a['pack'], a['cflat'], a['mean'], a['cov'], npts,
                            a['gfmean'], a['gfcov'], a['gxcov'], a['gmean'], a['gcov'], a['xcov'], a['red_slab'], a['gB_dense'],
                            a['work'], None)


def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, 'include', 'cbfssm_hip.h')).read()
    declared = set(re.findall(r'\b(cbfssm_[a-z0-9_]+)\s*\(', text))
    so = C.CDLL(lib.LIB_PATH)
    for name in (COUNT, CALL):
        assert name in declared and name in lib.SYMBOLS and hasattr(so, name), name
        assert re.search(r'\b%s\(.{0,160}?/\* gp_tf\.py:132-161 \*/' % name, text, re.S), name
    l = lib.load()
    fn = getattr(l, CALL)
    assert fn.restype is C.c_int and len(fn.argtypes) == 16
    assert fn.argtypes[5] is C.c_int64 and all(t is C.c_void_p for i, t in enumerate(fn.argtypes) if i not in (0, 5))
    cnt = getattr(l, COUNT)
    assert cnt.restype is C.c_int64 and len(cnt.argtypes) == 2 and cnt.argtypes[1] is C.c_int64
    # the input adjoint's entry point keeps its thirteen arguments
    assert len(l.cbfssm_gp_moment_match_bwd_f64.argtypes) == 13


def _documented(M, D, Do, npts):
    """the sections of `work` as DESIGN 3.2o lists them, each rounded up to eight doubles"""
    nb = (M + 15) // 16
    nwg = min(npts, 512)
    nch = max(1, min(-(-2048 // (nb * nb)), 64, (npts + 7) // 8))
    pc = max(1, -(-npts // nch))
    nch = max(1, -(-npts // pc))
    sections = [M * Do, Do * M * M, npts * M * D, npts * M, npts * D, npts * 2, nwg * (M * Do + M * D + D + 4),
                nch * (Do + 1) * M * M, nch * nb * M * D, nch * nb * M * Do, (Do + 1) * M * M, M * Do, M * D, D, 4, M, Do * M * M]
    return sum((s + 7) // 8 * 8 for s in sections)


def test_the_count_is_64_bit_and_as_documented_at_the_grid_rows():
    l = lib.load()
    cnt = getattr(l, COUNT)
    for _, M, D, Do in grid.ROWS:
        lay = lib.pack_layout(M, D, Do)
        for npts in (1, 16, 37, 5120, 16 * 1026 + 5):
            assert cnt(C.byref(lay), npts) == _documented(M, D, Do, npts), (M, D, Do, npts)
    # the two profile shapes: 167.6 MB and 3.7 MB
    assert cnt(C.byref(lib.pack_layout(100, 21, 14)), 5120) == _documented(100, 21, 14, 5120) == 20950600
    assert cnt(C.byref(lib.pack_layout(20, 19, 6)), 320) == _documented(20, 19, 6, 320) == 462360
    # sized by the launch, in 64 bits
    big = cnt(C.byref(lib.pack_layout(320, 24, 16)), 1 << 22)
    assert big > (1 << 34) and big == _documented(320, 24, 16, 1 << 22)
    assert cnt(None, 5) == -1 and cnt(C.byref(lib.pack_layout(100, 21, 14)), -1) == -1


def _broken(field, value):
    lay = lib.pack_layout(100, 21, 14)
    setattr(lay, field, value)
    return lay


def test_limits_and_bad_layouts_are_refused_before_any_launch():
    l = lib.load()
    for lay in (_broken('M', 321), _broken('D', 25), _broken('Do', 17), _broken('M', 0), _broken('NBLK', 3),
                _broken('rev_slab', 0), _broken('rev_slab', 12345), _broken('rev_stash', 1)):
        assert getattr(l, COUNT)(C.byref(lay), 41) == -1
        assert _call(l, lay, 41) == -3 and l.cbfssm_last_error().decode()
        # (before any pointer is looked at)
        assert _call(l, lay, 41, **{k: False for k in ARGS}) == -3


def test_null_pointers_missing_cotangents_and_a_negative_count_are_refused():
    l = lib.load()
    good, stash = lib.pack_layout(100, 21, 14), lib.pack_layout(130, 6, 4)
    assert not good.rev_stash and stash.rev_stash
    assert _call(l, None, 41) == -1
    for name in ('pack', 'cflat', 'mean', 'gmean', 'red_slab', 'work'):
        assert _call(l, good, 41, **{name: False}) == -1 and l.cbfssm_last_error().decode(), name
        assert _call(l, good, 0, **{name: False}) == -1, name
    assert _call(l, good, -1) == -1 and l.cbfssm_last_error().decode()
    # not all three cotangents may be NULL; gcov is NULL exactly when cov is; a cotangent for xcov needs xcov
    assert _call(l, good, 41, gfmean=False, gfcov=False, gxcov=False) == -1 and 'cotangent' in l.cbfssm_last_error().decode()
    assert _call(l, good, 41, cov=False) == -1 and _call(l, good, 41, gcov=False) == -1
    assert _call(l, good, 41, xcov=False) == -1 and 'xcov' in l.cbfssm_last_error().decode()
    # the dense K^-1 adjoint goes with the layout: required above seven row blocks, refused below
    assert _call(l, good, 41, gB_dense=True) == -1 and 'dense' in l.cbfssm_last_error().decode()
    assert _call(l, stash, 41, gB_dense=False) == -1 and 'dense' in l.cbfssm_last_error().decode()
    # nothing to do: returns before any launch (no device is needed)
    assert _call(l, good, 0) == 0 and _call(l, stash, 0) == 0
    assert _call(l, good, 0, gfcov=False, gxcov=False, xcov=False) == 0
    assert _call(l, good, 0, cov=False, gcov=False, gfmean=False) == 0
