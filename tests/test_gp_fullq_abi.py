"""Host-side checks of the full-covariance q(z) entry points (no GPU): the new symbols are declared, exported and bound,
their counts are 64-bit, and bad arguments are refused on the host before anything is launched."""
import ctypes as C
import os
import re

from cbfssm.hip import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = ('cbfssm_gp_fullq_bwd_workgroups', 'cbfssm_gp_fullq_a2_elems', 'cbfssm_gp_fullq_bwd_work_elems',
          'cbfssm_gp_fullq_wd_work_elems')
CALLS = ('cbfssm_gp_fullq_prepare_f64', 'cbfssm_gp_fullq_predict_f64', 'cbfssm_gp_fullq_kl_f64', 'cbfssm_gp_fullq_bwd_f64', 'cbfssm_gp_fullq_wd_f64',
         'cbfssm_gp_fullq_lbar_f64', 'cbfssm_gp_tail_fullq_f64')
NEW = ('cbfssm_gp_fullq_pack_elems',) + COUNTS + CALLS


def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, 'include', 'cbfssm_hip.h')).read()
    declared = set(re.findall(r'\b(cbfssm_[a-z0-9_]+)\s*\(', text))
    so = C.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in lib.SYMBOLS and hasattr(so, name), name
    l = lib.load()
    for name in CALLS:
        assert getattr(l, name).restype is C.c_int, name


def test_counts_are_64_bit():
    l = lib.load()
    for name in ('cbfssm_gp_fullq_pack_elems',) + COUNTS:
        assert getattr(l, name).restype is C.c_int64, name
    lay = lib.pack_layout(300, 6, 4)                          # 20 row blocks, stash mode
    npts = 2 ** 33
    nblocks = npts // 16
    assert l.cbfssm_gp_fullq_a2_elems(C.byref(lay), npts) == nblocks * 20 * 256 > 2 ** 32
    wk = l.cbfssm_gp_fullq_bwd_work_elems(C.byref(lay), npts)
    assert wk == 2 * nblocks * 20 * 256 + l.cbfssm_stash_contract_work_elems(C.byref(lay), nblocks) and wk > 2 ** 32
    assert l.cbfssm_gp_fullq_bwd_workgroups(C.byref(lay), npts) == l.cbfssm_gp_predict_bwd_workgroups(C.byref(lay), npts)
    # W_d: lower-triangular 16 x 16 tiles only, at most eight slices of the points
    assert l.cbfssm_gp_fullq_wd_work_elems(C.byref(lay), npts) == 8 * 4 * (20 * 21 // 2) * 256
    assert l.cbfssm_gp_fullq_wd_work_elems(C.byref(lay), 33) == 1 * 4 * (20 * 21 // 2) * 256
    assert l.cbfssm_gp_fullq_pack_elems(C.byref(lay)) == 4 * 20 * 80 * 64 + 4 * 300 * 300 + 300 * 300
    small = lib.pack_layout(100, 21, 14)                      # register-resident tile: no stash workspace
    assert l.cbfssm_gp_fullq_bwd_work_elems(C.byref(small), 10 ** 6) == 0
    assert l.cbfssm_gp_fullq_a2_elems(C.byref(small), 41) == 3 * 7 * 256
    for n in (0, 1, 16, 17, 41, 10 ** 6):
        assert l.cbfssm_gp_fullq_bwd_workgroups(C.byref(small), n) == l.cbfssm_gp_predict_bwd_workgroups(C.byref(small), n)


def _broken(field, value):
    lay = lib.pack_layout(100, 21, 14)
    setattr(lay, field, value)
    return lay


def test_bad_arguments_are_refused_without_a_device():
    l = lib.load()
    good = lib.pack_layout(100, 21, 14)
    for lay in (_broken('M', 321), _broken('D', 25), _broken('Do', 17), _broken('M', 0), _broken('NBLK', 3)):
        assert l.cbfssm_gp_fullq_pack_elems(C.byref(lay)) == -1
        for name in COUNTS:
            assert getattr(l, name)(C.byref(lay), 41) == -1, name
        assert l.cbfssm_gp_fullq_prepare_f64(C.byref(lay), None, None, None) == -3 and l.cbfssm_last_error().decode()
        assert l.cbfssm_gp_fullq_bwd_f64(C.byref(lay), None, None, None, 41, *([None] * 8)) == -3
        assert l.cbfssm_gp_fullq_wd_f64(C.byref(lay), None, None, 41, None, None, None) == -3
        assert l.cbfssm_gp_fullq_predict_f64(C.byref(lay), None, None, None, 41, None, None, None) == -3
        assert l.cbfssm_gp_fullq_lbar_f64(C.byref(lay), None, None, None, 0.0, None, None) == -3
        assert l.cbfssm_gp_fullq_kl_f64(C.byref(lay), None, None, None, None, None, None) == -3
    for name in COUNTS:
        assert getattr(l, name)(C.byref(good), -1) == -1, name
        assert getattr(l, name)(None, 41) == -1, name
    assert l.cbfssm_gp_fullq_pack_elems(None) == -1
    # NULL pointers: -1, with a message
    assert l.cbfssm_gp_fullq_prepare_f64(C.byref(good), None, None, None) == -1 and l.cbfssm_last_error().decode()
    assert l.cbfssm_gp_fullq_bwd_f64(C.byref(good), None, None, None, 41, *([None] * 8)) == -1
    assert l.cbfssm_gp_fullq_bwd_f64(None, None, None, None, 41, *([None] * 8)) == -1
    assert l.cbfssm_gp_fullq_wd_f64(C.byref(good), None, None, 41, None, None, None) == -1
    assert l.cbfssm_gp_fullq_predict_f64(C.byref(good), None, None, None, 41, None, None, None) == -1
    assert l.cbfssm_gp_fullq_predict_f64(None, None, None, None, 41, None, None, None) == -1
    assert l.cbfssm_gp_fullq_predict_f64(C.byref(good), None, None, None, -1, None, None, None) == -1
    assert l.cbfssm_gp_fullq_lbar_f64(C.byref(good), None, None, None, 0.0, None, None) == -1
    assert l.cbfssm_gp_fullq_kl_f64(C.byref(good), None, None, None, None, None, None) == -1
    assert l.cbfssm_gp_tail_fullq_f64(C.byref(good), None, None, None, None, 0, 1.0, None, None, None, None, None) == -1
    assert l.cbfssm_gp_fullq_bwd_f64(C.byref(good), None, None, None, -1, *([None] * 8)) == -1
