"""Host-side checks of the differentiable-GPModel entry points (no GPU): the new symbols are declared, exported and bound,
their counts are 64-bit, and bad arguments are refused on the host before anything is launched."""
import ctypes as C
import os
import re

from cbfssm.hip import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('cbfssm_gp_predict_bwd_workgroups', 'cbfssm_gp_predict_bwd_work_elems', 'cbfssm_gp_predict_bwd_f64', 'cbfssm_gp_tail_f64')


def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, 'include', 'cbfssm_hip.h')).read()
    declared = set(re.findall(r'\b(cbfssm_[a-z0-9_]+)\s*\(', text))
    so = C.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in lib.SYMBOLS and hasattr(so, name), name
    l = lib.load()
    assert l.cbfssm_gp_predict_bwd_f64.restype is C.c_int and l.cbfssm_gp_tail_f64.restype is C.c_int


def test_counts_are_64_bit_and_a_function_of_npts_and_tile_height():
    l = lib.load()
    for name in NEW[:2]:
        assert getattr(l, name).restype is C.c_int64, name
    lay = lib.pack_layout(300, 6, 4)                          # 20 row blocks, stash mode
    npts = 2 ** 33
    nblocks = npts // 16
    wk = l.cbfssm_gp_predict_bwd_work_elems(C.byref(lay), npts)
    assert wk == 2 * nblocks * 20 * 256 + l.cbfssm_stash_contract_work_elems(C.byref(lay), nblocks) and wk > 2 ** 32
    cap = l.cbfssm_gp_predict_bwd_workgroups(C.byref(lay), npts)
    assert 0 < cap <= 1024
    # one workgroup per 16-point block until the persistent grid is full; the same for every (D, Do) of a tile height
    lay2 = lib.pack_layout(290, 24, 16)
    for n in (0, 1, 16, 17, 41, 16 * cap, 16 * cap + 1, 10 ** 6):
        want = min((n + 15) // 16, cap)
        assert l.cbfssm_gp_predict_bwd_workgroups(C.byref(lay), n) == want
        assert l.cbfssm_gp_predict_bwd_workgroups(C.byref(lay2), n) == want
    small = lib.pack_layout(100, 21, 14)                      # register-resident tile: no workspace
    assert l.cbfssm_gp_predict_bwd_work_elems(C.byref(small), 10 ** 6) == 0
    assert l.cbfssm_gp_predict_bwd_workgroups(C.byref(small), 16 * 600 + 5) < 601   # persistent: several blocks each


def _broken(field, value):
    lay = lib.pack_layout(100, 21, 14)
    setattr(lay, field, value)
    return lay


def test_bad_arguments_are_refused_without_a_device():
    l = lib.load()
    good = lib.pack_layout(100, 21, 14)
    nul = [None] * 7
    for lay in (_broken('M', 321), _broken('D', 25), _broken('Do', 17), _broken('M', 0), _broken('NBLK', 3)):
        assert l.cbfssm_gp_predict_bwd_workgroups(C.byref(lay), 41) == -1
        assert l.cbfssm_gp_predict_bwd_work_elems(C.byref(lay), 41) == -1
        rc = l.cbfssm_gp_predict_bwd_f64(C.byref(lay), None, None, 41, *nul)
        assert rc < 0 and l.cbfssm_last_error().decode()
    assert l.cbfssm_gp_predict_bwd_workgroups(C.byref(good), -1) == -1
    assert l.cbfssm_gp_predict_bwd_work_elems(C.byref(good), -1) == -1
    assert l.cbfssm_gp_predict_bwd_workgroups(None, 41) == -1
    assert l.cbfssm_gp_predict_bwd_f64(C.byref(good), None, None, -1, *nul) < 0
    assert b'npts' in l.cbfssm_last_error()
    assert l.cbfssm_gp_predict_bwd_f64(C.byref(good), None, None, 41, *nul) < 0            # null pointers
    assert l.cbfssm_gp_predict_bwd_f64(None, None, None, 41, *nul) < 0
    # the tail: null pointers, limits
    assert l.cbfssm_gp_tail_f64(C.byref(good), None, None, None, 0, 1.0, None, None, None, None, None) < 0
    assert l.cbfssm_gp_tail_f64(None, None, None, None, 0, 1.0, None, None, None, None, None) < 0


def test_autograd_module_exposes_the_two_functions():
    from cbfssm.hip import autograd
    assert callable(autograd.gp_predict) and callable(autograd.gp_prior_kl)
    assert autograd.GP_PARAM_NAMES == ('zeta_pos', 'zeta_mean', 'zeta_var_unc', 'variance_unc', 'lengthscales_unc')
    from cbfssm.model import gp_tf
    assert 'valuation only' in gp_tf.conditional.__doc__ and hasattr(gp_tf.GPModel, 'parameters')
