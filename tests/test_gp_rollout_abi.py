"""Host-side checks of the GP-rollout entry points (no GPU): the new symbols are declared, exported and bound, their
counts are 64-bit host arithmetic, and bad arguments are refused on the host before anything is launched."""
import ctypes as C
import os
import re

from cbfssm.hip import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = ('cbfssm_gp_rollout_partials', 'cbfssm_gp_rollout_bwd_workgroups', 'cbfssm_gp_rollout_bwd_work_elems')
CALLS = ('cbfssm_gp_rollout_f64', 'cbfssm_gp_rollout_bwd_f64')


def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, 'include', 'cbfssm_hip.h')).read()
    declared = set(re.findall(r'\b(cbfssm_[a-z0-9_]+)\s*\(', text))
    so = C.CDLL(lib.LIB_PATH)
    for name in COUNTS + CALLS:
        assert name in declared and name in lib.SYMBOLS and hasattr(so, name), name
    l = lib.load()
    for name in CALLS:
        assert getattr(l, name).restype is C.c_int, name
    # each entry cites the reference lines it replaces
    for name in CALLS:
        at = text.index(' * ' + name)
        assert 'voliro.py:139-186' in text[at:at + 200] and 'cbfssm.py:199-206,224' in text[at:at + 200], name


def test_counts_are_64_bit_host_arithmetic():
    l = lib.load()
    for name in COUNTS:
        assert getattr(l, name).restype is C.c_int64, name
    for (M, D, Do) in ((12, 4, 3), (100, 21, 14), (113, 9, 1), (300, 6, 4)):
        lay = lib.pack_layout(M, D, Do)
        for N in (0, 1, 15, 16, 17, 37, 5120):
            groups = (N + 15) // 16
            assert l.cbfssm_gp_rollout_partials(C.byref(lay), N) == groups
            assert l.cbfssm_gp_rollout_bwd_workgroups(C.byref(lay), N) == groups
            for T in (0, 1, 7, 250):
                want = 0
                if lay.rev_stash:
                    want = 2 * groups * T * lay.NBLK * 256 + l.cbfssm_stash_contract_work_elems(C.byref(lay), groups * T)
                assert l.cbfssm_gp_rollout_bwd_work_elems(C.byref(lay), N, T) == want, (M, N, T)
    assert lib.pack_layout(112, 24, 16).rev_stash == 0 and lib.pack_layout(113, 9, 1).rev_stash == 1
    # a size above 2^32 doubles
    lay = lib.pack_layout(300, 6, 4)
    N, T = 2 ** 20, 2 ** 10
    slots = (N // 16) * T
    wk = l.cbfssm_gp_rollout_bwd_work_elems(C.byref(lay), N, T)
    assert wk == 2 * slots * 20 * 256 + l.cbfssm_stash_contract_work_elems(C.byref(lay), slots) and wk > 2 ** 32


def _broken(field, value):
    lay = lib.pack_layout(100, 21, 14)
    setattr(lay, field, value)
    return lay


def test_bad_arguments_are_refused_without_a_device():
    l = lib.load()
    good = lib.pack_layout(100, 21, 14)
    one = C.c_void_p(8)                              # a non-null address that is never dereferenced: every call below fails first

    def fwd(lay, N, T, ptr=None):
        return l.cbfssm_gp_rollout_f64(lay, ptr, ptr, ptr, ptr, ptr, N, T, 0, ptr, ptr, ptr, None)

    def bwd(lay, N, T, ptr=None):
        return l.cbfssm_gp_rollout_bwd_f64(lay, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, N, T, 0, ptr, ptr, ptr, ptr, ptr, None)

    for lay in (_broken('M', 321), _broken('D', 25), _broken('Do', 17), _broken('M', 0), _broken('NBLK', 3), _broken('Do', 22),
                _broken('gp_form', 7)):
        assert l.cbfssm_gp_rollout_partials(C.byref(lay), 37) == -1
        assert l.cbfssm_gp_rollout_bwd_workgroups(C.byref(lay), 37) == -1
        assert l.cbfssm_gp_rollout_bwd_work_elems(C.byref(lay), 37, 8) == -1
        # above the limits: -3 before any launch, even with plausible pointers
        assert fwd(C.byref(lay), 37, 8, one) == -3 and l.cbfssm_last_error().decode()
        assert bwd(C.byref(lay), 37, 8, one) == -3 and l.cbfssm_last_error().decode()
    for name in COUNTS[:2]:
        assert getattr(l, name)(C.byref(good), -1) == -1 and getattr(l, name)(None, 37) == -1
    assert l.cbfssm_gp_rollout_bwd_work_elems(C.byref(good), -1, 8) == -1
    assert l.cbfssm_gp_rollout_bwd_work_elems(C.byref(good), 37, -1) == -1
    assert l.cbfssm_gp_rollout_bwd_work_elems(None, 37, 8) == -1
    # negative sizes, no steps, too many chains
    assert fwd(C.byref(good), -1, 8, one) == -1 and fwd(C.byref(good), 37, -1, one) == -1 and fwd(C.byref(good), 37, 0, one) == -1
    assert bwd(C.byref(good), -1, 8, one) == -1 and bwd(C.byref(good), 37, 0, one) == -1
    assert fwd(C.byref(good), 2 ** 30 + 1, 8, one) == -3 and bwd(C.byref(good), 37, 2 ** 24 + 1, one) == -3
    # null pointers, null layout
    assert fwd(C.byref(good), 37, 8) == -1 and b'null' in l.cbfssm_last_error()
    assert bwd(C.byref(good), 37, 8) == -1 and b'null' in l.cbfssm_last_error()
    assert fwd(None, 37, 8, one) == -1 and bwd(None, 37, 8, one) == -1


def test_python_surface():
    from cbfssm.hip import autograd
    from cbfssm.model import gp_tf
    assert callable(autograd.gp_rollout) and callable(autograd.gp_rollout_eval)
    assert hasattr(gp_tf.GPModel, 'rollout') and 'addition to the reference' in gp_tf.GPModel.rollout.__doc__
