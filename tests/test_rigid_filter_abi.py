"""Host-side checks of the rigid-filter entry points (no GPU): the new symbols are declared, exported and bound, the count
is 64-bit host arithmetic, and bad arguments are refused on the host before anything is launched."""
import ctypes as C
import os
import re

from cbfssm.hip import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = ('cbfssm_rigid_filter_partials',)
CALLS = ('cbfssm_rigid_filter_f64', 'cbfssm_rigid_filter_bwd_f64')


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
        assert 'voliro.py:188-242,314-338' in text[at:at + 200], name
    assert 'struct cbfssm_rigid_body' in text
    assert C.sizeof(lib.RigidBody) == 8 * 8


def test_counts_are_64_bit_host_arithmetic():
    l = lib.load()
    assert l.cbfssm_rigid_filter_partials.restype is C.c_int64
    for N, want in ((0, 0), (1, 1), (63, 1), (64, 1), (65, 2), (320, 5), (2 ** 30, 2 ** 24)):
        assert l.cbfssm_rigid_filter_partials(N) == want, N
    assert l.cbfssm_rigid_filter_partials(-1) == -1


def test_bad_arguments_are_refused_without_a_device():
    l = lib.load()
    rb = lib.rigid_body(0.25, (12.0, 12.0, 6.0), (0.0, 0.0, 9.81), 0.01)
    one = C.c_void_p(8)                              # a non-null address that is never dereferenced: every call below fails first

    def fwd(body, N, S, ptr=None):
        return l.cbfssm_rigid_filter_f64(body, ptr, ptr, ptr, ptr, ptr, ptr, N, S, ptr, ptr, None)

    def bwd(body, N, S, ptr=None):
        return l.cbfssm_rigid_filter_bwd_f64(body, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, N, S, ptr, ptr, ptr, ptr, None)

    # negative sizes, no steps
    for call in (fwd, bwd):
        assert call(C.byref(rb), -1, 8, one) == -1 and l.cbfssm_last_error().decode()
        assert call(C.byref(rb), 37, 0, one) == -1 and call(C.byref(rb), 37, -1, one) == -1
        # too many chains or steps: -3 before any launch, even with plausible pointers
        assert call(C.byref(rb), 2 ** 30 + 1, 8, one) == -3 and l.cbfssm_last_error().decode()
        assert call(C.byref(rb), 37, 2 ** 24 + 1, one) == -3
        # null pointers, null body
        assert call(C.byref(rb), 37, 8) == -1 and b'null' in l.cbfssm_last_error()
        assert call(None, 37, 8, one) == -1 and b'null' in l.cbfssm_last_error()


def test_python_surface():
    from cbfssm.hip import autograd, voliro
    from cbfssm.utils.quaternions import Quaternion
    assert callable(autograd.rigid_filter) and callable(autograd.rigid_filter_eval)
    for name in ('multiply', 'multiply_np', 'invert', 'invert_np', 'pad_to_quat', 'rot_vec'):
        assert callable(getattr(Quaternion, name)), name
    for name in ('alloc_matrix', 'local_coord', 'force_torque', 'out_to_hidden', 'VoliroElbo'):
        assert callable(getattr(voliro, name)), name
    assert voliro.alloc_matrix().shape == (6, 12) and len(voliro.PARAM_NAMES) == 13
    for name in ('loss', 'predict_moments', 'parameters'):
        assert callable(getattr(voliro.VoliroElbo, name)), name
    # the model name stays unbuilt: this is the loss alone
    import pytest
    from cbfssm.model import Voliro
    with pytest.raises(NotImplementedError):
        Voliro({})
