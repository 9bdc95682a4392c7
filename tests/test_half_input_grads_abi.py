"""CPU-side checks of the forward-only variants' input-gradient surface (d loss / d u, d loss / d y of CBFSSMHALF and PR-SSM):
the new C symbols are declared, exported and listed; the host-side refusals of the new entry points answer before any launch;
cbfssm_forward_pass_bwd_in_f64 still refuses a half problem; the autograd wrapper imports without a device; and the
reference gradient of every set-up the GPU tests use has the structure those tests rely on (oracle alone)."""
import ctypes
import os
import re

import numpy as np
import pytest

from cbfssm.hip import lib

import half_input_grads_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('cbfssm_gru_recog_bwd_in_f64', 'cbfssm_conv_recog_bwd_in_f32', 'cbfssm_half_forward_pass_bwd_in_f64',
       'cbfssm_half_input_grads_f64')
ONE = ctypes.c_void_p(8)          # a non-null pointer that is never dereferenced: every call below is refused on the host


def test_new_symbols_are_declared_listed_and_exported():
    text = open(os.path.join(ROOT, 'include', 'cbfssm_hip.h')).read()
    declared = set(re.findall(r'\b(cbfssm_[a-z0-9_]+)\s*\(', text))
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert name in lib.SYMBOLS, name
        assert hasattr(so, name), name
        assert getattr(lib.load(), name).restype is ctypes.c_int, name
    # the declarations say what they replace
    block = text[text.index('input gradients of the forward-only variants'):text.index('int cbfssm_gru_recog_bwd_in_f64(')]
    assert 'tf.gradients' in block
    for ref in ('base_model.py:22-27', 'cbfssmhalf.py:82-93,117-199', 'prssm.py:96-157'):
        assert ref in block, ref


def test_the_cbfssm_entry_point_still_refuses_a_half_problem():
    l = lib.load()
    lay = lib.pack_layout(20, 5, 4)
    half = lib.make_problem(2, 3, 6, 4, 1, 2, 20, 3, 1.0, True, half=True)
    rc = l.cbfssm_forward_pass_bwd_in_f64(ctypes.byref(half), ctypes.byref(lay), *([None] * 10), 1.0, None, None, 4, 0, None,
                                          None, None, 0, None, None, None)
    assert rc != 0 and b'the forward-only variants have no input gradients' in l.cbfssm_last_error()


def _refused(rc, *words):
    msg = lib.load().cbfssm_last_error()
    assert rc != 0, 'accepted'
    assert any(w in msg for w in words), msg


def test_half_adjoint_entry_point_refusals():
    l = lib.load()
    lay = lib.pack_layout(20, 5, 4)
    full = lib.make_problem(2, 3, 6, 4, 1, 2, 20, 3, 1.0, True)
    half = lib.make_problem(2, 3, 6, 4, 1, 2, 20, 3, 1.0, True, half=True)

    def call(prob, gin_f=ONE, gyo=ONE, head=ONE, t_hi=4, t_lo=0, carry=None):
        return l.cbfssm_half_forward_pass_bwd_in_f64(ctypes.byref(prob) if prob is not None else None, ctypes.byref(lay),
                                                     *([head] * 9), 1.0, ONE, ONE, t_hi, t_lo, carry, None, None, 0, gin_f, gyo,
                                                     None)
    _refused(call(None), b'half must be 1')
    _refused(call(full), b'half must be 1')
    _refused(call(half, head=None), b'null pointer')
    _refused(call(half, gin_f=None), b'gin_f/gyo is null')
    _refused(call(half, gyo=None), b'gin_f/gyo is null')
    _refused(call(half, t_hi=5), b'bad step range')
    _refused(call(half, t_hi=2), b'gx_carry')


def test_reduction_entry_point_refusals():
    l = lib.load()
    lay = lib.pack_layout(20, 5, 4)
    half = lib.make_problem(2, 3, 6, 4, 1, 2, 20, 1, 1.0, False, half=True)
    full = lib.make_problem(2, 3, 6, 4, 1, 2, 20, 3, 1.0, True)

    def call(prob=half, pack=ONE, var_y=ONE, y=ONE, x=ONE, gin_f=ONE, gyo=ONE, gx0=None, gwin=ONE, R=3, gu=ONE, gy=ONE):
        return l.cbfssm_half_input_grads_f64(ctypes.byref(prob) if prob is not None else None, ctypes.byref(lay), pack, var_y,
                                             y, x, gin_f, gyo, gx0, gwin, R, 0.5, gu, gy, None)
    _refused(call(prob=None), b'null problem')
    _refused(call(prob=full), b'half must be 1')
    for k in ('pack', 'var_y', 'y', 'x', 'gin_f', 'gyo', 'gu', 'gy'):
        _refused(call(**{k: None}), b'null pointer')
    _refused(call(gx0=ONE, gwin=ONE), b'exactly one of gx0')
    _refused(call(gx0=None, gwin=None), b'exactly one of gx0')
    _refused(call(R=7), b'recog_len')              # recog_len > T
    _refused(call(R=0), b'recog_len')


def test_recogniser_entry_point_refusals():
    """limits and return codes are those of the weight-gradient calls; a null gwin is refused by the `_in` forms only"""
    l = lib.load()
    gru = lambda *d, gwin=ONE, u=ONE: l.cbfssm_gru_recog_bwd_in_f64(*d, u, ONE, ONE, ONE, ONE, ONE, gwin, None)   # noqa: E731
    conv = lambda *d, gwin=ONE, u=ONE: l.cbfssm_conv_recog_bwd_in_f32(*d, u, ONE, ONE, ONE, ONE, gwin, None)      # noqa: E731
    for fn, R in ((gru, 3), (conv, 4)):
        assert fn(2, 6, 1, 1, 4, R, gwin=None) == -1 and b'null pointer' in l.cbfssm_last_error()
        assert fn(2, 6, 1, 1, 4, R, u=None) == -1 and b'null pointer' in l.cbfssm_last_error()
        assert fn(2, 6, 1, 1, 4, 7) == -1 and b'recog_len exceeds' in l.cbfssm_last_error()
        assert fn(2, 6, 17, 16, 4, R) == -3
        assert fn(2, 6, 1, 1, 17, R) == -3
        assert fn(0, 6, 1, 1, 4, R) == -1
    assert conv(2, 6, 1, 1, 4, 3) == -1                       # conv: recog_len >= 4
    assert conv(2, 70, 1, 1, 4, 65) == -3


def test_autograd_module_imports_without_a_device():
    from cbfssm.hip import autograd
    assert callable(autograd.elbo_loss)
    with pytest.raises(KeyError):
        autograd.elbo_loss(None, {}, None, None, None)

    class Eng:                                               # a forward-only engine names its own tensors
        names = ('zeta_pos', 'var_x_unc')
    with pytest.raises(KeyError, match='zeta_pos, var_x_unc'):
        autograd.elbo_loss(Eng(), {}, None, None, None)


@pytest.mark.parametrize('name', sorted(hc.CASES))
def test_reference_input_gradients_have_the_expected_structure(name):
    """the guard of the GPU comparison, confirmed with the oracle alone for every set-up it uses: d loss / d y non-zero at every
    step, d loss / d u non-zero at every t <= T - 2 and exactly zero at t = T - 1 unless the window covers that row"""
    variant, w, cfg, p, u, y, noise = hc.setup(name)
    for cond in hc.CONDS(name):
        loss, gref, gu, gy = hc.oracle(name, cond)
        assert np.isfinite(loss)
        assert gu.shape == (w.B, w.T, w.dim_u) and gy.shape == (w.B, w.T, w.dim_y)
        hc.assert_reference_structure(name, cfg, gu, gy)
        R = hc.window_rows(cfg, w.T)
        print('%s cond=%d T=%d window=%d max|gu| window %.3e rest %.3e  max|gy| window %.3e rest %.3e'
              % (name, cond, w.T, R, np.abs(gu[:, :R]).max(initial=0.0), np.abs(gu[:, R:]).max(initial=0.0),
                 np.abs(gy[:, :R]).max(initial=0.0), np.abs(gy[:, R:]).max(initial=0.0)))
