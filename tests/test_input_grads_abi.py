"""CPU-side checks of the input-gradient surface (d loss / d u, d loss / d y): the new C symbols are declared, exported and
listed; their sizing calls return 64-bit counts; the autograd wrapper imports without a device; and the inputs the GPU tests
use give a reference gradient that is nowhere trivially zero (oracle alone)."""
import ctypes
import os
import re

import numpy as np
import pytest

from cbfssm.hip import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('cbfssm_input_adjoint_fwd_elems', 'cbfssm_input_adjoint_bwd_elems', 'cbfssm_input_adjoint_obs_elems',
       'cbfssm_forward_pass_bwd_in_f64', 'cbfssm_backward_pass_bwd_in_f64', 'cbfssm_input_grads_f64')


def test_new_symbols_are_declared_listed_and_exported():
    text = open(os.path.join(ROOT, 'include', 'cbfssm_hip.h')).read()
    declared = set(re.findall(r'\b(cbfssm_[a-z0-9_]+)\s*\(', text))
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert name in lib.SYMBOLS, name
        assert hasattr(so, name), name
    # each declaration says what it replaces
    block = text[text.index('input gradients: d loss / d u'):text.index('cbfssm_input_grads_f64(')]
    assert 'tf.gradients' in block and 'base_model.py' in block


def test_sizing_calls_return_64_bit_counts():
    l = lib.load()
    for name in NEW[:3]:
        assert getattr(l, name).restype is ctypes.c_int64, name
    # a shape whose backward-run buffer has more than 2^31 entries: B S = 25600 chains, T = 3000, 21 data rows, two runs
    prob = lib.make_problem(512, 50, 3000, 14, 7, 14, 100, 50, 1.0, True)
    N = 512 * 50
    assert l.cbfssm_input_adjoint_fwd_elems(ctypes.byref(prob)) == 2999 * 7 * N
    nb = l.cbfssm_input_adjoint_bwd_elems(ctypes.byref(prob))
    assert nb == 2 * 3000 * 21 * N and nb > 2 ** 31
    assert l.cbfssm_input_adjoint_obs_elems(ctypes.byref(prob)) == 3000 * 14 * N
    assert l.cbfssm_input_adjoint_bwd_elems(None) == -1


def test_entry_points_refuse_the_forward_only_variants_on_the_host():
    l = lib.load()
    lay = lib.pack_layout(20, 5, 4)
    half = lib.make_problem(2, 3, 6, 4, 1, 2, 20, 3, 1.0, True, half=True)
    nul = [None] * 10
    rc = l.cbfssm_forward_pass_bwd_in_f64(ctypes.byref(half), ctypes.byref(lay), *nul, 1.0, None, None, 4, 0, None, None,
                                          None, 0, None, None, None)
    assert rc != 0 and b'input gradients' in l.cbfssm_last_error()


def test_autograd_module_imports_without_a_device():
    from cbfssm.hip import autograd
    assert callable(autograd.elbo_loss)
    with pytest.raises(KeyError):
        autograd.elbo_loss(None, {}, None, None, None)


@pytest.mark.parametrize('cond', [True, False])
def test_reference_input_gradients_are_nowhere_trivially_zero(cond):
    """the guard of the GPU comparison, confirmed with the oracle alone for every shape it uses"""
    import input_grads_cases as igc
    for shape in sorted(igc.SHAPES):
        w, cfg, p, u, y, noise = igc._setup(igc.SHAPES[shape])
        _, _, gu, gy = igc.oracle_input_grads(cfg, p, u, y, noise, cond)
        assert gu.shape == (w.B, w.T, w.dim_u) and gy.shape == (w.B, w.T, w.dim_y)
        igc.assert_reference_is_informative(gu, gy)
        assert np.isfinite(gu).all() and np.isfinite(gy).all()
