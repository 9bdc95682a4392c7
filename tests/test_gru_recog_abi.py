"""CPU-side checks of the GRU recognition entry points (reference cbfssm/model/cbfssmhalf.py:82-93): the element counts are
host arithmetic, both compute entry points decide their limits on the host, before anything is launched (null device
pointers throughout: no GPU needed) -- and the fixtures of tests/test_gru_recog_gpu.py are well conditioned, so that
the tolerances derived there measure the kernel and not the reference."""
import ctypes

import numpy as np
import pytest

from cbfssm.hip import lib
from test_gru_recog_gpu import A_MAX, CAP, CASES, EPS64, FACTOR, H, NAMES, _case, _restate, _rule


@pytest.mark.parametrize('dims', [(0, 1, 1), (1, 1, 4), (7, 7, 14), (8, 15, 16), (16, 16, 16), (31, 1, 2)])
def test_param_elems_is_the_size_of_the_six_tensors(dims):
    dim_u, dim_y, dim_x = dims
    n_in = dim_u + dim_y
    fn = lib.load().cbfssm_gru_recog_param_elems
    assert fn.restype is ctypes.c_int64
    assert int(fn(*dims)) == (n_in + 16) * 48 + 48 + 16 * dim_x + dim_x


@pytest.mark.parametrize('B,R', [(1, 1), (3, 4), (129, 64), (40000, 1000)])
def test_act_elems_is_four_vectors_a_step_and_the_final_state(B, R):
    fn = lib.load().cbfssm_gru_recog_act_elems
    assert fn.restype is ctypes.c_int64
    assert int(fn(B, R)) == B * R * 64 + B * 16              # (the last one is past 2^31: 64-bit arithmetic)


def test_elems_report_bad_dimensions_and_know_no_upper_limit():
    """-1 for dimensions that are no recognition model at all; the counts themselves have no upper limit (the compute entry
    points refuse dim_u + dim_y > 32 and dim_x > 16), as include/cbfssm_hip.h says"""
    l = lib.load()
    for dims in ((-1, 1, 4), (1, 0, 4), (1, 1, 0)):
        assert int(l.cbfssm_gru_recog_param_elems(*dims)) == -1, dims
    for dims in ((0, 3), (2, 0), (-1, -1)):
        assert int(l.cbfssm_gru_recog_act_elems(*dims)) == -1, dims
    assert int(l.cbfssm_gru_recog_param_elems(17, 16, 4)) == (33 + 16) * 48 + 48 + 16 * 4 + 4
    assert int(l.cbfssm_gru_recog_param_elems(1, 1, 17)) == (2 + 16) * 48 + 48 + 16 * 17 + 17


# (B, T, dim_u, dim_y, dim_x, recog_len), what the message says; every pointer is null, so nothing can be launched
BAD = [
    ('dim_u + dim_y = 33', (2, 10, 17, 16, 4, 3), 'limits'),
    ('dim_x = 17', (2, 10, 1, 1, 17, 3), 'limits'),
    ('recog_len > T', (2, 3, 1, 1, 4, 4), 'sequence length'),
    ('dim_y = 0', (2, 10, 1, 0, 4, 3), 'bad dimensions'),
    ('recog_len = 0', (2, 10, 1, 1, 4, 0), 'bad dimensions'),
    ('null params', (2, 10, 1, 1, 4, 3), 'null pointer'),
    ('null params, no u', (2, 10, 0, 1, 4, 3), 'null pointer'),
]


@pytest.mark.parametrize('what,dims,says', BAD, ids=[b[0] for b in BAD])
def test_compute_entry_points_refuse_on_the_host(what, dims, says):
    l = lib.load()
    for fn, tail in ((l.cbfssm_gru_recog_f64, (None, None, None)), (l.cbfssm_gru_recog_bwd_f64, (None, None, None, None))):
        rc = fn(*dims, None, None, None, *tail)
        assert rc != 0, (what, fn.__name__)
        msg = l.cbfssm_last_error().decode()
        assert msg and says in msg, (what, fn.__name__, msg)


@pytest.mark.parametrize('variant', ['half', 'prssm'])
@pytest.mark.parametrize('workload', ['C2', 'C3'])
def test_synthetic_gru_parameters_fill_the_flat_vector(workload, variant):
    """the initial values of synthetic.make_variant_params(.., 'rnn') are the six tensors in RECOG_NAMES order, as the last
    entries of the parameter dict, with exactly the element count the kernels take"""
    from cbfssm import synthetic as syn
    from cbfssm.hip.train_half import RECOG_NAMES, half_param_names
    w = syn.WORKLOADS[workload]
    cfg, p = syn.make_variant_params(w, variant, 'rnn')
    assert tuple(p) == half_param_names(cfg, variant) and tuple(p)[-6:] == RECOG_NAMES
    n_in = w.dim_u + w.dim_y
    shapes = ((n_in + 16, 32), (32,), (n_in + 16, 16), (16,), (16, w.dim_x), (w.dim_x,))
    assert tuple(p[k].shape for k in RECOG_NAMES) == shapes
    assert sum(p[k].size for k in RECOG_NAMES) == int(lib.load().cbfssm_gru_recog_param_elems(w.dim_u, w.dim_y, w.dim_x))


@pytest.mark.parametrize('name', list(CASES))
def test_fixture_is_well_conditioned(name):
    """the condition the GPU tests assert first, here without a GPU: every amplification A (float32 oracle against float64
    oracle, in units of 2^-24) of x0 and of the six gradient tensors is <= 64, and the rule stays below its cap.  Where
    long double carries 63 mantissa bits, the float64 oracle and the float64 restatement themselves sit inside the
    GPU tests' bound against an 80-bit evaluation of the same lines: the bound is wide enough for a correct float64
    coding, so what it measures on the GPU is the kernel."""
    case = _case(name)
    A = case['A']
    print('GRU_RECOG_RECORD cpu case=%s A: %s' % (name, ' '.join('%s=%.2f' % kv for kv in A.items())))
    assert max(A.values()) <= A_MAX, A
    assert _rule(max(A.values())) < CAP and FACTOR * A_MAX * EPS64 < CAP
    assert np.abs(case['x0_restated'] - case['x0']).max() <= 4 * 2.0 ** -52 * np.abs(case['x0']).max()
    if np.finfo(np.longdouble).nmant < 63:
        return
    fx = case['fx']
    x0_t, act_t, hR_t = _restate(fx, np.longdouble)
    B, R = fx['B'], fx['R']
    pairs = [('x0 (oracle)', case['x0'], x0_t), ('x0 (restated)', case['x0_restated'], x0_t), ('h_final', case['hR'], hR_t)]
    pairs += [('act.' + blk, case['act'].reshape(B, R, 4, H)[:, :, j], act_t.reshape(B, R, 4, H)[:, :, j])
              for j, blk in enumerate('hruc')]
    for what, got, truth in pairs:
        scale = float(np.abs(truth).max())
        err = float(np.abs(got.astype(np.longdouble) - truth).max())
        if scale == 0.0:
            assert err == 0.0, what
            continue
        print('GRU_RECOG_RECORD cpu case=%s %s float64-against-80-bit: %.2f ulp of the largest entry, err/bound=%.4f'
              % (name, what, err / (EPS64 * scale), err / (_rule(A['x0']) * scale)))
        assert err <= _rule(A['x0']) * scale, (what, err / (_rule(A['x0']) * scale))


def test_names_follow_the_documented_flat_order():
    """the test's flat vector is the header's: gate kernel, gate bias, candidate kernel, candidate bias, dense kernel, bias"""
    fx = _case('odd')['fx']
    n_in = fx['n_in']
    assert [fx[k].shape for k in NAMES] == [(n_in + 16, 32), (32,), (n_in + 16, 16), (16,), (16, fx['dim_x']), (fx['dim_x'],)]
