"""CPU-side checks of the conv recognition entry points (reference cbfssm/model/prssm.py:146-157): the element count is host
arithmetic, and both compute entry points decide their limits on the host, before anything is launched (null device
pointers throughout: no GPU needed)."""
import ctypes

import pytest

from cbfssm.hip import lib


def _elems(dim_u, dim_y, dim_x, R):
    return int(lib.load().cbfssm_conv_recog_param_elems(dim_u, dim_y, dim_x, R))


@pytest.mark.parametrize('dims,want', [((1, 1, 4, 16), 179), ((7, 7, 14, 16), 719), ((2, 2, 5, 17), 245), ((1, 1, 2, 4), 47)])
def test_param_elems_is_the_size_of_the_four_tensors(dims, want):
    dim_u, dim_y, dim_x, R = dims
    n_in, P = dim_u + dim_y, (R - 2) // 2
    assert 15 * n_in + 5 + 5 * P * dim_x + dim_x == want
    assert _elems(*dims) == want
    assert lib.load().cbfssm_conv_recog_param_elems.restype is ctypes.c_int64


@pytest.mark.parametrize('dims,want', [((1, 1, 4, 3), -1), ((1, 0, 4, 16), -1), ((1, 1, 4, 65), -3), ((1, 1, 17, 16), -3)])
def test_param_elems_reports_bad_dimensions_and_limits(dims, want):
    assert _elems(*dims) == want


# (B, T, dim_u, dim_y, dim_x, recog_len), what the message says; every pointer is null, so nothing can be launched
BAD = [
    ('recog_len > T', (2, 10, 1, 1, 4, 16), 'sequence length'),
    ('recog_len = 3', (2, 10, 1, 1, 4, 3), 'bad dimensions'),
    ('null params', (2, 20, 1, 1, 4, 16), 'null pointer'),
    ('dim_x = 17', (2, 20, 1, 1, 17, 16), 'limits'),
]


@pytest.mark.parametrize('what,dims,says', BAD, ids=[b[0] for b in BAD])
def test_compute_entry_points_refuse_on_the_host(what, dims, says):
    l = lib.load()
    for fn, tail in ((l.cbfssm_conv_recog_f32, (None, None)), (l.cbfssm_conv_recog_bwd_f32, (None, None, None))):
        rc = fn(*dims, None, None, None, *tail)
        assert rc != 0, (what, fn.__name__)
        msg = l.cbfssm_last_error().decode()
        assert msg and says in msg, (what, fn.__name__, msg)


@pytest.mark.parametrize('workload', ['C2', 'C3'])
def test_synthetic_conv_parameters_fill_the_flat_vector(workload):
    """the initial values of synthetic.make_variant_params(.., 'prssm', 'conv') are the four tensors in CONV_NAMES order, as
    the last entries of the parameter dict, with exactly the element count the kernels take"""
    from cbfssm import synthetic as syn
    from cbfssm.hip.train_half import CONV_NAMES, half_param_names
    w = syn.WORKLOADS[workload]
    cfg, p = syn.make_variant_params(w, 'prssm', 'conv')
    assert tuple(p) == half_param_names(cfg, 'prssm') and tuple(p)[-4:] == CONV_NAMES
    assert p['recog.conv_kernel'].shape == (3, w.dim_u + w.dim_y, 5)
    assert sum(p[k].size for k in CONV_NAMES) == _elems(w.dim_u, w.dim_y, w.dim_x, w.recog_len)
