"""cbfssm_reduce_partials_f64 on its own: out[i] = the sum over nwg slabs in a fixed order, single-stage below
nwg = 4 * 32 = 128 slabs and two-stage from there on, with the 32 stage-1 partial sums written to the scratch slabs the caller
reserves behind its nwg slabs (include/cbfssm_hip.h: CBFSSM_REDUCE_SPLIT).  Every gradient of every train step passes
through it; the batch sizes of the model-level tests never reach its second form."""
import math

import numpy as np
import pytest
import torch

from cbfssm.hip import lib, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CBFSSM_REDUCE_SPLIT = 32                                     # include/cbfssm_hip.h
GUARD, SENTINEL = 8, -7.25


def _slabs(kind, nwg, slab, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nwg, slab))
    if kind == 'cancelling':                                 # pairs +-1e8 plus N(0,1): the sum is of order sqrt(nwg), the terms 1e8
        big = 1e8 * rng.choice([-1.0, 1.0], size=(nwg // 2, slab))
        x[:2 * (nwg // 2):2] += big
        x[1:2 * (nwg // 2):2] -= big
    return x


def _exact_sum(x):
    """the sum over the slabs in long double where it carries 63 mantissa bits, else correctly rounded per element"""
    if np.finfo(np.longdouble).nmant >= 63:
        return np.sum(x.astype(np.longdouble), axis=0)
    return np.array([math.fsum(x[:, i]) for i in range(x.shape[1])])


def _reduce(x):
    """one call on a buffer of (nwg + 32) slabs between guard words, the scratch slabs pre-filled with NaN, out with a
    sentinel between guard words; returns (out, the buffer afterwards) with the guards checked"""
    nwg, slab = x.shape
    n = (nwg + CBFSSM_REDUCE_SPLIT) * slab
    buf = torch.full((n + 2 * GUARD,), float('nan'), dtype=torch.float64, device=DEV)
    buf[:GUARD] = SENTINEL
    buf[GUARD + n:] = SENTINEL
    buf[GUARD:GUARD + nwg * slab] = torch.tensor(x.reshape(-1), device=DEV)
    out = torch.full((slab + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=DEV)
    rc = lib.load().cbfssm_reduce_partials_f64(ops._ptr(buf[GUARD:]), slab, nwg, ops._ptr(out[GUARD:]), ops._stream())
    lib.check(rc, 'cbfssm_reduce_partials_f64')
    torch.cuda.synchronize()
    o, b = out.cpu().numpy(), buf.cpu().numpy()
    for g in (o, b):
        assert np.all(g[:GUARD] == SENTINEL) and np.all(g[-GUARD:] == SENTINEL), 'a guard word was written'
    return o[GUARD:-GUARD], b[GUARD:-GUARD]


@pytest.mark.parametrize('kind', ['normal', 'cancelling'])
@pytest.mark.parametrize('slab', [1, 255, 257, 1713])
@pytest.mark.parametrize('nwg', [1, 2, 127, 128, 129, 1000])
def test_sum_of_the_slabs(nwg, slab, kind):
    """|got - sum| <= (nwg - 1) 2^-53 sum_k |x_k| element-wise: the first-order bound of nwg - 1 float64 additions in any
    fixed order.  No NaN leaks from the scratch, the input slabs are read only, a second call gives the same bits."""
    x = _slabs(kind, nwg, slab, 1000 * nwg + slab)
    ref = _exact_sum(x)
    bound = (nwg - 1) * 2.0 ** -53 * np.abs(x).sum(axis=0)
    got, buf = _reduce(x)
    assert np.all(np.isfinite(got)), 'a scratch NaN (or the sentinel path) reached the result'
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    worst = float((err / bound).max()) if nwg > 1 else float(err.max())
    print('REDUCE_PARTIALS_RECORD nwg=%d slab=%d %s max err=%.3e worst err/bound=%.4f' % (nwg, slab, kind, err.max(), worst))
    assert np.all(err <= bound), (nwg, slab, kind, worst)
    assert np.array_equal(buf[:nwg * slab].reshape(nwg, slab), x), 'the reduction wrote into its input slabs'
    got2, _ = _reduce(x)
    assert np.array_equal(got, got2)


def test_refuses_bad_arguments():
    l = lib.load()
    buf = torch.zeros(64, dtype=torch.float64, device=DEV)
    for args in ((None, 1, 1, ops._ptr(buf)), (ops._ptr(buf), 1, 1, None), (ops._ptr(buf), 0, 1, ops._ptr(buf)),
                 (ops._ptr(buf), 1, 0, ops._ptr(buf))):
        assert l.cbfssm_reduce_partials_f64(*args, ops._stream()) != 0
        assert 'bad reduce arguments' in l.cbfssm_last_error().decode()
