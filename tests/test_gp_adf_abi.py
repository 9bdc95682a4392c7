"""Host-side checks of the GPModel.adf / GPModel.ads entry points (no GPU): the three symbols are declared, exported and
bound, the count is 64-bit, and bad arguments are refused on the host -- the limits before any pointer is looked at --
before anything is launched."""
import ctypes as C
import os
import re

import pytest

from cbfssm.hip import lib
from test_gp_moment_match_abi import _broken

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT = 'cbfssm_gp_adf_work_elems'
ADF, ADS = 'cbfssm_gp_adf_f64', 'cbfssm_gp_ads_f64'
# in call order after the layout; `a`, P0, cond, var_x (and lag1 of ads) may be NULL
ADF_PTRS = ('pack', 'm0', 'P0', 'a', 'y', 'cond', 'var_x', 'var_y')
ADF_OUT = ('means', 'covs', 'loglik', 'pmeans', 'pcovs', 'cross')
ADS_OUT = ('smeans', 'scovs', 'sm_init', 'sP_init', 'lag1')
OPTIONAL = ('P0', 'cond', 'var_x', 'lag1')


def _call(l, name, lay, Dy, N, T, null=()):
    """the call with a (never dereferenced) pointer everywhere but at the names in `null`"""
    buf = (C.c_double * 4)()
    p = C.cast(buf, C.c_void_p)
    ptr = lambda k: None if (k in null or null == 'all') else p
    args = [C.byref(lay) if lay is not None else None] + [ptr(k) for k in ADF_PTRS] + [Dy, N, T] + [ptr(k) for k in ADF_OUT]
    if name == ADS:
        args += [ptr(k) for k in ADS_OUT]
    args += [ptr('info'), ptr('work'), None]
    return getattr(l, name)(*args)


def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, 'include', 'cbfssm_hip.h')).read()
    declared = set(re.findall(r'\b(cbfssm_[a-z0-9_]+)\s*\(', text))
    so = C.CDLL(lib.LIB_PATH)
    for name in (COUNT, ADF, ADS):
        assert name in declared and name in lib.SYMBOLS and hasattr(so, name), name
    l = lib.load()
    assert getattr(l, COUNT).restype is C.c_int64 and len(getattr(l, COUNT).argtypes) == 1
    assert getattr(l, ADF).restype is C.c_int and len(getattr(l, ADF).argtypes) == 21
    assert getattr(l, ADS).restype is C.c_int and len(getattr(l, ADS).argtypes) == 26
    # the header's parameter lists have the same lengths
    for name, n in ((ADF, 21), (ADS, 26)):
        m = re.search(r'\bint %s\(([^;]*)\);' % name, text)
        assert m and len(m.group(1).split(',')) == n, name


def test_the_count_is_64_bit():
    l = lib.load()
    for (M, D, Do), nblk in (((1, 1, 1), 1), ((100, 21, 14), 7), ((113, 9, 1), 10), ((320, 24, 16), 20)):
        lay = lib.pack_layout(M, D, Do)
        assert lay.NBLK == nblk
        # alpha = K^-1 mu, [16][16 NBLK], and the W_d tiles [Do][NBLK][NBLK][256]
        assert getattr(l, COUNT)(C.byref(lay)) == 16 * 16 * nblk + Do * nblk * nblk * 256
    assert getattr(l, COUNT)(None) == -1


@pytest.mark.parametrize('name', [ADF, ADS])
def test_limits_are_refused_before_any_pointer_is_read(name):
    l = lib.load()
    bad = [_broken('M', 321), _broken('D', 25), _broken('Do', 17), _broken('M', 0), _broken('NBLK', 3)]
    bad.append(lib.pack_layout(64, 2, 3))                               # D < Do: the transition does not exist
    for lay in bad:
        assert getattr(l, COUNT)(C.byref(lay)) == -1
        assert _call(l, name, lay, 1, 21, 5) == -3 and l.cbfssm_last_error().decode()
        assert _call(l, name, lay, 1, 21, 5, null='all') == -3
    good = lib.pack_layout(100, 21, 14)
    for Dy in (0, 15):                                                  # Dy outside 1..Do
        assert _call(l, name, good, Dy, 21, 5) == -3 and l.cbfssm_last_error().decode()
        assert _call(l, name, good, Dy, 21, 5, null='all') == -3


@pytest.mark.parametrize('name', [ADF, ADS])
def test_null_pointers_and_negative_sizes_are_refused(name):
    l = lib.load()
    good = lib.pack_layout(100, 21, 14)
    assert _call(l, name, None, 7, 21, 5) == -1
    outs = ADF_OUT + (ADS_OUT if name == ADS else ()) + ('info', 'work')
    for k in ADF_PTRS + outs:
        if k in OPTIONAL:
            continue                                                    # (a launch would follow: not tried without a device)
        assert _call(l, name, good, 7, 21, 5, null=(k,)) == -1 and l.cbfssm_last_error().decode(), k
        assert _call(l, name, good, 7, 0, 5, null=(k,)) == -1, k
    assert _call(l, name, good, 7, -1, 5) == -1 and l.cbfssm_last_error().decode()
    assert _call(l, name, good, 7, 21, -1) == -1
    assert _call(l, name, good, -1, 21, 5) == -1
    # a GP that takes the state alone needs no `a`
    alone = lib.pack_layout(30, 5, 5)
    assert _call(l, name, alone, 2, 0, 5, null=('a',)) == 0


@pytest.mark.parametrize('name', [ADF, ADS])
def test_nothing_to_do_returns_before_any_launch(name):
    l = lib.load()
    good = lib.pack_layout(100, 21, 14)
    assert _call(l, name, good, 7, 0, 5) == 0 and _call(l, name, good, 7, 21, 0) == 0
    assert _call(l, name, good, 7, 0, 5, null=OPTIONAL) == 0
