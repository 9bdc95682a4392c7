"""The stash-mode contraction through the C ABI (cbfssm_stash_contract_f64) on random operand images: the symmetric form
(default: the lower-triangular blocks of sum A2bar K^T + K A2bar^T, expanded to the symmetric part of the sum -- all that
d loss / d K_mm = -K^-1 (.) K^-1 uses) and the full-matrix forms (CBFSSM_CONTRACT_FULL=1) against a float64 matrix product,
at the four tile heights that run in stash mode, with slot counts that do not divide the slice count (one slot: one slice;
200 slots: 24 slices of 9, the last one empty).  The work buffer comes with NaN in it and 64 doubles longer than the library
asks for: the result may not depend on what the buffer held, and the tail must still be NaN afterwards."""
import ctypes as C

import numpy as np
import pytest
import torch

from cbfssm.hip import lib, ops
from cbfssm.hip.train import _unpack_c

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dense(img, nblk, nslots):
    """operand image [slot][rb][s][lane] -> X (16 nblk, 16 nslots): X[16 rb + (lane & 15)][16 slot + 4 s + (lane >> 4)]"""
    v = img.view(nslots, nblk, 4, 4, 16)                    # slot, rb, s, g = lane >> 4, m = lane & 15
    return v.permute(1, 4, 0, 2, 3).reshape(16 * nblk, 16 * nslots)


GUARD = 64


def _contraction(M, nslots, forms, monkeypatch):
    l = lib.load()
    lay = lib.pack_layout(M, 6, 4)
    nblk = lay.NBLK
    assert lay.rev_stash == 1
    g = torch.Generator(device=DEV)
    g.manual_seed(M + nslots)
    sa = torch.randn(nslots * nblk * 256, dtype=torch.float64, device=DEV, generator=g)
    sk = torch.randn(nslots * nblk * 256, dtype=torch.float64, device=DEV, generator=g)
    B = _dense(sa, nblk, nslots) @ _dense(sk, nblk, nslots).T
    nwork = int(l.cbfssm_stash_contract_work_elems(C.byref(lay), nslots))
    for full, v1 in forms:
        want = B if full else 0.5 * (B + B.T)
        for key, on in (('CBFSSM_CONTRACT_FULL', full), ('CBFSSM_CONTRACT_V1', v1)):
            if on:
                monkeypatch.setenv(key, '1')
            else:
                monkeypatch.delenv(key, raising=False)
        work = torch.full((nwork + GUARD,), float('nan'), dtype=torch.float64, device=DEV)
        img = torch.full((nblk * nblk * 256,), 1.0, dtype=torch.float64, device=DEV)      # the call ADDS to the image
        for _ in range(2):
            lib.check(l.cbfssm_stash_contract_f64(C.byref(lay), ops._ptr(sa), ops._ptr(sk), nslots, ops._ptr(work),
                                                  ops._ptr(img), ops._stream()), 'contract')
        torch.cuda.synchronize()
        got = _unpack_c(img, nblk, nblk)
        err = float((got - (1.0 + 2.0 * want)).abs().max()) / float(want.abs().max())
        assert err < 1e-13, (M, nslots, full, v1, err)
        if not full:
            assert float((got - got.T).abs().max()) == 0.0                                # symmetric to the last bit
        assert bool(torch.isnan(work[nwork:]).all()), (M, nslots, full, v1)               # nothing written past work_elems


@pytest.mark.parametrize('M,nslots', [(150, 1), (150, 5), (200, 37), (200, 200), (200, 1000), (250, 19), (300, 23)])
def test_contraction_matches_a_matrix_product(M, nslots, monkeypatch):
    _contraction(M, nslots, ((False, False), (True, False)), monkeypatch)


@pytest.mark.parametrize('M,nslots', [(150, 5), (150, 200), (200, 37), (200, 200)])
def test_row_group_form_at_ten_and_thirteen_row_blocks(M, nslots, monkeypatch):
    """CBFSSM_CONTRACT_FULL=1 with CBFSSM_CONTRACT_V1=1: stash_contract_kernel where the one-workgroup form would run"""
    assert lib.pack_layout(M, 6, 4).NBLK == (10 if M == 150 else 13)
    _contraction(M, nslots, ((True, True),), monkeypatch)
