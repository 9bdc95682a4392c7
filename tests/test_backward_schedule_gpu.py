"""The backward runs without their dead segment and with the adjoint's chunk table (cbfssm_bwd_schedule).

Run 1 resamples at t = R-1 (mod 2R) and writes y2 only where t mod 2R >= R (cbfssm.py:123-128): its last segment
t = R-1 .. 0 reaches nothing the loss sees, so the backward-pass kernels skip it and the adjoint has no chunk for it.
Every gradient comparison is against reverse-mode autodiff of the float64 restatement (oracle.cbfssm_torch_ref) at the
suite's tolerances (tests/test_hip_grad.py): loss 1e-9 relative, each gradient 1e-6 of its largest entry."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from cbfssm import synthetic as syn
from cbfssm.hip import lib, train

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (T, R): run 1 wholly dead (T < R, T = R), one written step of run 1 (T = R + 1), several chunks with a tapered tail
SMALL = [(2, 3), (3, 3), (4, 3), (7, 3), (9, 1), (23, 2), (41, 4)]


def _case(T, R, **kw):
    """workload, config, parameters (numpy), inputs and noise: 21 chains = two chain groups, the second ragged"""
    base = dict(M=20, B=3, S=7)
    base.update(kw)
    w = syn.tiny(T=T, recog_len=R, **base)
    p = syn.perturb_params(syn.make_params(w, seed=1), scale=0.1)
    u, y = syn.make_inputs(w)
    return w, w.model_config(), p, u, y, syn.make_noise(w)


@functools.lru_cache(maxsize=None)
def _oracle(T, R, cond, kw=()):
    from oracle import cbfssm_torch_ref as tref
    w, cfg, p, u, y, noise = _case(T, R, **dict(kw))
    return tref.loss_and_grads(cfg, p, u, y, noise, cond)


def _dev(p):
    return {k: torch.tensor(v, device=DEV) for k, v in p.items()}


def _check(loss, grads, scal, gref, rtol=1e-6):
    rel = abs(float(loss) - scal['loss']) / abs(scal['loss'])
    worst = 0.0
    for k in train.PARAM_NAMES:
        g, r = grads[k].cpu().numpy(), gref[k]
        assert g.shape == r.shape, k
        worst = max(worst, np.abs(g - r).max() / (np.abs(r).max() + 1e-300))
    print('loss rel %.2e, worst gradient error / largest entry %.2e' % (rel, worst))
    assert rel <= 1e-9
    for k in train.PARAM_NAMES:
        g, r = grads[k].cpu().numpy(), gref[k]
        assert np.abs(g - r).max() / (np.abs(r).max() + 1e-300) < rtol, k


@pytest.mark.parametrize('T,R,cond', [(T, R, True) for T, R in SMALL] + [(23, 2, False)])
def test_small_shapes_match_oracle(T, R, cond):
    w, cfg, p, u, y, noise = _case(T, R)
    eng = train.HipElboGrad(cfg, DEV)
    loss, grads, terms = eng.loss_and_grads(_dev(p), u, y, noise, condition=cond)
    assert float(terms['info']) == 0.0
    _check(loss, grads, *_oracle(T, R, cond))


C3_TILE = (('M', 100), ('dim_x', 14), ('dim_u', 7), ('dim_y', 7), ('B', 2), ('S', 20), ('k_factor', 50.),
           ('var_y', 0.05 ** 2))
STASH = (('M', 130), ('dim_x', 9), ('dim_u', 3), ('dim_y', 2), ('B', 2), ('S', 9), ('k_factor', 20.))


@pytest.mark.parametrize('T,R,kw,stash', [(12, 3, C3_TILE, False), (14, 3, STASH, True)], ids=['c3_tile', 'stash'])
def test_compiled_c3_tile_and_stash_mode_match_oracle(T, R, kw, stash):
    w, cfg, p, u, y, noise = _case(T, R, **dict(kw))
    eng = train.HipElboGrad(cfg, DEV)
    assert bool(eng.stash) == stash
    loss, grads, _ = eng.loss_and_grads(_dev(p), u, y, noise)
    _check(loss, grads, *_oracle(T, R, True, kw))


def test_adjoint_with_input_gradients_matches_oracle():
    """with input gradients the adjoint runs its `_in` kernels over the same table: the twelve parameter gradients are
    those of the plain adjoint to reordered-sum accuracy, and d loss / d u, d loss / d y are finite everywhere"""
    T, R = 23, 2
    w, cfg, p, u, y, noise = _case(T, R)
    eng = train.HipElboGrad(cfg, DEV)
    loss, grads, _ = eng.loss_and_grads(_dev(p), u, y, noise, input_grads=True)
    _check(loss, grads, *_oracle(T, R, True))
    assert torch.isfinite(grads['u']).all() and torch.isfinite(grads['y']).all()


def test_float32_tracks_the_float64_gradients():
    """tests/test_f32_gpu.py's tolerance for the two-triangular form: loss 2e-4, gradients 2e-3 of the largest entry"""
    T, R = 23, 2
    w, cfg, p, u, y, noise = _case(T, R)
    cfg['gp_form'] = 'tri'
    l64, g64, _ = train.HipElboGrad(cfg, DEV).loss_and_grads(_dev(p), u, y, noise)
    g64 = {k: v.cpu().numpy().copy() for k, v in g64.items()}
    l32, g32, t32 = train.HipElboGrad(cfg, DEV, dtype='float32').loss_and_grads(_dev(p), u, y, noise)
    assert float(t32['info']) == 0.0
    assert float(l32) == pytest.approx(float(l64), rel=2e-4)
    for k in train.PARAM_NAMES:
        err = np.abs(g32[k].cpu().numpy() - g64[k]).max() / np.abs(g64[k]).max()
        print(k, 'float32 against float64: %.2e' % err)
        assert err <= 2e-3, k


@pytest.mark.parametrize('T,R', [(2, 3), (4, 3), (23, 2)])
def test_dead_segment_rows_are_never_written_nor_read(T, R):
    """Through the C ABI: with h_all, fmv_b and the saved tiles prefilled with NaN, cbfssm_backward_pass_f64 leaves the rows
    (run 1, t < min(R, T)) of h_all / fmv_b as they were and writes every other row and all of y2; the adjoint on those
    buffers gives finite slabs (it reads no dead row, no dead tile), and the dead rows of gin_b read as exact zeros."""
    w, cfg, p, u, y, noise = _case(T, R)
    eng = train.HipElboGrad(cfg, DEV)
    ud, yd, prob, pflat, pp, c = eng._prepare(_dev(p), u, y, True)
    ws = eng._workspace(prob)
    lp = eng._loops(prob, ws, c, ud, yd, noise)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan = float('nan')
    assert ws.a2s_b is not None
    for t in (ws.h_all, ws.fmv_b, ws.a2s_b, ws.y2):
        t.fill_(nan)
    ws.ent_part.fill_(nan)
    lp.backward_pass(prob, st)
    torch.cuda.synchronize()
    dead = min(R, T)
    assert torch.isnan(ws.h_all[1, :dead]).all() and torch.isnan(ws.fmv_b[1, :dead]).all()
    assert torch.isfinite(ws.h_all[0]).all() and torch.isfinite(ws.h_all[1, dead:]).all()
    assert torch.isfinite(ws.fmv_b[0]).all() and torch.isfinite(ws.fmv_b[1, dead:]).all()
    assert torch.isfinite(ws.y2).all() and torch.isfinite(ws.ent_part).all()
    lp.forward_pass(prob, st)
    # the plain adjoint, then the one with input gradients, on the same buffers
    for with_inputs in (False, True):
        if with_inputs:
            lp.in_bufs = eng._input_buffers(prob, ws)
            for b in lp.in_bufs:
                b.fill_(nan)
        ws.gpart_b.fill_(nan)
        lp.forward_pass_bwd(prob, st)
        lp.backward_pass_bwd(prob, st)
        torch.cuda.synchronize()
        n_b = int(lib.load().cbfssm_rev_workgroups(C.byref(prob), 1))
        assert n_b == ws.n_b
        assert torch.isfinite(ws.gpart_b[:n_b * eng.slab_b]).all()
        if with_inputs:
            gin_b = lp.in_bufs[1][:2 * T * (w.dim_u + w.dim_y) * w.N].view(2, T, w.dim_u + w.dim_y, w.N)
            assert (gin_b[1, :dead] == 0.0).all()
            assert torch.isfinite(gin_b).all()


def test_two_calls_are_bitwise_equal_and_the_split_changes_no_bit(monkeypatch):
    T, R = 23, 2
    w, cfg, p, u, y, noise = _case(T, R)
    params = _dev(p)
    monkeypatch.setenv('CBFSSM_NO_SPLIT', '1')
    eng = train.HipElboGrad(cfg, DEV)
    l0, g0, _ = eng.loss_and_grads(params, u, y, noise, input_grads=True)
    g0 = {k: v.clone() for k, v in g0.items()}
    l1, g1, _ = eng.loss_and_grads(params, u, y, noise, input_grads=True)
    assert float(l0) == float(l1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    monkeypatch.delenv('CBFSSM_NO_SPLIT')
    monkeypatch.setenv('CBFSSM_SPLIT_MAIN', '1')
    eng2 = train.HipElboGrad(cfg, DEV)
    l2, g2, _ = eng2.loss_and_grads(params, u, y, noise, input_grads=True)
    assert float(l2) == float(l0)
    for k in g0:
        assert torch.equal(g0[k], g2[k]), k
