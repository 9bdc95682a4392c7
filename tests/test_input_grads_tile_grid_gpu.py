"""The input-gradient adjoint (launch_revin_n: rev_kernel<..., IG = true>, 96 compiled kernels of which 72 can be launched;
tests/test_tile_grid_cpu.py proves that the rows below reach every one of them) at every row of tests/tile_grid.py, path by
path.

d loss / d u and d loss / d y are sums of the paths of DESIGN 3.2a, and the 1e-6-of-the-largest-entry rule on the sum does
not see a path that is 1e-3 of it.  So the paths are rebuilt from the per-chain buffers the engine keeps
(eng.last_ws.in_bufs = (gin_f, gin_b, gyo)) and each is held to 1e-6 of the largest entry of ITS OWN reference tensor
(input_grads_cases.oracle_path_grads; tests/test_input_grads_tile_grid_cpu.py proves every path tensor informative in
every channel and step):

    u_f   1/l_f sum_s gin_f                          u through gp_f, written by the MODE_FWD kernels
    u_b   1/l_b sum_s (gin_b[0] + gin_b[1]), u rows  u through gp_b, written by the MODE_BWD kernels
    y_b   the same, y rows                           y through gp_b
    y_o   grads['y'] - y_b                           gyo + the log-likelihood term

Tolerances are the suite's: loss 1e-9, the twelve parameter gradients by test_hip_grad._check, d loss / d u and d loss / d y
by input_grads_cases.within_rule (also on the channels with GP input row j >= 16 on their own), the forward-only variant by
tests/test_half_input_grads_gpu.py::_judge_reference.  Every test starts from a fresh engine and prints what it achieved
before it asserts (lines starting with IG_GRID_RECORD, HALF_IN_RECORD for the forward-only rows;
profiles/input_grads_tile_grid/README.md holds one run).  Nothing skips."""
import numpy as np
import pytest
import torch

from cbfssm.hip import ops, train

import input_grads_cases as igc
from input_grads_cases import within_rule
import tile_grid as tg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

GRID = [(n, True) for n in tg.CASE_IDS] + [(n, False) for n in tg.GRAD_NOCOND_CASES]


def _dev(p):
    return {k: torch.tensor(v, device=DEV) for k, v in p.items()}


def _path_case(name, cond, tag):
    from test_hip_grad import _check
    w, cfg, p, u, y, noise = tg.setup(tg.CASE_KW[name])
    cfg['gp_form'] = 'dense'
    scal, gref, ref = igc.tile_grid_path_reference(name, cond)
    igc.assert_paths_are_informative(name, ref)
    gu_ref, gy_ref = ref['u_f'] + ref['u_b'], ref['y_o'] + ref['y_b']
    eng = train.HipElboGrad(cfg, DEV)
    assert eng.stash == (w.M > 112) and eng.pack_f.gp_form() == 'dense'
    params = _dev(p)
    loss, grads, terms = eng.loss_and_grads(params, u, y, noise, condition=cond, input_grads=True)
    assert float(terms['info']) == 0.0
    loss = float(loss)
    g = {k: v.cpu().numpy().copy() for k, v in grads.items()}
    bufs = [b.cpu().numpy().copy() for b in eng.last_ws.in_bufs]
    gu, gy = g['u'], g['y']
    got = igc.paths_from_buffers(w, p, eng.last_ws.in_bufs, gy)
    tag = 'IG_GRID_RECORD %s%s M=%d D=%d cond=%d ' % (tag, name, w.M, w.D, cond)

    def rel(a, r):
        return np.abs(a - r).max() / (np.abs(r).max() + 1e-300)
    # printed before anything is asserted
    print('%sloss rel %.1e worst parameter gradient %.1e whole u %.1e whole y %.1e | paths %s' % (
        tag, abs(loss - scal['loss']) / abs(scal['loss']), max(rel(g[k], gref[k]) for k in train.PARAM_NAMES),
        rel(gu, gu_ref), rel(gy, gy_ref), ' '.join('%s %.1e' % (k, rel(got[k], ref[k])) for k in igc.PATHS)))
    assert loss == pytest.approx(scal['loss'], rel=1e-9)
    _check(grads, gref)
    within_rule(tag + 'd loss/d u', gu, gu_ref)
    within_rule(tag + 'd loss/d y', gy, gy_ref)
    for k, what in igc.PATHS.items():
        within_rule(tag + what, got[k], ref[k])
    # the rebuilt u paths add up to the engine's own d loss / d u (the test reads the buffers as the library does)
    within_rule(tag + 'u_f + u_b against grads[u]', got['u_f'] + got['u_b'], gu)
    assert not got['u_f'][:, -1].any()
    if w.D > 16:
        # the channels in the second 16-row block of a GP's input, on their own: u is row dim_x + k of gp_f and row
        # dim_x - dim_y + k of gp_b, y is row dim_x - dim_y + dim_u + d of gp_b (tests/test_input_grads_gpu.py) -- on the
        # whole tensors and on the path that owns the rows
        dob = w.dim_x - w.dim_y
        ku, kb, ky = max(0, 16 - w.dim_x), max(0, 16 - dob), max(0, 16 - dob - w.dim_u)
        assert ku < w.dim_u and ky < w.dim_y
        within_rule(tag + 'u rows j>=16 of gp_f', gu, gu_ref, sel=slice(ku, None))
        within_rule(tag + 'u rows j>=16 of gp_b', gu, gu_ref, sel=slice(kb, None))
        within_rule(tag + 'y rows j>=16 of gp_b', gy, gy_ref, sel=slice(ky, None))
        within_rule(tag + 'path u_f rows j>=16', got['u_f'], ref['u_f'], sel=slice(ku, None))
        within_rule(tag + 'path u_b rows j>=16', got['u_b'], ref['u_b'], sel=slice(kb, None))
        within_rule(tag + 'path y_b rows j>=16', got['y_b'], ref['y_b'], sel=slice(ky, None))
    # a second evaluation: the same bits, in the results and in the per-chain buffers
    loss2, grads2, _ = eng.loss_and_grads(params, u, y, noise, condition=cond, input_grads=True)
    assert float(loss2) == loss
    for k in g:
        assert np.array_equal(grads2[k].cpu().numpy(), g[k]), k
    for b0, b1 in zip(bufs, eng.last_ws.in_bufs):
        assert np.array_equal(b1.cpu().numpy(), b0)


@pytest.mark.parametrize('name,cond', GRID)
def test_input_gradients_path_by_path(name, cond, monkeypatch):
    monkeypatch.delenv('CBFSSM_NO_BLDS', raising=False)
    _path_case(name, cond, '')


@pytest.mark.parametrize('name', tg.IG_NO_BLDS_CASES)
def test_input_gradients_with_streamed_kinv_at_one_two_and_four_row_blocks(name, monkeypatch):
    """the K^-1 placement no shape reaches at these heights (with IG the image always fits there)"""
    monkeypatch.setenv('CBFSSM_NO_BLDS', '1')
    _path_case(name, True, 'streamed ')


@pytest.mark.parametrize('name', tg.IG_STASH_CHUNK_CASES)
def test_stash_mode_time_chunks_at_thirteen_sixteen_and_twenty_row_blocks(name, monkeypatch):
    """a stash budget that holds one step (forward-pass adjoint) / one segment (backward runs) per launch: several
    time-chunked launches, the bits of the single-chunk run (tests/test_input_grads_gpu.py holds this at ten row blocks)"""
    w, cfg, p, u, y, noise = tg.setup(tg.CASE_KW[name])
    params = _dev(p)
    calls = {'f': 0, 'b': 0}
    f0, b0 = ops.TimeLoops.forward_pass_bwd, ops.TimeLoops.backward_pass_bwd

    def cf(self, *a, **k):
        calls['f'] += 1
        return f0(self, *a, **k)

    def cb(self, *a, **k):
        calls['b'] += 1
        return b0(self, *a, **k)
    monkeypatch.setattr(ops.TimeLoops, 'forward_pass_bwd', cf)
    monkeypatch.setattr(ops.TimeLoops, 'backward_pass_bwd', cb)
    eng = train.HipElboGrad(cfg, DEV)
    assert eng.stash
    _, g0, _ = eng.loss_and_grads(params, u, y, noise, input_grads=True)
    u0, y0 = g0['u'].clone(), g0['y'].clone()
    bufs0 = [b.clone() for b in eng.last_ws.in_bufs]
    single = dict(calls)
    calls.update(f=0, b=0)
    eng2 = train.HipElboGrad(dict(cfg, adjoint_stash_gib=1e-9), DEV)
    _, g1, _ = eng2.loss_and_grads(params, u, y, noise, input_grads=True)
    print('IG_GRID_RECORD chunks %s M=%d launches single-chunk %s, small budget %s' % (name, w.M, single, calls))
    assert calls['f'] >= 3 and calls['b'] >= 2 and calls['f'] > single['f'] and calls['b'] > single['b']
    assert float(u0.abs().max()) > 0.0 and float(y0.abs().max()) > 0.0
    assert torch.equal(u0, g1['u']) and torch.equal(y0, g1['y'])
    for b0_, b1 in zip(bufs0, eng2.last_ws.in_bufs):
        assert torch.equal(b0_, b1)


# ---- forward-only variants: the MODE_FWD kernels with RevArgs::half ------------------------------------------------------
_HALF_REF = {}


def _forward_only_case(name, variant, cond):
    import half_input_grads_cases as hc
    from cbfssm.hip.train_half import HipHalfGrad, half_param_names
    from test_half_input_grads_gpu import _judge_reference
    from test_oracle import _half_setup, _prssm_setup
    w, cfg, p, u, y, noise = (_prssm_setup if variant == 'prssm' else _half_setup)('rnn', **tg.CASE_KW[name])
    if (name, variant, cond) not in _HALF_REF:
        _HALF_REF[(name, variant, cond)] = hc.oracle_run(variant, cfg, p, u, y, noise, cond)
    eng = HipHalfGrad(cfg, DEV, variant=variant)
    assert eng.stash == (w.M > 112) and eng.fused_gru
    loss, grads, terms = eng.loss_and_grads(_dev(p), u, y, noise, condition=cond, input_grads=True)
    assert float(terms['info']) == 0.0
    assert set(grads) == set(half_param_names(cfg, variant)) | {'u', 'y'}
    _judge_reference(name, variant, _HALF_REF[(name, variant, cond)], cond, cfg, w, loss, grads,
                     tag='tile grid %s M=%d D=%d ' % (variant, w.M, w.D))


@pytest.mark.parametrize('cond', [True, False])
@pytest.mark.parametrize('name', tg.IG_HALF_CASES)
def test_forward_only_variant_input_gradients(name, cond, monkeypatch):
    for k in ('CBFSSM_TORCH_GRU', 'CBFSSM_GP_FORM', 'CBFSSM_NO_BLDS'):
        monkeypatch.delenv(k, raising=False)
    _forward_only_case(name, 'half', cond)


@pytest.mark.parametrize('name', tg.IG_PRSSM_CASES)
def test_prssm_input_gradients_above_ten_row_blocks(name, monkeypatch):
    for k in ('CBFSSM_TORCH_GRU', 'CBFSSM_GP_FORM', 'CBFSSM_NO_BLDS'):
        monkeypatch.delenv(k, raising=False)
    _forward_only_case(name, 'prssm', True)
