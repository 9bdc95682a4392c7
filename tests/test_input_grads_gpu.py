"""d loss / d u and d loss / d y from the HIP adjoints (HipElboGrad.loss_and_grads(..., input_grads=True), cbfssm.hip.autograd,
the model's grad_sample_in / grad_sample_out fetches) against reverse-mode autodiff of the float64 restatement
(oracle/cbfssm_torch_ref.elbo_step with u and y requiring grad).

Shapes: the eight of tests/test_input_adjoint_gpu.py (D = 7, 13, 16, 18, 21, 24, ragged chain groups and row blocks, M = 130
in stash mode), both `condition` values.  Tolerance: the rule of tests/test_hip_grad.py, every entry within 1e-6 of the largest
entry of its tensor -- on d loss / d u, d loss / d y, on the channels whose GP input row is j >= 16 on their own, and on the
twelve parameter gradients of the same call."""
import numpy as np
import pytest
import torch

from cbfssm.hip import train

import input_grads_cases as igc
from input_grads_cases import SHAPES, _setup, within_rule

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _params(p):
    return {k: torch.tensor(v, device=DEV) for k, v in p.items()}


@pytest.mark.parametrize('cond', [True, False])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_input_gradients_match_oracle(shape, cond):
    from test_hip_grad import _check
    w, cfg, p, u, y, noise = _setup(SHAPES[shape])
    scal, gref, gu_ref, gy_ref = igc.oracle_input_grads(cfg, p, u, y, noise, cond)
    igc.assert_reference_is_informative(gu_ref, gy_ref)
    eng = train.HipElboGrad(cfg, DEV)
    assert eng.stash == (w.M > 112)
    loss, grads, terms = eng.loss_and_grads(_params(p), u, y, noise, condition=cond, input_grads=True)
    assert float(terms['info']) == 0.0
    assert float(loss) == pytest.approx(scal['loss'], rel=1e-9)
    gu, gy = grads['u'].cpu().numpy(), grads['y'].cpu().numpy()
    tag = '%s cond=%d ' % (shape, cond)
    # printed before anything is asserted
    for name, g, r in (('u', gu, gu_ref), ('y', gy, gy_ref)):
        print('%s%s max|ref| %.3e err/max %.2e' % (tag, name, np.abs(r).max(), np.abs(g - r).max() / np.abs(r).max()))
    within_rule(tag + 'd loss/d u', gu, gu_ref)
    within_rule(tag + 'd loss/d y', gy, gy_ref)
    # the channels that sit in the second 16-row block of a GP's input, on their own: u is row dim_x + k of gp_f and row
    # dim_x - dim_y + k of gp_b, y is row dim_x - dim_y + dim_u + d of gp_b
    dob = w.dim_x - w.dim_y
    ku = max(0, 16 - w.dim_x)
    kb = max(0, 16 - dob)
    ky = max(0, 16 - dob - w.dim_u)
    if w.D > 16:
        assert ku < w.dim_u and ky < w.dim_y
        within_rule(tag + 'u rows j>=16 of gp_f', gu, gu_ref, sel=slice(ku, None))
        within_rule(tag + 'u rows j>=16 of gp_b', gu, gu_ref, sel=slice(kb, None))
        within_rule(tag + 'y rows j>=16 of gp_b', gy, gy_ref, sel=slice(ky, None))
    _check(grads, gref)


@pytest.mark.parametrize('cond', [True, False])
def test_chain_group_split_and_repeat_are_bitwise_invisible(monkeypatch, cond):
    kw = dict(SHAPES['a_D21_M100'], B=3, S=13)          # 39 chains = 3 groups of 16, the last one ragged
    w, cfg, p, u, y, noise = _setup(kw)
    params = _params(p)
    monkeypatch.setenv('CBFSSM_NO_SPLIT', '1')
    eng = train.HipElboGrad(cfg, DEV)
    _, g0, _ = eng.loss_and_grads(params, u, y, noise, condition=cond, input_grads=True)
    u0, y0 = g0['u'].clone(), g0['y'].clone()
    assert float(u0.abs().max()) > 0.0 and float(y0.abs().max()) > 0.0
    _, g1, _ = eng.loss_and_grads(params, u, y, noise, condition=cond, input_grads=True)       # two runs
    assert torch.equal(u0, g1['u']) and torch.equal(y0, g1['y'])
    monkeypatch.delenv('CBFSSM_NO_SPLIT')
    for main in (1, 2):
        monkeypatch.setenv('CBFSSM_SPLIT_MAIN', str(main))
        _, g2, _ = train.HipElboGrad(cfg, DEV).loss_and_grads(params, u, y, noise, condition=cond, input_grads=True)
        assert torch.equal(u0, g2['u']), main
        assert torch.equal(y0, g2['y']), main


@pytest.mark.parametrize('shape', ['d_D21_M130', 'd_D13_M130'])
def test_stash_mode_time_chunks_write_their_own_range_only(monkeypatch, shape):
    """a stash budget that holds one step (forward-pass adjoint) / one segment (backward runs) per launch: several
    time-chunked launches, the same bits as the single-chunk run"""
    from cbfssm.hip import ops
    w, cfg, p, u, y, noise = _setup(SHAPES[shape])
    params = _params(p)
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
    single = dict(calls)
    calls.update(f=0, b=0)
    cfg_small = dict(cfg, adjoint_stash_gib=1e-9)
    eng2 = train.HipElboGrad(cfg_small, DEV)
    _, g1, _ = eng2.loss_and_grads(params, u, y, noise, input_grads=True)
    print('launches single-chunk %s, small budget %s' % (single, calls))
    assert calls['f'] >= 3 and calls['b'] >= 2 and calls['f'] > single['f'] and calls['b'] > single['b']
    assert torch.equal(u0, g1['u']) and torch.equal(y0, g1['y'])


def _front(fr, u, y):
    return u * fr['gain'] + fr['bias_u'], y + fr['bias_y']


@pytest.mark.parametrize('cond', [True, False])
@pytest.mark.parametrize('shape', ['a_D21_M100', 'c_D7_M70', 'd_D13_M130'])
def test_autograd_trains_a_gain_and_bias_in_front_of_the_model(shape, cond):
    from cbfssm.hip.autograd import elbo_loss
    from test_hip_grad import _check
    w, cfg, p, u, y, noise = _setup(SHAPES[shape])
    rng = np.random.default_rng(5)
    fr = {'gain': 1.0 + 0.2 * rng.standard_normal(w.dim_u), 'bias_u': 0.1 * rng.standard_normal(w.dim_u),
          'bias_y': 0.05 * rng.standard_normal(w.dim_y)}
    scal, gref, _, _, gfr_ref = igc.oracle_input_grads(cfg, p, u, y, noise, cond, front=(fr, _front))
    eng = train.HipElboGrad(cfg, DEV)
    params = {k: torch.tensor(v, device=DEV, requires_grad=True) for k, v in p.items()}
    frt = {k: torch.tensor(v, device=DEV, requires_grad=True) for k, v in fr.items()}
    ut, yt = torch.tensor(np.asarray(u), device=DEV), torch.tensor(np.asarray(y), device=DEV)
    u2, y2 = _front(frt, ut, yt)
    loss = elbo_loss(eng, params, u2, y2, noise, cond)
    assert float(loss) == pytest.approx(scal['loss'], rel=1e-9)
    loss.backward()
    for k in ('gain', 'bias_u', 'bias_y'):
        within_rule('%s cond=%d %s' % (shape, cond, k), frt[k].grad.cpu().numpy(), gfr_ref[k])
    _check({k: params[k].grad for k in train.PARAM_NAMES}, gref)


def test_autograd_without_input_grads_is_the_default_call_bit_for_bit():
    from cbfssm.hip.autograd import elbo_loss
    w, cfg, p, u, y, noise = _setup(SHAPES['a_D21_M100'])
    eng = train.HipElboGrad(cfg, DEV)
    l0, g0, _ = eng.loss_and_grads(_params(p), u, y, noise)
    assert 'u' not in g0 and 'y' not in g0
    l0, g0 = float(l0), {k: g0[k].clone() for k in train.PARAM_NAMES}
    params = {k: torch.tensor(v, device=DEV, requires_grad=True) for k, v in p.items()}
    ut = torch.tensor(np.asarray(u), device=DEV, requires_grad=True)
    yt = torch.tensor(np.asarray(y), device=DEV)
    loss = elbo_loss(eng, params, ut, yt, noise, True, input_grads=False)
    loss.backward()
    assert float(loss) == l0 and ut.grad is None
    for k in train.PARAM_NAMES:
        assert torch.equal(params[k].grad, g0[k]), k
    # and the engine's own flag off, after a call with it on
    eng.loss_and_grads(_params(p), u, y, noise, input_grads=True)
    l1, g1, _ = eng.loss_and_grads(_params(p), u, y, noise, input_grads=False)
    assert float(l1) == l0
    for k in train.PARAM_NAMES:
        assert torch.equal(g1[k], g0[k]), k


def test_model_fetches_serve_the_loaded_mini_batch():
    from cbfssm.model import CBFSSM
    from cbfssm.model.session import Session
    w, cfg, p, u, y, noise = _setup(SHAPES['c_D7_M70'])
    cfg = dict(cfg, batch_size=w.B, shuffle=1, seed=3)
    model = CBFSSM(cfg)
    with model.graph.as_default(), Session(DEV) as sess:
        sess.run(model.init)
        model.load_ds(sess, np.asarray(u), np.asarray(y))
        gu, gy, loss = sess.run((model.grad_sample_in, model.grad_sample_out, model.loss), {model.condition: True})
    assert gu.shape == (w.B, w.T, w.dim_u) and gy.shape == (w.B, w.T, w.dim_y)
    assert np.isfinite(gu).all() and np.isfinite(gy).all() and np.abs(gu).max() > 0 and np.abs(gy).max() > 0
    assert np.isfinite(loss)


def test_refused_cases_raise_the_documented_error():
    from cbfssm.model import CBFSSMHALF, PRSSM
    from cbfssm.model.session import Session
    w, cfg, p, u, y, noise = _setup(SHAPES['c_D7_M70'])
    # float32 engines
    eng32 = train.HipElboGrad(cfg, DEV, dtype='float32')
    with pytest.raises(NotImplementedError, match='float64'):
        eng32.loss_and_grads(_params(p), u, y, noise, input_grads=True)
    # runs under a process group (refused before any collective)
    engd = train.HipElboGrad(cfg, DEV, dist=object())
    with pytest.raises(NotImplementedError, match='process group'):
        engd.loss_and_grads(_params(p), u, y, noise, input_grads=True)
    # the forward-only variants
    for cls, extra in ((CBFSSMHALF, {}), (PRSSM, {'recog_model': 'output'})):
        c2 = dict(cfg, batch_size=w.B, shuffle=1, seed=3, var_y=np.asarray([0.1] * w.dim_y), **extra)
        model = cls(c2)
        with model.graph.as_default(), Session(DEV) as sess:
            model.load_ds(sess, np.asarray(u), np.asarray(y))
            with pytest.raises(NotImplementedError, match='no input gradients'):
                sess.run(model.grad_sample_in, {model.condition: True})
