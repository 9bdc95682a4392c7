"""GPU parity of the adjoint path: loss and d loss/d(12 unconstrained tensors) from the HIP kernels against the
golden fixtures (reverse-mode autodiff of the float64 CPU restatement, itself pinned by finite differences in
tests/test_oracle.py).  Tolerance: 1e-6 relative to the largest entry of each gradient tensor (north_star asks
1e-5 on the ELBO; gradients are not named there, they are held to the same order)."""
import os
import numpy as np
import pytest
import torch

from cbfssm import synthetic as syn
from cbfssm.hip import train

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
DEV = 'cuda:0'


def _check(grads, gref, rtol=1e-6):
    """every tensor within rtol of its largest reference entry; returns the worst achieved ratio"""
    worst = 0.0
    for k in train.PARAM_NAMES:
        g = grads[k].cpu().numpy()
        r = gref[k]
        assert g.shape == r.shape, k
        scale = np.abs(r).max() + 1e-300
        err = np.abs(g - r).max() / scale
        assert err < rtol, (k, err, g.reshape(-1)[:4], r.reshape(-1)[:4])
        worst = max(worst, err)
    return worst


@pytest.mark.parametrize('name', ['tiny', 'mini_smallscale', 'mini_sarcos'])
@pytest.mark.parametrize('cond', [True, False])
def test_grad_matches_golden(name, cond):
    from test_hip_parity import _load_golden
    z, w, p, noise = _load_golden(name)
    eng = train.HipElboGrad(w.model_config(), DEV)
    params = {k: torch.tensor(v, device=DEV) for k, v in p.items()}
    loss, grads, terms = eng.loss_and_grads(params, z['u'], z['y'], noise, condition=cond)
    tag = 'c1_' if cond else 'c0_'
    assert float(terms['info']) == 0.0
    assert float(loss) == pytest.approx(float(z[tag + 'loss']), rel=1e-9)
    _check(grads, {k: z[tag + 'grad_' + k] for k in train.PARAM_NAMES})


def test_grad_sarcos_tile_matches_oracle_and_is_deterministic():
    from oracle import cbfssm_torch_ref as tref
    w = syn.tiny(M=100, dim_x=14, dim_u=7, dim_y=7, T=12, B=2, S=20, recog_len=3, k_factor=50., var_y=0.05 ** 2,
                 loss_factors=(6., 0.5))
    cfg = w.model_config()
    p = syn.perturb_params(syn.make_params(w, seed=1), scale=0.1)
    u, y = syn.make_inputs(w)
    noise = syn.make_noise(w)
    eng = train.HipElboGrad(cfg, DEV)
    params = {k: torch.tensor(v, device=DEV) for k, v in p.items()}
    loss, grads, _ = eng.loss_and_grads(params, u, y, noise)
    scal, gref = tref.loss_and_grads(cfg, p, u, y, noise, True)
    assert float(loss) == pytest.approx(scal['loss'], rel=1e-9)
    _check(grads, gref)
    g1 = {k: v.clone() for k, v in grads.items()}
    loss2, grads2, _ = eng.loss_and_grads(params, u, y, noise)
    assert float(loss2) == float(loss)
    for k in train.PARAM_NAMES:
        assert torch.equal(g1[k], grads2[k]), k


def test_train_step_decreases_loss_and_matches_tf_adam_rule():
    w = syn.tiny(M=20, T=16, B=4, S=8, learning_rate=0.01)
    cfg = w.model_config()
    p = syn.make_params(w)
    u, y = syn.make_inputs(w)
    noise = syn.make_noise(w)
    step = train.HipTrainStep(cfg, {k: torch.tensor(v, device=DEV) for k, v in p.items()}, DEV)
    p0 = {k: v.clone() for k, v in step.params.items()}
    l0 = float(step.step(u, y, noise))
    # TF 1.8 rule at t = 1: lr_t = lr sqrt(1-b2)/(1-b1), m = (1-b1) g, v = (1-b2) g^2, p -= lr_t m / (sqrt(v) + eps)
    #   => p -= lr g / (|g| + eps / sqrt(1-b2))
    _, g0, _ = train.HipElboGrad(cfg, DEV).loss_and_grads(p0, u, y, noise)
    for k in train.PARAM_NAMES:
        expect = p0[k] - cfg['learning_rate'] * g0[k] / (g0[k].abs() + 1e-8 / (1 - 0.999) ** 0.5)
        assert torch.allclose(step.params[k], expect, rtol=0, atol=1e-12), k
    losses = [l0] + [float(step.step(u, y, noise)) for _ in range(10)]
    assert losses[-1] < losses[0]


@pytest.mark.parametrize('M', [70, 110])
def test_grad_seven_row_block_tiles_other_heights(M):
    """The seven-row-block tile (M = 65..112) away from the Sarcos height: M = 70 (18 k-steps: the general loop of the
    K^-1 A2bar product, untrimmed pass tiles) and M = 110 (the K^-1 image no longer fits the LDS next to the adjoint's tiles:
    streamed from L2) -- both with kept kernel tiles -- against reverse-mode autodiff of the restatement."""
    from oracle import cbfssm_torch_ref as tref
    w = syn.tiny(M=M, dim_x=14, dim_u=7, dim_y=7, T=11, B=2, S=12, recog_len=3, k_factor=50., var_y=0.05 ** 2,
                 loss_factors=(3., 0.7))
    cfg = w.model_config()
    p = syn.perturb_params(syn.make_params(w, seed=2), scale=0.1)
    u, y = syn.make_inputs(w)
    noise = syn.make_noise(w)
    eng = train.HipElboGrad(cfg, DEV)
    loss, grads, _ = eng.loss_and_grads({k: torch.tensor(v, device=DEV) for k, v in p.items()}, u, y, noise)
    scal, gref = tref.loss_and_grads(cfg, p, u, y, noise, True)
    assert float(loss) == pytest.approx(scal['loss'], rel=1e-9)
    _check(grads, gref)


@pytest.mark.parametrize('kw', [
    dict(M=20, T=13, B=2, S=8),
    dict(M=130, dim_x=9, dim_u=3, dim_y=2, T=14, B=2, S=9, recog_len=3, k_factor=20.),       # stash mode: dense K^-1 adjoint
])
def test_hip_train_tail_equals_tensor_library_tail(kw, monkeypatch):
    """cbfssm_train_tail_f64 (five launches) against the same adjoint written with torch ops (CBFSSM_TORCH_TAIL=1)."""
    monkeypatch.delenv('CBFSSM_TORCH_TAIL', raising=False)
    w = syn.tiny(loss_factors=(2., 0.4), **kw)
    cfg = w.model_config()
    p = {k: torch.tensor(v, device=DEV) for k, v in syn.perturb_params(syn.make_params(w, seed=3), scale=0.1).items()}
    u, y = syn.make_inputs(w)
    noise = syn.make_noise(w)
    eng = train.HipElboGrad(cfg, DEV)
    assert eng.fused_tail
    l1, g1, _ = eng.loss_and_grads(p, u, y, noise)
    g1 = {k: v.clone() for k, v in g1.items()}
    monkeypatch.setenv('CBFSSM_TORCH_TAIL', '1')
    eng2 = train.HipElboGrad(cfg, DEV)
    assert not eng2.fused_tail
    l2, g2, _ = eng2.loss_and_grads(p, u, y, noise)
    assert float(l1) == float(l2)
    for k in train.PARAM_NAMES:
        scale = float(g2[k].abs().max()) + 1e-300
        assert float((g1[k] - g2[k]).abs().max()) <= 1e-11 * scale, k


@pytest.mark.parametrize('split', [None, '1'])
def test_graph_captured_train_step_equals_eager(split, monkeypatch):
    """HipTrainStep replays one captured HIP graph per step (default); the eager path must give the same parameters,
    also with the chain-group split on two streams inside the capture and with fresh inputs every step."""
    if split:
        monkeypatch.setenv('CBFSSM_SPLIT_MAIN', split)
    w = syn.tiny(M=20, T=16, B=4, S=8, learning_rate=0.01)
    cfg = w.model_config()
    p = syn.make_params(w)
    mk = lambda graph: train.HipTrainStep(cfg, {k: torch.tensor(v, device=DEV) for k, v in p.items()}, DEV, graph=graph)
    sg, se = mk(True), mk(False)
    assert sg.use_graph and not se.use_graph
    for it in range(4):
        u, y = syn.make_inputs(w, seed=10 + it)
        noise = syn.make_noise(w, seed=20 + it)
        lg, le = float(sg.step(u, y, noise)), float(se.step(u, y, noise))
        assert abs(lg - le) <= 1e-12 * abs(le), (it, lg, le)
        for k in train.PARAM_NAMES:
            assert torch.allclose(sg.params[k], se.params[k], rtol=1e-12, atol=1e-14), (it, k)
    assert sg.opt.t == se.opt.t == 4 and float(sg.opt.t_dev) == 4.0


@pytest.mark.parametrize('kw,gib', [
    (dict(M=130, dim_x=9, dim_u=3, dim_y=2, T=14, B=2, S=9, recog_len=3, k_factor=20.), 4.0),       # tile height 10
    (dict(M=200, dim_x=14, dim_u=7, dim_y=7, T=11, B=1, S=20, recog_len=2, k_factor=50., var_y=0.05 ** 2), 4.0),   # C4 tile
    (dict(M=200, dim_x=14, dim_u=7, dim_y=7, T=11, B=1, S=20, recog_len=2, k_factor=50., var_y=0.05 ** 2), 3e-4),  # many launches
    (dict(M=250, dim_x=4, dim_u=2, dim_y=2, T=9, B=2, S=9, recog_len=50, k_factor=1.), 4.0),        # tile height 16, T < R
    (dict(M=300, dim_x=4, dim_u=2, dim_y=2, T=12, B=1, S=17, recog_len=2, k_factor=1.), 2e-4),      # C5 tile, chunked
])
def test_grad_stash_mode_matches_oracle(kw, gib):
    """M > 112: the K^-1-adjoint is contracted from stashed tiles by GEMMs, in several time chunks when the stash
    budget is small (gx_carry hand-off between launches)."""
    from oracle import cbfssm_torch_ref as tref
    w = syn.tiny(loss_factors=(2., 0.4), **kw)
    cfg = w.model_config()
    cfg['adjoint_stash_gib'] = gib
    p = syn.perturb_params(syn.make_params(w, seed=1), scale=0.1)
    u, y = syn.make_inputs(w)
    noise = syn.make_noise(w)
    eng = train.HipElboGrad(cfg, DEV)
    assert eng.stash
    params = {k: torch.tensor(v, device=DEV) for k, v in p.items()}
    loss, grads, _ = eng.loss_and_grads(params, u, y, noise)
    scal, gref = tref.loss_and_grads(cfg, p, u, y, noise, True)
    assert float(loss) == pytest.approx(scal['loss'], rel=1e-9)
    _check(grads, gref)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_chain_group_split_is_bitwise_identical(monkeypatch, dtype):
    """The two-stream chain-group split (hip/train.py:_split) must not change a single bit: chains are independent and
    every partial sum keeps its slot.  (float32: the float32 passes and adjoint take chain-group ranges too.)"""
    w = syn.tiny(M=20, T=19, B=5, S=11, recog_len=3)          # 55 chains = 4 groups of 16 (last one ragged)
    cfg = w.model_config()
    p = syn.perturb_params(syn.make_params(w))
    u, y = syn.make_inputs(w)
    noise = syn.make_noise(w)
    params = {k: torch.tensor(v, device=DEV) for k, v in p.items()}
    monkeypatch.setenv('CBFSSM_NO_SPLIT', '1')
    eng = train.HipElboGrad(cfg, DEV, dtype=dtype)
    l0, g0, _ = eng.loss_and_grads(params, u, y, noise)
    le0, _, ws0 = eng.forward(params, u, y, noise)
    x0 = ws0.x.clone()
    monkeypatch.delenv('CBFSSM_NO_SPLIT')
    for main in (1, 3):
        monkeypatch.setenv('CBFSSM_SPLIT_MAIN', str(main))
        eng2 = train.HipElboGrad(cfg, DEV, dtype=dtype)
        l1, g1, _ = eng2.loss_and_grads(params, u, y, noise)
        le1, _, ws1 = eng2.forward(params, u, y, noise)
        assert float(l1) == float(l0) and float(le1) == float(le0)
        assert torch.equal(ws1.x, x0)
        for k in train.PARAM_NAMES:
            assert torch.equal(g0[k], g1[k]), (main, k)
