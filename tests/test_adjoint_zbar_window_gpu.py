"""The inducing-input adjoint Zbar~ += Ebar x~^T of the eight-wave adjoint tile (seven row blocks: M = 65 .. 112, float64, K^-1 adjoint in
registers) is not accumulated by the wave that owns the row block: every row-block wave leaves its rows of Ebar in the LDS
tile, and behind the barrier that releases the carry chain the waves 4 .. 6 and the eighth wave accumulate Zbar~ for all
seven row blocks by a compile-time deal table (cbfssm_adjoint.hpp: rev_zdeal).  The owner writes the slab tiles and its
term of the lengthscale rebuild of the input rows j >= 16.

Pinned here, against reverse-mode autodiff of the float64 restatement (oracle/cbfssm_torch_ref.py) with the rule of
tests/test_hip_grad.py (1e-6 of the largest entry of a tensor; loss to 1e-9):

  - M = 97 / 100 / 112: the last row block (dealt to wave 6) holds 1, 4 and 16 real rows; M = 70 is the control: it runs on
    the same seven-row-block tile (the next smaller one ends at M = 64), with five real row blocks -- the dealt waves also
    accumulate the two all-padding row blocks 5 and 6, whose rows of the (Z~)^T image are zero;
  - D = 21 (two input blocks, the rows j >= 16 rebuilt from Zbar~ behind the time loop), D = 13 (two blocks, ones row in
    block 0, nothing rebuilt), D = 7 (one block); B S = 21 chains: the last chain group is ragged;
  - launches and chunks of one step (T = 2, T = 3 with recog_len = 1: backward run 1 is wholly or partly dead) and a
    tapered tail of single segments (T = 7, recog_len = 3): the last step of a chunk must still reach the accumulators;
  - bit-for-bit: two evaluations, the chain-group split, and graph replay against eager launches of one train step."""
import numpy as np
import pytest
import torch

from cbfssm import synthetic as syn
from cbfssm.hip import train

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

SARCOS = dict(dim_x=14, dim_u=7, dim_y=7, k_factor=50., var_y=0.05 ** 2)
SHAPES = {
    'D21_M97': dict(M=97, T=12, recog_len=3, B=3, S=7, **SARCOS),
    'D21_M100': dict(M=100, T=12, recog_len=3, B=3, S=7, **SARCOS),
    'D21_M112': dict(M=112, T=12, recog_len=3, B=3, S=7, **SARCOS),
    'D13_M100': dict(M=100, dim_x=9, dim_u=4, dim_y=3, T=12, recog_len=3, B=3, S=7, k_factor=20.),
    'D7_M100': dict(M=100, dim_x=5, dim_u=2, dim_y=2, T=12, recog_len=3, B=3, S=7),
    'control_D21_M70': dict(M=70, T=12, recog_len=3, B=3, S=7, **SARCOS),
    # edges of the time range
    'T2_R1': dict(M=100, T=2, recog_len=1, B=3, S=7, **SARCOS),
    'T3_R1': dict(M=100, T=3, recog_len=1, B=3, S=7, **SARCOS),
    'T7_R3': dict(M=100, T=7, recog_len=3, B=3, S=7, **SARCOS),
}
_cache = {}


def _setup(name, **over):
    w = syn.tiny(loss_factors=(3., 0.7), **dict(SHAPES[name], **over))
    cfg = w.model_config()
    p = syn.perturb_params(syn.make_params(w, seed=2), scale=0.1)
    u, y = syn.make_inputs(w)
    noise = syn.make_noise(w)
    return w, cfg, p, u, y, noise


def _oracle(name, cond):
    """Computed once per (shape, condition), shared and left unchanged."""
    from oracle import cbfssm_torch_ref as tref
    if (name, cond) not in _cache:
        w, cfg, p, u, y, noise = _setup(name)
        _cache[(name, cond)] = tref.loss_and_grads(cfg, p, u, y, noise, cond)
    return _cache[(name, cond)]


@pytest.mark.parametrize('cond', [True, False])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_gradients_match_oracle(shape, cond):
    from test_hip_grad import _check
    w, cfg, p, u, y, noise = _setup(shape)
    assert (w.B * w.S) % 16 != 0                        # padded chains in the last group
    eng = train.HipElboGrad(cfg, DEV)
    assert not eng.stash
    params = {k: torch.tensor(v, device=DEV) for k, v in p.items()}
    loss, grads, terms = eng.loss_and_grads(params, u, y, noise, condition=cond)
    scal, gref = _oracle(shape, cond)
    for k in train.PARAM_NAMES:                         # printed before anything is asserted
        g, r = grads[k].cpu().numpy(), gref[k]
        print('%s cond=%d %-20s max|g| %.3e  err/max %.2e' % (shape, cond, k, np.abs(r).max(),
                                                               np.abs(g - r).max() / (np.abs(r).max() + 1e-300)))
    assert float(terms['info']) == 0.0
    assert float(loss) == pytest.approx(scal['loss'], rel=1e-9)
    if w.D > 16:
        # the rebuilt rows themselves: each entry of the lengthscale gradient of the rows j >= 16, not only the largest
        for gp in 'fb':
            k = gp + '.lengthscales_unc'
            g, r = grads[k].cpu().numpy().reshape(-1), gref[k].reshape(-1)
            assert np.abs(g[16:] - r[16:]).max() < 1e-6 * np.abs(r).max(), (k, g[16:], r[16:])
    _check(grads, gref)


@pytest.mark.parametrize('shape', ['D21_M100', 'T3_R1'])
def test_two_evaluations_agree_bit_for_bit(shape):
    w, cfg, p, u, y, noise = _setup(shape)
    params = {k: torch.tensor(v, device=DEV) for k, v in p.items()}
    eng = train.HipElboGrad(cfg, DEV)
    l1, g1, _ = eng.loss_and_grads(params, u, y, noise)
    l1, g1 = float(l1), {k: v.clone() for k, v in g1.items()}
    l2, g2, _ = eng.loss_and_grads(params, u, y, noise)
    assert float(l2) == l1
    for k in train.PARAM_NAMES:
        assert torch.equal(g1[k], g2[k]), k


@pytest.mark.parametrize('cond', [True, False])
def test_chain_group_split_stays_invisible(monkeypatch, cond):
    w, cfg, p, u, y, noise = _setup('D21_M100', B=3, S=13)      # 39 chains = 3 groups of 16, the last one ragged
    params = {k: torch.tensor(v, device=DEV) for k, v in p.items()}
    monkeypatch.delenv('CBFSSM_SPLIT_MAIN', raising=False)
    monkeypatch.setenv('CBFSSM_NO_SPLIT', '1')
    l0, g0, _ = train.HipElboGrad(cfg, DEV).loss_and_grads(params, u, y, noise, condition=cond)
    l0, g0 = float(l0), {k: v.clone() for k, v in g0.items()}
    monkeypatch.delenv('CBFSSM_NO_SPLIT')
    for main in (1, 2):
        monkeypatch.setenv('CBFSSM_SPLIT_MAIN', str(main))
        l1, g1, _ = train.HipElboGrad(cfg, DEV).loss_and_grads(params, u, y, noise, condition=cond)
        assert float(l1) == l0
        for k in train.PARAM_NAMES:
            assert torch.equal(g0[k], g1[k]), (main, k)


def test_graph_replay_and_eager_launches_give_the_same_parameters(monkeypatch):
    w, cfg, p, u, y, noise = _setup('D21_M100', B=3, S=13)
    out = {}
    for tag, env in (('eager', '0'), ('graph', '1')):
        monkeypatch.setenv('CBFSSM_HIP_GRAPH', env)
        st = train.HipTrainStep(cfg, {k: torch.tensor(v, device=DEV) for k, v in p.items()}, DEV)
        assert st.use_graph == (tag == 'graph')
        loss = float(st.step(u, y, noise))
        out[tag] = (loss, {k: st.params[k].clone() for k in train.PARAM_NAMES})
    for k in train.PARAM_NAMES:                         # printed before anything is asserted
        print('%-20s max|eager - graph| %.3e' % (k, float((out['eager'][1][k] - out['graph'][1][k]).abs().max())))
    assert out['eager'][0] == out['graph'][0]
    for k in train.PARAM_NAMES:
        assert torch.equal(out['eager'][1][k], out['graph'][1][k]), k
