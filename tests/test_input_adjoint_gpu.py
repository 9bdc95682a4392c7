"""The input adjoint of the reverse time loops when the GP input spans two 16-row blocks (D + 1 > 16 rows with the ones
row): only block 0 -- every state row -- goes through the per-step MFMAs, the column sums of Ebar are summed in the lanes,
and the lengthscale adjoint of the input rows j >= 16 is rebuilt after the time loop from the Z-adjoint accumulator:

    sum_{t,n} xbar~[j,n] x~[j,n]  =  sum_m z~[m,j] Zbar~[m][j]  -  sum_{t,n} colsum(Ebar)[n] x~[j,n]^2

What the golden full-length and tile-height tests do not pin is pinned here, against reverse-mode autodiff of the float64
restatement (oracle/cbfssm_torch_ref.py) with the rule of tests/test_hip_grad.py (1e-6 of the largest entry of a tensor):

  (a) D >= 17 with B S not a multiple of 16: the rebuilt rows exist and padded chains exist (their Ebar columns must
      not reach the Z-adjoint accumulator the rebuild reads);
  (b) D = 13 .. 16 (four k-steps of the input dimension): two blocks, but the ones row sits in block 0 (D < 16) or is
      the only row of block 1 (D = 16) and no input row is rebuilt;
  (c) D <= 8: one block, the unchanged code path;
  (d) M = 70 / 100 / 130: the last row block is ragged, the in-lane column sum has to mask its padding rows (the
      kernel tile is finite but not zero there); 130 is the stash-mode tile with two row blocks per wave.

Both values of `condition`; all twelve gradients are compared, so lengthscales, inducing inputs and kernel variance of
both GPs are among them.  The chain-group split must stay bitwise invisible for shape (a)."""
import numpy as np
import pytest
import torch

from cbfssm import synthetic as syn
from cbfssm.hip import train

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

SARCOS = dict(k_factor=50., var_y=0.05 ** 2, recog_len=3)
SHAPES = {
    # (a) D = 21 (the Sarcos class) and D = 18, ragged last chain group
    'a_D21_M100': dict(M=100, dim_x=14, dim_u=7, dim_y=7, T=12, B=3, S=7, **SARCOS),
    'a_D18_M70': dict(M=70, dim_x=12, dim_u=6, dim_y=5, T=11, B=3, S=7, **SARCOS),
    'a_D24_M20': dict(M=20, dim_x=16, dim_u=8, dim_y=6, T=9, B=1, S=19, **SARCOS),      # D at the interface limit
    # (b) four k-steps: the ones row inside block 0 / alone in block 1
    'b_D13_M100': dict(M=100, dim_x=9, dim_u=4, dim_y=3, T=12, B=2, S=9, recog_len=3, k_factor=20.),
    'b_D16_M70': dict(M=70, dim_x=11, dim_u=5, dim_y=4, T=11, B=2, S=9, recog_len=3, k_factor=20.),
    # (c) one block
    'c_D7_M70': dict(M=70, dim_x=5, dim_u=2, dim_y=2, T=11, B=3, S=7),
    # (d) on the stash-mode tile (two row blocks per wave, the last wave owns one ragged block)
    'd_D21_M130': dict(M=130, dim_x=14, dim_u=7, dim_y=7, T=10, B=3, S=7, **SARCOS),
    'd_D13_M130': dict(M=130, dim_x=9, dim_u=4, dim_y=3, T=10, B=3, S=7, recog_len=3, k_factor=20.),
}
INPUT_ADJOINT_PARAMS = ('f.zeta_pos', 'f.variance_unc', 'f.lengthscales_unc',
                        'b.zeta_pos', 'b.variance_unc', 'b.lengthscales_unc')


def _setup(kw):
    w = syn.tiny(loss_factors=(3., 0.7), **kw)
    cfg = w.model_config()
    p = syn.perturb_params(syn.make_params(w, seed=2), scale=0.1)
    u, y = syn.make_inputs(w)
    noise = syn.make_noise(w)
    return w, cfg, p, u, y, noise


@pytest.mark.parametrize('cond', [True, False])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_input_adjoint_gradients_match_oracle(shape, cond):
    from oracle import cbfssm_torch_ref as tref
    from test_hip_grad import _check
    w, cfg, p, u, y, noise = _setup(SHAPES[shape])
    assert (w.B * w.S) % 16 != 0                        # padded chains in the last group
    eng = train.HipElboGrad(cfg, DEV)
    assert eng.stash == (w.M > 112)
    params = {k: torch.tensor(v, device=DEV) for k, v in p.items()}
    loss, grads, terms = eng.loss_and_grads(params, u, y, noise, condition=cond)
    scal, gref = tref.loss_and_grads(cfg, p, u, y, noise, cond)
    assert float(terms['info']) == 0.0
    assert float(loss) == pytest.approx(scal['loss'], rel=1e-9)
    for k in INPUT_ADJOINT_PARAMS:                      # printed before anything is asserted
        g, r = grads[k].cpu().numpy(), gref[k]
        print('%s cond=%d %-20s max|g| %.3e  err/max %.2e' % (shape, cond, k, np.abs(r).max(),
                                                               np.abs(g - r).max() / (np.abs(r).max() + 1e-300)))
    if w.D > 16:
        # the rebuilt rows themselves: each entry of the lengthscale gradient of the rows j >= 16, not only the largest
        for gp in 'fb':
            k = gp + '.lengthscales_unc'
            g, r = grads[k].cpu().numpy().reshape(-1), gref[k].reshape(-1)
            assert np.abs(g[16:] - r[16:]).max() < 1e-6 * np.abs(r).max(), (k, g[16:], r[16:])
    _check(grads, gref)


@pytest.mark.parametrize('cond', [True, False])
def test_chain_group_split_stays_bitwise_identical_with_two_input_blocks(monkeypatch, cond):
    kw = dict(SHAPES['a_D21_M100'], B=3, S=13)          # 39 chains = 3 groups of 16, the last one ragged
    w, cfg, p, u, y, noise = _setup(kw)
    params = {k: torch.tensor(v, device=DEV) for k, v in p.items()}
    monkeypatch.setenv('CBFSSM_NO_SPLIT', '1')
    l0, g0, _ = train.HipElboGrad(cfg, DEV).loss_and_grads(params, u, y, noise, condition=cond)
    g0 = {k: v.clone() for k, v in g0.items()}
    monkeypatch.delenv('CBFSSM_NO_SPLIT')
    for main in (1, 2):
        monkeypatch.setenv('CBFSSM_SPLIT_MAIN', str(main))
        l1, g1, _ = train.HipElboGrad(cfg, DEV).loss_and_grads(params, u, y, noise, condition=cond)
        assert float(l1) == float(l0)
        for k in train.PARAM_NAMES:
            assert torch.equal(g0[k], g1[k]), (main, k)


@pytest.mark.parametrize('no_blds', [False, True])
def test_input_adjoint_with_streamed_kinv_at_seven_row_blocks(monkeypatch, no_blds):
    """M = 110, D = 21: with one block of partial tiles per wave the K^-1 image fits the LDS up to M = 112, so the
    variant of the seven-row-block kernel that streams it from L2 is reached through CBFSSM_NO_BLDS only -- both are held."""
    from oracle import cbfssm_torch_ref as tref
    from test_hip_grad import _check
    if no_blds:
        monkeypatch.setenv('CBFSSM_NO_BLDS', '1')
    else:
        monkeypatch.delenv('CBFSSM_NO_BLDS', raising=False)
    w, cfg, p, u, y, noise = _setup(dict(SHAPES['a_D21_M100'], M=110))
    eng = train.HipElboGrad(cfg, DEV)
    loss, grads, _ = eng.loss_and_grads({k: torch.tensor(v, device=DEV) for k, v in p.items()}, u, y, noise)
    scal, gref = tref.loss_and_grads(cfg, p, u, y, noise, True)
    assert float(loss) == pytest.approx(scal['loss'], rel=1e-9)
    _check(grads, gref)


def test_input_adjoint_gradient_is_reproducible():
    """The rebuild sums over the row-block waves through LDS in wave order: two evaluations agree bit for bit."""
    w, cfg, p, u, y, noise = _setup(SHAPES['a_D21_M100'])
    params = {k: torch.tensor(v, device=DEV) for k, v in p.items()}
    eng = train.HipElboGrad(cfg, DEV)
    _, g1, _ = eng.loss_and_grads(params, u, y, noise)
    g1 = {k: v.clone() for k, v in g1.items()}
    _, g2, _ = eng.loss_and_grads(params, u, y, noise)
    for k in train.PARAM_NAMES:
        assert torch.equal(g1[k], g2[k]), k
