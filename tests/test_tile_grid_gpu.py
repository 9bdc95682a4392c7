"""The parity grid: every row of tests/tile_grid.py -- one per compiled leaf of the time-loop kernels, the completeness is
proved by tests/test_tile_grid_cpu.py -- against the CPU oracle, with the tolerances the suite already holds the same
quantities to (the helpers of the tests that own them are called, not restated):

    GP predict                  rtol 1e-8, atol 1e-11            test_hip_parity._check_prepare_and_predict
    float64 forward             loss 1e-9, trajectories 1e-8     test_hip_edges._run
    float64 gradient            1e-6 of the largest entry        test_hip_grad._check, + the last data row block alone
    kept / recomputed tiles     1e-12 of the largest entry       (test_workspace_gpu, M = 20 and 100 only there)
    float32 forward, gradient   2e-4 / 2e-3 against float64 HIP  test_f32_gpu._check_elbo_f32_tracks_f64
    forward-only variant        1e-9 / 1e-8 / 1e-6               test_half_gpu._check_half
    skewed two-block passes     as the float64 forward           test_hip_parity._compare, on the trimmed tiles

Every test starts from a fresh engine and prints what it achieved before it asserts (pytest -s shows it; the worst values
per block are recorded in profiles/tile_grid/README.md).  Nothing here skips: the share of the table a GPU run may leave out
is zero."""
import numpy as np
import pytest
import torch

from cbfssm.hip import ops, train
import tile_grid as tg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

_REF = {}     # (row, condition) -> (scalars, gradients) of the autograd restatement
_G64 = {}     # (row, form) -> (loss, gradients) of the float64 HIP adjoint, condition = True

KT12_CASES = [n for n in tg.CASE_IDS if 100 < tg.CASE_KW[n]['M'] <= 108]
KEPT_CASES = [n for n in tg.CASE_IDS if tg.CASE_KW[n]['M'] <= 112]
GRAD_CASES = [(n, True) for n in tg.CASE_IDS] + [(n, False) for n in tg.GRAD_NOCOND_CASES]


def _grad_ref(name, condition):
    from oracle import cbfssm_torch_ref as tref
    if (name, condition) not in _REF:
        w, cfg, p, u, y, noise = tg.setup(tg.CASE_KW[name])
        _REF[(name, condition)] = tref.loss_and_grads(cfg, p, u, y, noise, condition)
    return _REF[(name, condition)]


def _dev(p):
    return {k: torch.tensor(v, device=DEV) for k, v in p.items()}


def _hip_grads(name, form, condition=True, dtype='float64'):
    """(loss, gradients as numpy, engine, device parameters, inputs) of a fresh engine"""
    w, cfg, p, u, y, noise = tg.setup(tg.CASE_KW[name])
    cfg['gp_form'] = form
    eng = train.HipElboGrad(cfg, DEV, dtype=dtype)
    params = _dev(p)
    loss, grads, terms = eng.loss_and_grads(params, u, y, noise, condition=condition)
    assert float(terms['info']) == 0.0
    assert eng.pack_f.gp_form() == form and eng.pack_b.gp_form() == form
    return float(loss), {k: v.cpu().numpy().copy() for k, v in grads.items()}, eng, params, (u, y, noise)


@pytest.mark.parametrize('form', ['dense', 'tri'])
@pytest.mark.parametrize('name', tg.CASE_IDS)
def test_gp_predict(name, form):
    from test_hip_parity import _check_prepare_and_predict
    w, cfg, p, u, y, noise = tg.setup(tg.CASE_KW[name])
    _check_prepare_and_predict(w, p, form)


@pytest.mark.parametrize('form', ['dense', 'tri'])
@pytest.mark.parametrize('condition', [True, False])
@pytest.mark.parametrize('name', tg.CASE_IDS)
def test_forward_f64(name, condition, form):
    from test_hip_edges import _run
    _run(tg.CASE_KW[name], condition=condition, grads=False, scale=tg.PERTURB_SCALE, form=form)


def _gradient_case(name, condition, form, keep=False):
    from test_hip_grad import _check
    w = tg.workload(tg.CASE_KW[name])
    scal, gref = _grad_ref(name, condition)
    loss, g, eng, params, (u, y, noise) = _hip_grads(name, form, condition)
    # the slices where padding and trimming act, against the bound of their whole tensor: the largest entry of a tensor
    # usually sits elsewhere
    lo, hi = tg.last_data_block(w.M)
    slices = {}
    for gp in 'fb':
        slices[gp + '.lengthscales_unc'] = slice(None)
        for k in ('zeta_pos', 'zeta_mean', 'zeta_var_unc'):
            slices['%s.%s' % (gp, k)] = slice(lo, hi)
    errs = {}
    for k, sl in slices.items():
        errs[k] = (np.abs(g[k][sl] - gref[k][sl]).max() / (np.abs(gref[k]).max() + 1e-300),
                   np.abs(g[k][sl] - gref[k][sl]).max() / (np.abs(gref[k][sl]).max() + 1e-300))
    full = max(np.abs(g[k] - gref[k]).max() / (np.abs(gref[k]).max() + 1e-300) for k in train.PARAM_NAMES)
    print('gradient %s M=%d condition=%d form=%s: loss rel %.1e, worst tensor %.1e, rows %d..%d of the zeta tensors and the '
          'lengthscales %.1e of the tensor maximum (%.1e of their own)' % (
              name, w.M, condition, form, abs(loss - scal['loss']) / abs(scal['loss']), full, lo, hi - 1,
              max(e[0] for e in errs.values()), max(e[1] for e in errs.values())))
    assert loss == pytest.approx(scal['loss'], rel=1e-9)
    _check({k: torch.as_tensor(v) for k, v in g.items()}, gref)
    for k, (err, _) in errs.items():
        assert err < 1e-6, (k, err)
    loss2, grads2, _ = eng.loss_and_grads(params, u, y, noise, condition=condition)
    assert float(loss2) == loss
    for k in train.PARAM_NAMES:
        assert np.array_equal(grads2[k].cpu().numpy(), g[k]), k
    if keep and condition:
        _G64[(name, form)] = (loss, g)


@pytest.mark.parametrize('form', ['dense', 'tri'])
@pytest.mark.parametrize('name,condition', GRAD_CASES)
def test_gradient_f64(name, condition, form):
    _gradient_case(name, condition, form, keep=True)


@pytest.mark.parametrize('name', tg.NO_BLDS_CASES)
def test_gradient_f64_with_streamed_kinv_at_seven_row_blocks(name, monkeypatch):
    """the side of launch_rev_k's LDS-or-streamed switch that no M reaches at DK = 4 and DK = 6"""
    monkeypatch.setenv('CBFSSM_NO_BLDS', '1')
    _gradient_case(name, True, 'dense')


@pytest.mark.parametrize('name', KEPT_CASES)
def test_kept_kernel_tiles_give_the_gradient_of_the_recomputing_adjoint(name, monkeypatch):
    monkeypatch.delenv('CBFSSM_NO_SAVE_K', raising=False)
    l1, g1, e1, _, _ = _hip_grads(name, 'dense')
    n_kept = e1.tile_pool.bytes()
    monkeypatch.setenv('CBFSSM_NO_SAVE_K', '1')
    l2, g2, e2, _, _ = _hip_grads(name, 'dense')
    assert e2.tile_pool.bytes() * 2 == n_kept                      # the record is [A2 | K] resp. [A2]
    assert l1 == l2
    print('kept tiles %s: worst %.1e' % (name, max(np.abs(g1[k] - g2[k]).max() / max(np.abs(g2[k]).max(), 1e-300) for k in g1)))
    for k in g1:
        np.testing.assert_allclose(g1[k], g2[k], rtol=0, atol=1e-12 * max(np.abs(g2[k]).max(), 1e-300), err_msg=k)


@pytest.mark.parametrize('condition', [True, False])
@pytest.mark.parametrize('name', tg.CASE_IDS)
def test_forward_f32(name, condition):
    from test_f32_gpu import _check_elbo_f32_tracks_f64
    _check_elbo_f32_tracks_f64(tg.CASE_KW[name], condition, form='tri')


@pytest.mark.parametrize('name', tg.CASE_IDS)
def test_gradient_f32(name):
    """the float32 adjoint in the form a float32 engine selects by itself, against the float64 HIP adjoint"""
    if (name, 'tri') not in _G64:
        _G64[(name, 'tri')] = _hip_grads(name, 'tri')[:2]
    l64, g64 = _G64[(name, 'tri')]
    l32, g32, _, _, _ = _hip_grads(name, 'tri', dtype='float32')
    errs = {k: np.abs(g32[k] - g64[k]).max() / np.abs(g64[k]).max() for k in train.PARAM_NAMES}
    print('float32 gradient %s: loss rel %.1e, worst tensor %.1e' % (name, abs(l32 - l64) / abs(l64), max(errs.values())))
    assert l32 == pytest.approx(l64, rel=2e-4)
    for k, err in errs.items():
        assert err <= 2e-3, (k, err)


@pytest.mark.parametrize('condition', [True, False])
@pytest.mark.parametrize('name', tg.HALF_CASES)
def test_forward_only_variant(name, condition):
    from test_half_gpu import _check_half
    _check_half('rnn', tg.CASE_KW[name], condition)


@pytest.mark.parametrize('name', KT12_CASES)
def test_skewed_pass_variant_on_trimmed_tiles(name, monkeypatch):
    """pass_kernel_skew<..., KT = 1 | 2> (opt-in: CBFSSM_NC_FWD / CBFSSM_NC_BWD = 2), the dense form"""
    from oracle import cbfssm_oracle as orc
    from test_hip_parity import _compare
    monkeypatch.setenv('CBFSSM_NC_FWD', '2')
    monkeypatch.setenv('CBFSSM_NC_BWD', '2')
    w, cfg, p, u, y, noise = tg.setup(tg.CASE_KW[name])
    cfg['gp_form'] = 'dense'
    eng = ops.HipElbo(cfg, DEV)
    eng.prepare(p)
    _compare(eng.run(u, y, noise, condition=True), w, orc.elbo_step(cfg, p, u, y, noise, True))
