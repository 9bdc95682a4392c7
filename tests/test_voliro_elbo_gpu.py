"""cbfssm.hip.voliro.VoliroElbo on the GPU against the float64 CPU restatement of the whole Voliro loss
(tests/voliro_cases.py, which states the inputs and the rules: scalars 1e-9 relative, pred_mean / pred_var within 1e-8
of their largest entry, every gradient entry within 1e-6 of its tensor's largest entry)."""
import numpy as np
import pytest
import torch

import voliro_cases as vc
from voliro_cases import CASES, LEAVES, TERMS, within_rule, traj_rule, scalar_rule

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64, device=DEV)


def _engine(cfg, leaves):
    """a VoliroElbo carrying the case's parameters as leaves that require grad; returns (engine, dict by LEAVES name)"""
    from cbfssm.hip import voliro
    eng = voliro.VoliroElbo(cfg, DEV, seed=0)
    assert voliro.PARAM_NAMES == LEAVES
    for gp, pre in ((eng.gp_f, 'gp_f.'), (eng.gp_b, 'gp_b.')):
        gp.zeta_pos, gp.zeta_mean, gp.zeta_var_unc = (_dev(leaves[pre + k]) for k in ('zeta_pos', 'zeta_mean', 'zeta_var_unc'))
        gp.kern.variance_unc, gp.kern.lengthscales_unc = _dev(leaves[pre + 'variance_unc']), _dev(leaves[pre + 'lengthscales_unc'])
    eng.var_x_unc, eng.var_y_unc, eng.var_z_unc = (_dev(leaves[k]) for k in ('var_x_unc', 'var_y_unc', 'var_z_unc'))
    eng.requires_grad_()
    params = eng.parameters()
    assert len(params) == 13
    return eng, dict(zip(LEAVES, params))


def test_initial_values_follow_the_config():
    from cbfssm.hip import voliro
    from cbfssm.hip.ops import tf_forward
    cfg = vc.config(20, 7)
    eng = voliro.VoliroElbo(cfg, DEV, seed=3)
    shapes = [tuple(p.shape) for p in eng.parameters()]
    assert shapes == [(20, 12), (20, 3), (20, 3), (1,), (12,), (20, 19), (20, 6), (20, 6), (1,), (19,), (13,), (13,), (6,)]
    np.testing.assert_allclose(tf_forward(eng.var_x_unc).cpu().numpy(), cfg['var_x'], rtol=1e-12)
    np.testing.assert_allclose(tf_forward(eng.var_y_unc).cpu().numpy(), cfg['var_y'], rtol=1e-12)
    np.testing.assert_allclose(tf_forward(eng.var_z_unc).cpu().numpy(), cfg['var_z'], rtol=1e-12)
    np.testing.assert_allclose(eng.gp_b.kern.lengthscales.cpu().numpy(), [5.0] * 19, rtol=1e-12)


@pytest.mark.parametrize('case', CASES, ids=str)
def test_loss_terms_moments_and_gradients(case):
    ref = vc.reference(case)
    cfg, leaves, si, so, noise = vc.make_case(case)
    eng, lv = _engine(cfg, leaves)
    loss, terms = eng.loss(si, so, noise)
    assert loss.grad_fn is not None and loss.shape == () and set(terms) == set(TERMS)
    scalar_rule('loss', float(loss.detach()), ref['loss'])
    for k in TERMS:
        scalar_rule(k, float(terms[k].detach()), ref[k])
    pm, pv = eng.predict_moments()
    B, S, T, M = case
    assert pm.shape == (B, T, 13) and pv.shape == (B, T, 13) and pm.grad_fn is None
    traj_rule('pred_mean', pm.cpu().numpy(), ref['pred_mean'])
    traj_rule('pred_var', pv.cpu().numpy(), ref['pred_var'])
    loss.backward()
    for k in LEAVES:
        assert lv[k].grad is not None, k
        within_rule(k, lv[k].grad.cpu().numpy(), ref['g_' + k])


def test_device_inputs_and_pipeline_noise_shapes():
    """device tensors are taken as they are, and one NoisePipeline draw has the three noise arrays"""
    from cbfssm.hip import ops, voliro
    case = CASES[0]
    B, S, T, M = case
    ref = vc.reference(case)
    cfg, leaves, si, so, noise = vc.make_case(case)
    eng, _ = _engine(cfg, leaves)
    with torch.no_grad():
        loss, _ = eng.loss(_dev(si), _dev(so), {k: _dev(v) for k, v in noise.items()})
    assert loss.grad_fn is None
    scalar_rule('loss', float(loss), ref['loss'])
    pipe = ops.NoisePipeline(DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    draw = voliro.VoliroElbo.noise_from(pipe.next(T, B * S), B, T, S)
    assert draw['gp'].shape == (B, T, S) and draw['b'].shape == (T, B * S) and draw['f'].shape == (T - 1, B * S)
    loss2, _ = eng.loss(si, so, draw)
    assert bool(torch.isfinite(loss2.detach()))


def test_ten_adam_steps_track_the_restatement():
    case = CASES[0]
    cfg, leaves, si, so, noise = vc.make_case(case)
    t = vc.leaf_tensors(leaves)
    eng, lv = _engine(cfg, leaves)
    opt_r = torch.optim.Adam([t[k] for k in LEAVES], lr=0.01)
    opt_d = torch.optim.Adam([lv[k] for k in LEAVES], lr=0.01)
    for step in range(10):
        opt_r.zero_grad()
        lr, _, _, _ = vc.loss_cpu(cfg, t, si, so, noise)
        lr.backward()
        opt_r.step()
        opt_d.zero_grad()
        ld, _ = eng.loss(si, so, noise)
        ld.backward()
        opt_d.step()
        rel = abs(float(ld.detach()) - float(lr.detach())) / abs(float(lr.detach()))
        print('step %d  restatement %.9e  hip %.9e  rel %.2e' % (step, float(lr.detach()), float(ld.detach()), rel))
        assert rel < 1e-6, (step, rel)
