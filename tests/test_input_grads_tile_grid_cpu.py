"""The reference per path of tests/test_input_grads_tile_grid_gpu.py, without a GPU (input_grads_cases.oracle_path_grads:
the restatement with the backward runs' copy of u, y as leaves of their own), on every row of tests/tile_grid.py and both
`condition` values:

  * the split changes nothing: the loss is the default graph's bit for bit, the paths sum to the gradients of the default
    graph (u_f + u_b = d loss / d u, y_o + y_b = d loss / d y) within 1e-13 of the largest entry -- autograd adds the same
    terms in another order, a few ulp of the largest one;
  * every path tensor is informative, channel by channel and step by step (the caps of assert_paths_are_informative), so the
    1e-6 rule of the GPU test cannot be met by a kernel that leaves part of a buffer unwritten;
  * the forward-only rows have well-conditioned K_mm at their own parameter draw and a reference with the structure of
    half_input_grads_cases.assert_reference_structure.

Each test prints the shares it found (pytest -s)."""
import numpy as np
import pytest

from cbfssm import synthetic as syn
import input_grads_cases as igc
import tile_grid as tg


@pytest.mark.parametrize('cond', [True, False])
@pytest.mark.parametrize('name', tg.CASE_IDS)
def test_paths_sum_to_the_default_graph_and_are_informative(name, cond):
    w, cfg, p, u, y, noise = tg.setup(tg.CASE_KW[name])
    scal0, gref0, gu, gy = igc.oracle_input_grads(cfg, p, u, y, noise, cond)
    scal, gref, paths = igc.tile_grid_path_reference(name, cond)
    assert scal['loss'] == scal0['loss']
    for k in syn.PARAM_NAMES:
        assert np.array_equal(gref[k], gref0[k]), k
    for total, parts in ((gu, ('u_f', 'u_b')), (gy, ('y_o', 'y_b'))):
        assert all(paths[k].shape == total.shape for k in parts)
        err = np.abs(paths[parts[0]] + paths[parts[1]] - total).max() / np.abs(total).max()
        print('%s cond=%d %s + %s against the default graph: %.1e of the largest entry' % (name, cond, *parts, err))
        assert err <= 1e-13, (parts, err)
    shares = {k: np.abs(paths[k]).max() / np.abs(gu if k[0] == 'u' else gy).max() for k in igc.PATHS}
    print('%s cond=%d largest entry of each path / largest of the sum: %s' % (
        name, cond, ' '.join('%s %.1e' % kv for kv in shares.items())))
    worst_c, worst_t = igc.assert_paths_are_informative(name, paths)
    print('%s cond=%d worst channel share %.3f, worst step share %.4f' % (name, cond, worst_c, worst_t))


def test_the_default_call_of_the_restatement_takes_no_new_leaf():
    """u_b = y_b = None is the graph that existed: passing the tensors themselves gives the same bits"""
    import torch
    from oracle import cbfssm_torch_ref as tref
    w, cfg, p, u, y, noise = tg.setup(tg.CASE_KW['nb1_fill_dk4'])
    params = {k: torch.tensor(v) for k, v in p.items()}
    ut, yt = torch.tensor(np.asarray(u)), torch.tensor(np.asarray(y))
    nz = {k: torch.tensor(np.asarray(v)) for k, v in noise.items()}
    a = tref.elbo_step(cfg, params, ut, yt, nz, True)
    b = tref.elbo_step(cfg, params, ut, yt, nz, True, u_b=ut, y_b=yt)
    assert all(float(a[k]) == float(b[k]) for k in a)
    # and the new leaves do feed the backward runs: other values there move the entropy, not a bit of it through u / y
    c = tref.elbo_step(cfg, params, ut, yt, nz, True, u_b=ut + 0.1, y_b=yt - 0.1)
    assert float(c['entropy']) != float(a['entropy']) and float(c['kl_z_b']) == float(a['kl_z_b'])


def _forward_only_setup(name, variant):
    from test_oracle import _half_setup, _prssm_setup
    return (_prssm_setup if variant == 'prssm' else _half_setup)('rnn', **tg.CASE_KW[name])


@pytest.mark.parametrize('name,variant', [(n, 'half') for n in tg.IG_HALF_CASES] + [(n, 'prssm') for n in tg.IG_PRSSM_CASES])
def test_forward_only_rows_are_well_conditioned_and_structured(name, variant):
    import torch
    import half_input_grads_cases as hc
    from oracle import cbfssm_torch_ref as tref
    w, cfg, p, u, y, noise = _forward_only_setup(name, variant)
    pre = 'f.' if variant == 'half' else ''
    kern = tref.RBF(torch.tensor(p[pre + 'variance_unc']), torch.tensor(p[pre + 'lengthscales_unc']))
    K = kern.K(torch.tensor(p[pre + 'zeta_pos'])).numpy() + tref.JITTER * np.eye(w.M)
    cond_k = np.linalg.cond(K)
    print('%s %s cond(K_mm) %.2e' % (name, variant, cond_k))
    assert cond_k < 1e6
    for cond in ((True, False) if variant == 'half' else (True,)):
        loss, gref, gu, gy = hc.oracle_run(variant, cfg, p, u, y, noise, cond)
        assert np.isfinite(loss)
        hc.assert_reference_structure(name, cfg, gu, gy)
