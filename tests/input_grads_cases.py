"""Shared by the input-gradient tests: the shapes, and the reference -- reverse-mode autodiff of the float64 restatement
(oracle/cbfssm_torch_ref.elbo_step) with u and y requiring grad."""
import numpy as np
import torch

from test_input_adjoint_gpu import SHAPES, _setup      # the eight shapes: D = 7 .. 24, ragged groups / row blocks, stash mode

__all__ = ['SHAPES', '_setup', 'oracle_input_grads', 'assert_reference_is_informative', 'within_rule']


def oracle_input_grads(cfg, p, u, y, noise, cond, front=None):
    """(scalars, d loss / d params, d loss / d u, d loss / d y[, d loss / d front tensors]) on the CPU.
    front: optional (tensors dict, fn(tensors, u, y) -> (u', y')) placed in front of the model."""
    from oracle import cbfssm_torch_ref as tref
    params = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    ut = torch.tensor(np.asarray(u), dtype=torch.float64, requires_grad=True)
    yt = torch.tensor(np.asarray(y), dtype=torch.float64, requires_grad=True)
    nz = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in noise.items()}
    fr = None
    u_in, y_in = ut, yt
    if front is not None:
        fr = {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in front[0].items()}
        u_in, y_in = front[1](fr, ut, yt)
    out = tref.elbo_step(cfg, params, u_in, y_in, nz, cond)
    out['loss'].backward()
    res = ({k: float(v.detach()) for k, v in out.items()}, {k: v.grad.numpy().copy() for k, v in params.items()},
           ut.grad.numpy().copy(), yt.grad.numpy().copy())
    if fr is not None:
        res = res + ({k: v.grad.numpy().copy() for k, v in fr.items()},)
    return res


def assert_reference_is_informative(gu, gy):
    """a comparison against zeros would hide a buffer that was never written: the reference has no time step whose u rows
    are all zero, and its y gradient is non-zero at t = 0 and at t = T - 1"""
    T = gu.shape[1]
    for t in range(T):
        assert np.abs(gu[:, t, :]).max() > 0.0, ('d loss / d u is all zero at step', t)
    assert np.abs(gy[:, 0, :]).max() > 0.0 and np.abs(gy[:, T - 1, :]).max() > 0.0


def within_rule(name, g, r, rtol=1e-6, sel=None):
    """the rule of tests/test_hip_grad.py: every entry within rtol of the largest entry of its tensor; sel: a slice of the
    last axis checked on its own against the same scale (as tests/test_input_adjoint_gpu.py does for the lengthscales)"""
    g, r = np.asarray(g), np.asarray(r)
    assert g.shape == r.shape, (name, g.shape, r.shape)
    scale = np.abs(r).max() + 1e-300
    d = np.abs(g - r) if sel is None else np.abs(g[..., sel] - r[..., sel])
    err = (d.max() if d.size else 0.0) / scale
    print('%-28s max|ref| %.3e  err/max %.2e' % (name, scale, err))
    assert err < rtol, (name, err)
    return err
