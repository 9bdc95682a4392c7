"""Shared by the input-gradient tests: the shapes, and the reference -- reverse-mode autodiff of the float64 restatement
(oracle/cbfssm_torch_ref.elbo_step) with u and y requiring grad.

The reference per path (oracle_path_grads): d loss / d u and d loss / d y are sums of the paths of DESIGN 3.2a, and one
path can be 1e-3 of the sum's largest entry -- the 1e-6-of-the-largest-entry rule on the sum then lets a relative error of
1e-3 in that path through.  The restatement takes the backward runs' copy of u, y as leaves of their own (u_b, y_b: same
values), so one reverse sweep gives every path as a tensor of its own, and the rule is applied to each."""
import functools

import numpy as np
import torch

from test_input_adjoint_gpu import SHAPES, _setup      # the eight shapes: D = 7 .. 24, ragged groups / row blocks, stash mode

__all__ = ['SHAPES', '_setup', 'oracle_input_grads', 'assert_reference_is_informative', 'within_rule', 'PATHS',
           'oracle_path_grads', 'tile_grid_path_reference', 'assert_paths_are_informative', 'paths_from_buffers']


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


# path tensor -> (leaf of the restatement, what it is in DESIGN 3.2a)
PATHS = {'u_f': 'u through gp_f (path 1)', 'u_b': 'u through gp_b (path 2)', 'y_b': 'y through gp_b (path 2)',
         'y_o': 'gyo + log-likelihood term (paths 3 + 4)'}


def oracle_path_grads(cfg, p, u, y, noise, cond):
    """(scalars, d loss / d params, {path: tensor}) on the CPU: u_f + u_b is d loss / d u, y_o + y_b is d loss / d y."""
    from oracle import cbfssm_torch_ref as tref
    params = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    leaf = {k: torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=True)
            for k, a in (('u_f', u), ('y_o', y), ('u_b', u), ('y_b', y))}
    nz = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in noise.items()}
    out = tref.elbo_step(cfg, params, leaf['u_f'], leaf['y_o'], nz, cond, u_b=leaf['u_b'], y_b=leaf['y_b'])
    out['loss'].backward()
    paths = {k: v.grad.numpy().copy() for k, v in leaf.items()}
    for a in paths.values():
        a.setflags(write=False)
    return ({k: float(v.detach()) for k, v in out.items()}, {k: v.grad.numpy().copy() for k, v in params.items()}, paths)


@functools.lru_cache(maxsize=None)
def tile_grid_path_reference(name, cond):
    """oracle_path_grads of a row of tests/tile_grid.py, computed once and shared (the path tensors are read-only)"""
    import tile_grid as tg
    w, cfg, p, u, y, noise = tg.setup(tg.CASE_KW[name])
    return oracle_path_grads(cfg, p, u, y, noise, cond)


CHANNEL_SHARE, STEP_SHARE = 0.1, 0.01


def assert_paths_are_informative(name, paths):
    """a path tensor with a channel or a time step near zero would let a kernel that never wrote it pass: every channel's
    largest entry is >= 0.1 and every time step's >= 0.01 of the tensor's largest; the one exception is exact: u[T - 1]
    feeds no forward step, the gp_f path of u is zero there.  Returns (worst channel share, worst step share)."""
    worst_c, worst_t = 1.0, 1.0
    for k in PATHS:
        g = paths[k]
        top = np.abs(g).max()
        assert np.isfinite(g).all() and top > 0.0, (name, k)
        chan = np.abs(g).max(axis=(0, 1)) / top
        step = np.abs(g).max(axis=(0, 2)) / top
        if k == 'u_f':
            assert not g[:, -1, :].any(), (name, 'the gp_f path of u must be exactly zero at t = T - 1')
            step = step[:-1]
        assert chan.min() >= CHANNEL_SHARE, (name, k, 'channel', int(chan.argmin()), chan.min())
        assert step.min() >= STEP_SHARE, (name, k, 'step', int(step.argmin()), step.min())
        worst_c, worst_t = min(worst_c, chan.min()), min(worst_t, step.min())
    return worst_c, worst_t


def paths_from_buffers(w, p, in_bufs, grad_y):
    """the four paths rebuilt from what the engine keeps: gin_f (T-1, dim_u, N), gin_b (2, T, dim_u + dim_y, N),
    chain n = b S + s; 1/lengthscale of the GP and input row from the parameters.  grad_y: the engine's d loss / d y."""
    from cbfssm import synthetic as syn
    gin_f, gin_b, _ = (np.asarray(b.cpu().numpy(), dtype=np.float64) for b in in_bufs)
    B, S, T, du, dy, dob = w.B, w.S, w.T, w.dim_u, w.dim_y, w.dim_x - w.dim_y
    invl_f = 1.0 / syn.softplus(np.asarray(p['f.lengthscales_unc'], dtype=np.float64).reshape(-1))
    invl_b = 1.0 / syn.softplus(np.asarray(p['b.lengthscales_unc'], dtype=np.float64).reshape(-1))
    assert gin_f.size == (T - 1) * du * B * S and gin_b.size == 2 * T * (du + dy) * B * S
    u_f = np.zeros((B, T, du))
    u_f[:, :T - 1] = gin_f.reshape(T - 1, du, B, S).sum(3).transpose(2, 0, 1) * invl_f[w.dim_x:w.dim_x + du]
    aux = gin_b.reshape(2, T, du + dy, B, S).sum(4).sum(0).transpose(2, 0, 1) * invl_b[dob:dob + du + dy]
    u_b, y_b = aux[..., :du], aux[..., du:]
    return {'u_f': u_f, 'u_b': u_b, 'y_b': y_b, 'y_o': np.asarray(grad_y) - y_b}


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
