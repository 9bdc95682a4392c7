"""Shared by the input-gradient tests of the forward-only variants (CBFSSMHALF, PR-SSM): the engine-level set-ups, the
reference -- reverse-mode autodiff of oracle/cbfssm_torch_ref.half_elbo_step / prssm_elbo_step with u and y requiring grad
-- and the structure that reference has (it replaces input_grads_cases.assert_reference_is_informative, whose "no zero
step" rule does not hold here: the last input feeds nothing, so d loss / d u is exactly zero at t = T - 1 unless the
recognition window covers that row)."""
import contextlib
import functools

import numpy as np
import torch

from input_grads_cases import within_rule
from test_oracle import _half_setup, _prssm_setup

__all__ = ['CASES', 'CONDS', 'setup', 'oracle', 'assert_reference_structure', 'rows_within_rule', 'window_rows', 'within_rule']

STASH = dict(M=130, dim_x=6, dim_u=2, dim_y=2, B=2, S=9, recog_len=2)
CONV = dict(T=20, B=2, S=5, M=33, recog_len=16, dim_x=4, dim_u=1, dim_y=1)
# name -> (variant, recogniser, workload keywords, extra config)
CASES = {
    'half-rnn': ('half', 'rnn', dict(T=11, B=3, S=4, M=12, recog_len=3), {}),
    'half-output': ('half', 'output', dict(T=9, B=2, S=7, M=20, recog_len=4, k_factor=20.), {}),
    # D = 21: the u rows sit in the second 16-row block of gp_f's input; 18 chains: a ragged second chain group
    'half-rnn-D21': ('half', 'rnn', dict(dim_x=14, dim_u=7, dim_y=7, M=20, T=6, B=2, S=9, recog_len=2), {}),
    'half-rnn-no-hidden': ('half', 'rnn', dict(dim_x=3, dim_u=2, dim_y=3, M=10, T=7, B=2, S=5, recog_len=3), {}),
    # both kernel limits (n_in = 23 <= 32 at dim_x = 16, D = 24), and recog_len = T: the window covers u[T - 1]
    'half-rnn-limits': ('half', 'rnn', dict(dim_x=16, dim_u=8, dim_y=15, M=20, T=6, recog_len=6, B=3, S=3), {}),
    'half-rnn-T1': ('half', 'rnn', dict(T=1, B=2, S=4, M=8, recog_len=3), {}),
    'half-rnn-stash': ('half', 'rnn', dict(STASH, T=9), {'adjoint_stash_gib': 3e-4}),
    'prssm-output': ('prssm', 'output', dict(T=9, B=2, S=7, M=20, recog_len=4), {}),
    'prssm-rnn': ('prssm', 'rnn', dict(T=11, B=3, S=4, M=12, recog_len=3), {}),
    'prssm-conv': ('prssm', 'conv', CONV, {}),
    'prssm-rnn-stash': ('prssm', 'rnn', dict(STASH, T=9), {'adjoint_stash_gib': 3e-4}),
}


def CONDS(name):
    """both `condition` values for CBFSSMHALF; PR-SSM never conditions (the engine ignores the argument)"""
    return (True, False) if CASES[name][0] == 'half' else (True,)


def setup(name, **over):
    """(variant, w, cfg, p, u, y, noise) of a case; the conv case takes the float32-valued, margin-checked draw of
    tests/test_conv_recog_gpu.py (asserted here, on the CPU, before anything is compared)"""
    variant, recog, kw, extra = CASES[name]
    kw = dict(kw, **over)
    if recog == 'conv':
        from test_conv_recog_gpu import MARGIN, _engine_setup
        w, cfg, p, u, y, noise, margin = _engine_setup(3, **kw)
        assert margin >= MARGIN, (name, margin)
    else:
        w, cfg, p, u, y, noise = (_prssm_setup if variant == 'prssm' else _half_setup)(recog, **kw)
    cfg = dict(cfg, **extra)
    return variant, w, cfg, p, u, y, noise


def window_rows(cfg, T):
    """rows of u, y that the recognition model reads (none for the `output` recogniser, whose x_0 reads y_0 directly)"""
    return 0 if cfg.get('recog_model', 'rnn') == 'output' else min(int(cfg['recog_len']), T)


@contextlib.contextmanager
def float64_conv():
    """the oracle's conv recogniser evaluated in float64 (tests/test_conv_recog_gpu.py::_truth): the truth both float32 codings
    are measured against"""
    from oracle import cbfssm_torch_ref as tref
    from test_conv_recog_gpu import _truth
    keep = tref.conv_recognition
    tref.conv_recognition = lambda rp, u, y, R: _truth(rp['conv_kernel'], rp['conv_bias'], rp['dense_kernel'], rp['dense_bias'],
                                                       u, y, R)[0]
    try:
        yield
    finally:
        tref.conv_recognition = keep


def oracle_run(variant, cfg, p, u, y, noise, cond, front=None):
    """(loss, d loss / d params, d loss / d u, d loss / d y[, d loss / d front tensors]) on the CPU.
    front: optional (tensors dict, fn(tensors, u, y) -> (u', y')) placed in front of the model."""
    from oracle import cbfssm_torch_ref as tref
    params = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    ut = torch.tensor(np.asarray(u), dtype=torch.float64, requires_grad=True)
    yt = torch.tensor(np.asarray(y), dtype=torch.float64, requires_grad=True)
    nz = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in noise.items()}
    fr, u_in, y_in = None, ut, yt
    if front is not None:
        fr = {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in front[0].items()}
        u_in, y_in = front[1](fr, ut, yt)
    if variant == 'prssm':
        out = tref.prssm_elbo_step(cfg, params, u_in, y_in, nz)
    else:
        out = tref.half_elbo_step(cfg, params, u_in, y_in, nz, cond)
    out['loss'].backward()

    def g(t):
        return (t.grad if t.grad is not None else torch.zeros_like(t)).numpy().copy()
    res = (float(out['loss'].detach()), {k: g(v) for k, v in params.items()}, g(ut), g(yt))
    if fr is not None:
        res = res + ({k: g(v) for k, v in fr.items()},)
    for a in res[2:4]:
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def oracle(name, cond, truth=False):
    """the reference of a case, computed once and shared (never written to); truth: with the conv recogniser in float64"""
    variant, w, cfg, p, u, y, noise = setup(name)
    with (float64_conv() if truth else contextlib.nullcontext()):
        return oracle_run(variant, cfg, p, u, y, noise, cond)


def assert_reference_structure(name, cfg, gu, gy):
    """a comparison against zeros would hide a buffer that was never written.  The reference's d loss / d y is non-zero at
    every step, its d loss / d u at every t <= T - 2; at t = T - 1 it is EXACTLY zero when that row lies outside the
    recognition window (u[T - 1] feeds no GP evaluation) and non-zero when the window covers it."""
    T = gy.shape[1]
    R = window_rows(cfg, T)
    assert np.isfinite(gu).all() and np.isfinite(gy).all()
    for t in range(T):
        assert np.abs(gy[:, t, :]).max() > 0.0, (name, 'd loss / d y is all zero at step', t)
    for t in range(T - 1):
        assert np.abs(gu[:, t, :]).max() > 0.0, (name, 'd loss / d u is all zero at step', t)
    if T - 1 >= R:
        assert not gu[:, T - 1, :].any(), (name, 'd loss / d u must be exactly zero at t = T - 1')
    else:
        assert np.abs(gu[:, T - 1, :]).max() > 0.0, (name, 'the window covers u[T - 1]')


def rows_within_rule(tag, g, r, R, rtol=1e-6, sel=None):
    """within_rule on the window rows t < R and on the rows t >= R separately, each against its own largest reference entry
    (the window part can be 1e3 times larger and would otherwise hide the time-loop part)"""
    errs = []
    for what, sl in (('window rows', slice(0, R)), ('rows t>=R', slice(R, None))):
        gs, rs = g[:, sl], r[:, sl]
        if rs.size == 0:
            continue
        if not np.abs(rs).max() > 0.0:              # (u[T - 1] alone behind the window: exactly zero on both sides)
            assert not gs.any(), (tag, what, 'reference is exactly zero, kernel is not')
            continue
        errs.append(within_rule('%s %s' % (tag, what), gs, rs, rtol=rtol, sel=sel))
    return max(errs) if errs else 0.0


# ---- the recognition kernels' window adjoint at the ABI level -----------------------------------------------------------
def _gru_window(fx, dtype):
    """d (x0 . gx0).sum() / d [u, y][:, :R] of oracle.cbfssm_torch_ref.gru_recognition at `dtype`: (B, R, n_in) float64"""
    from oracle import cbfssm_torch_ref as tref
    from test_gru_recog_gpu import NAMES, ORACLE_NAMES
    rp = {o: torch.tensor(fx[k], dtype=dtype) for k, o in zip(NAMES, ORACLE_NAMES)}
    u = torch.tensor(fx['u'], dtype=dtype, requires_grad=True)
    y = torch.tensor(fx['y'], dtype=dtype, requires_grad=True)
    x0 = tref.gru_recognition(rp, u, y, fx['R'])
    gu, gy = torch.autograd.grad((x0 * torch.tensor(fx['gx0'], dtype=dtype)).sum(), [u, y])
    return torch.cat((gu, gy), dim=2)[:, :fx['R']].numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def gru_window_case(name):
    """(the case of tests/test_gru_recog_gpu.py, the float64 reference of gwin, its amplification A measured as that file
    does: the float32 oracle's relative error against the float64 one in units of 2^-24)"""
    from test_gru_recog_gpu import EPS32, _case, _rel
    case = _case(name)
    ref = _gru_window(case['fx'], torch.float64)
    A = _rel(_gru_window(case['fx'], torch.float32), ref) / EPS32
    ref.setflags(write=False)
    return case, ref, A


def conv_window_reference(fx):
    """(g_truth, g_ref) of gwin for a fixture of tests/test_conv_recog_gpu.py: the float64 autograd of that file's _truth and
    the float32 oracle's autograd, both of (x0 . gx0).sum() with respect to [u, y][:, :R]"""
    from oracle import cbfssm_torch_ref as tref
    from test_conv_recog_gpu import _truth
    gx0, R = torch.tensor(fx['gx0']), fx['R']
    out = []
    for truth in (True, False):
        u, y = torch.tensor(fx['u'], requires_grad=True), torch.tensor(fx['y'], requires_grad=True)
        if truth:
            x0 = _truth(*(torch.tensor(fx[k]) for k in ('K', 'bc', 'Wd', 'bd')), u, y, R)[0]
        else:
            rp = {n: torch.tensor(fx[k]) for n, k in (('conv_kernel', 'K'), ('conv_bias', 'bc'), ('dense_kernel', 'Wd'),
                                                      ('dense_bias', 'bd'))}
            x0 = tref.conv_recognition(rp, u, y, R)
        gu, gy = torch.autograd.grad((x0 * gx0).sum(), [u, y])
        out.append(torch.cat((gu, gy), dim=2)[:, :R].numpy().astype(np.float64))
    return tuple(out)
