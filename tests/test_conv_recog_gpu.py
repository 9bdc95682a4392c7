"""PR-SSM's conv recognition model as HIP kernels (cbfssm_conv_recog_f32 / _bwd_f32; reference cbfssm/model/prssm.py:146-157)
against the committed float32 restatement (oracle.cbfssm_torch_ref.conv_recognition) and a float64 evaluation of the same
four lines written here -- the "truth" that both float32 codings are measured against.

Every parity test prints its figures before it asserts (lines starting with CONV_RECOG_RECORD: run with -s to keep them;
profiles/conv_recog/ holds one such run)."""
import numpy as np
import pytest
import torch

from cbfssm.hip import lib, ops
from cbfssm.hip import train_half
from cbfssm.hip.train import TFAdam
from cbfssm.hip.train_half import CONV_NAMES, HipHalfGrad, HipHalfTrainStep, half_param_names

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = 2.0 ** -24          # unit round-off of float32
MARGIN = 64.0             # rounding bounds between a float64 value and a decision boundary (relu mask, pooling winner)


def _f32(a):
    """rounded to float32 and widened again: the casts of the float32 codings are then exact, not part of the comparison"""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _fixture(seed, B, R, dim_u, dim_y, dim_x):
    """one default_rng(seed); draws in the order conv kernel, conv bias, dense kernel, dense bias, u, y, gx0 (scales of
    tests/test_oracle.py::_prssm_setup, T = R + 3); gx0 stays float64, everything else is a float32 value"""
    rng = np.random.default_rng(seed)
    n_in, P = dim_u + dim_y, (R - 2) // 2
    fx = {'K': _f32(0.4 * rng.standard_normal((3, n_in, 5))), 'bc': _f32(0.1 * rng.standard_normal(5)),
          'Wd': _f32(0.3 * rng.standard_normal((5 * P, dim_x))), 'bd': _f32(0.1 * rng.standard_normal(dim_x)),
          'u': _f32(rng.standard_normal((B, R + 3, dim_u))), 'y': _f32(rng.standard_normal((B, R + 3, dim_y)))}
    fx['gx0'] = rng.standard_normal((B, dim_x))
    fx.update(B=B, R=R, T=R + 3, dim_u=dim_u, dim_y=dim_y, dim_x=dim_x, P=P, n_in=n_in)
    return fx


def _truth(K, bc, Wd, bd, u, y, R):
    """prssm.py:146-157 in float64 on torch tensors (differentiable): x_0 and the pre-activations"""
    x = torch.cat((u, y), dim=2)[:, :R, :]
    B, P = x.shape[0], (R - 2) // 2
    pre = bc + sum(x[:, w:w + R - 2, :] @ K[w] for w in range(3))                          # (B, R - 2, 5): valid conv
    act = torch.relu(pre)
    pool = act[:, :2 * P, :].reshape(B, P, 2, 5).max(dim=2).values                        # an odd last position is dropped
    return pool.reshape(B, 5 * P) @ Wd + bd, pre                                          # flattened (time, channel)


def _abs_bounds(fx):
    """the same lines on absolute values: apre (B, R - 2, 5) >= |any partial sum of a pre-activation|, and the first-order
    bound of |x0_float32 - x0_truth| for float32 dot products summed in any order"""
    t = {k: torch.tensor(np.abs(fx[k])) for k in ('K', 'bc', 'Wd', 'bd', 'u', 'y')}
    R, P, B = fx['R'], fx['P'], fx['B']
    x = torch.cat((t['u'], t['y']), dim=2)[:, :R, :]
    apre = t['bc'] + sum(x[:, w:w + R - 2, :] @ t['K'][w] for w in range(3))
    apool = apre[:, :2 * P, :].reshape(B, P, 2, 5).max(dim=2).values.reshape(B, 5 * P)    # relu and max are 1-Lipschitz
    bound = (3 * fx['n_in'] + 5 * P + 2) * EPS * (t['bd'] + apool @ t['Wd'])
    return apre.numpy(), bound.numpy()


def _margin(fx):
    """the smallest distance, in float32 rounding bounds of the values involved, between a pre-activation and zero and
    between the two members of a pooling pair whose maximum is positive: two correct float32 codings agree on every relu
    mask and pooling winner when this is comfortably above 1"""
    t = {k: torch.tensor(fx[k]) for k in ('K', 'bc', 'Wd', 'bd', 'u', 'y')}
    _, pre = _truth(t['K'], t['bc'], t['Wd'], t['bd'], t['u'], t['y'], fx['R'])
    pre = pre.numpy()
    apre, _ = _abs_bounds(fx)
    rb = (3 * fx['n_in'] + 1) * EPS * apre
    m_zero = float((np.abs(pre) / rb).min())
    P = fx['P']
    p0, p1, r0, r1 = pre[:, 0:2 * P:2], pre[:, 1:2 * P:2], rb[:, 0:2 * P:2], rb[:, 1:2 * P:2]
    live = np.maximum(p0, p1) > 0
    m_pair = float((np.abs(p0 - p1) / (r0 + r1))[live].min()) if live.any() else np.inf
    return min(m_zero, m_pair)


def _flat_params(fx):
    return torch.tensor(np.concatenate([fx[k].reshape(-1) for k in ('K', 'bc', 'Wd', 'bd')]), device=DEV)


def _kernel_x0(fx):
    l = lib.load()
    u, y, prm = torch.tensor(fx['u'], device=DEV), torch.tensor(fx['y'], device=DEV), _flat_params(fx)
    x0 = torch.zeros(fx['B'], fx['dim_x'], dtype=torch.float64, device=DEV)
    rc = l.cbfssm_conv_recog_f32(fx['B'], fx['T'], fx['dim_u'], fx['dim_y'], fx['dim_x'], fx['R'], ops._ptr(u), ops._ptr(y),
                                 ops._ptr(prm), ops._ptr(x0), ops._stream())
    lib.check(rc, 'cbfssm_conv_recog_f32')
    torch.cuda.synchronize()
    return x0.cpu().numpy()


def _kernel_grads(fx):
    """(slabs (B, E), their fixed-order sum (E,)) of the backward entry point"""
    l = lib.load()
    B = fx['B']
    E = int(l.cbfssm_conv_recog_param_elems(fx['dim_u'], fx['dim_y'], fx['dim_x'], fx['R']))
    assert E == 15 * fx['n_in'] + 5 + 5 * fx['P'] * fx['dim_x'] + fx['dim_x']
    u, y, prm = torch.tensor(fx['u'], device=DEV), torch.tensor(fx['y'], device=DEV), _flat_params(fx)
    gx0 = torch.tensor(fx['gx0'], device=DEV)
    gpart = torch.zeros((B + 32) * E, dtype=torch.float64, device=DEV)        # + CBFSSM_REDUCE_SPLIT scratch slabs
    rc = l.cbfssm_conv_recog_bwd_f32(B, fx['T'], fx['dim_u'], fx['dim_y'], fx['dim_x'], fx['R'], ops._ptr(u), ops._ptr(y),
                                     ops._ptr(prm), ops._ptr(gx0), ops._ptr(gpart), ops._stream())
    lib.check(rc, 'cbfssm_conv_recog_bwd_f32')
    slabs = gpart[:B * E].view(B, E).clone()
    out = torch.zeros(E, dtype=torch.float64, device=DEV)
    ops.reduce_partials(gpart, E, B, out, ops._stream())
    torch.cuda.synchronize()
    return slabs.cpu().numpy(), out.cpu().numpy()


def _oracle_x0(fx, grad=False):
    from oracle import cbfssm_torch_ref as tref
    rp = {n: torch.tensor(fx[k], requires_grad=grad) for n, k in (('conv_kernel', 'K'), ('conv_bias', 'bc'),
                                                                  ('dense_kernel', 'Wd'), ('dense_bias', 'bd'))}
    return tref.conv_recognition(rp, torch.tensor(fx['u']), torch.tensor(fx['y']), fx['R']), rp


X0_SHAPES = [(64, 16, 1, 1, 4), (256, 16, 7, 7, 14), (5, 17, 2, 2, 5), (7, 27, 2, 1, 16), (3, 4, 1, 1, 2), (33, 9, 3, 2, 6)]


@pytest.mark.parametrize('shape', X0_SHAPES, ids=['-'.join(map(str, s)) for s in X0_SHAPES])
def test_x0_is_inside_the_float32_rounding_bound(shape):
    """|x0_kernel - x0_truth| <= (3 n_in + 5 P + 2) 2^-24 (|b_d| + sum_j apool_j |W_d[j]|) element-wise: the first-order bound
    of float32 dot products in any summation order, evaluated on absolute values -- derived, not tuned."""
    B, R = shape[:2]
    fx = _fixture(11 + 1000 * B + R, *shape)
    t = {k: torch.tensor(fx[k]) for k in ('K', 'bc', 'Wd', 'bd', 'u', 'y')}
    truth = _truth(t['K'], t['bc'], t['Wd'], t['bd'], t['u'], t['y'], R)[0].numpy()
    _, bound = _abs_bounds(fx)
    x0 = _kernel_x0(fx)
    err = np.abs(x0 - truth)
    err_o = np.abs(_oracle_x0(fx)[0].detach().numpy() - truth)
    print('CONV_RECOG_RECORD x0 shape=%s max|kernel-truth|=%.3e max|oracle-truth|=%.3e worst err/bound kernel=%.4f oracle=%.4f'
          % (shape, err.max(), err_o.max(), (err / bound).max(), (err_o / bound).max()))
    assert np.all(err <= bound), (shape, float((err / bound).max()))


GRAD_CASES = [((64, 16, 1, 1, 4), 1), ((16, 16, 7, 7, 14), 1), ((32, 16, 7, 7, 14), 5), ((5, 17, 2, 2, 5), 1),
              ((7, 27, 2, 1, 16), 1), ((3, 4, 1, 1, 2), 1), ((33, 9, 3, 2, 6), 1)]


def _split(fx, flat):
    out, o = {}, 0
    for k in ('K', 'bc', 'Wd', 'bd'):
        out[k] = flat[o:o + fx[k].size].reshape(fx[k].shape)
        o += fx[k].size
    assert o == flat.size
    return out


@pytest.mark.parametrize('shape,seed', GRAD_CASES, ids=['-'.join(map(str, s)) + '-seed%d' % sd for s, sd in GRAD_CASES])
def test_gradients_against_float64_autograd(shape, seed):
    """e_kernel[k] <= 4 e_ref[k] + 2^-23 per tensor, e = max|g - g_truth| / max|g_truth|, g_truth the float64 autograd of
    the float64 evaluation with (x0 . gx0).sum(), e_ref the oracle's float32 autograd on the same inputs.  The kernel sums
    over the batch in float64 where the tensor library sums in float32, so it should be the more accurate of the two; 4
    covers another order inside a sequence, 2^-23 the rounding of gx0 and of the result.  Condition, asserted first: no
    relu mask or pooling winner of the fixture is within 64 rounding bounds of flipping."""
    fx = _fixture(seed, *shape)
    margin = _margin(fx)
    print('CONV_RECOG_RECORD grad shape=%s seed=%d margin=%.1f' % (shape, seed, margin))
    assert margin >= MARGIN, (shape, seed, margin)
    t = {k: torch.tensor(fx[k], requires_grad=k in ('K', 'bc', 'Wd', 'bd')) for k in ('K', 'bc', 'Wd', 'bd', 'u', 'y')}
    gx0 = torch.tensor(fx['gx0'])
    x0 = _truth(t['K'], t['bc'], t['Wd'], t['bd'], t['u'], t['y'], fx['R'])[0]
    g_truth = dict(zip(('K', 'bc', 'Wd', 'bd'), torch.autograd.grad((x0 * gx0).sum(), [t[k] for k in ('K', 'bc', 'Wd', 'bd')])))
    x0o, rp = _oracle_x0(fx, grad=True)
    g_ref = dict(zip(('K', 'bc', 'Wd', 'bd'), torch.autograd.grad((x0o * gx0).sum(), list(rp.values()))))
    g_ker = _split(fx, _kernel_grads(fx)[1])
    bad = []
    for k in ('K', 'bc', 'Wd', 'bd'):
        gt = g_truth[k].numpy()
        scale = np.abs(gt).max()
        e_ker = np.abs(g_ker[k] - gt).max() / scale
        e_ref = np.abs(g_ref[k].numpy() - gt).max() / scale
        print('CONV_RECOG_RECORD grad shape=%s seed=%d tensor=%s e_kernel=%.3e e_ref=%.3e ratio=%.3f'
              % (shape, seed, k, e_ker, e_ref, e_ker / max(e_ref, 1e-300)))
        if not e_ker <= 4 * e_ref + 2.0 ** -23:
            bad.append((k, e_ker, e_ref))
    assert not bad, bad


def test_reproducible_and_independent_of_the_batch():
    fx = _fixture(1, 33, 9, 3, 2, 6)
    assert np.array_equal(_kernel_x0(fx), _kernel_x0(fx))
    slabs, total = _kernel_grads(fx)
    slabs2, total2 = _kernel_grads(fx)
    assert np.array_equal(slabs, slabs2) and np.array_equal(total, total2)
    for b in (0, 17, 32):                                   # the same sequence alone: bitwise the slab it has inside the batch
        one = dict(fx, B=1, u=fx['u'][b:b + 1], y=fx['y'][b:b + 1], gx0=fx['gx0'][b:b + 1])
        s1, t1 = _kernel_grads(one)
        assert np.array_equal(s1[0], slabs[b]) and np.array_equal(t1, slabs[b])
        assert np.array_equal(_kernel_x0(one)[0], _kernel_x0(fx)[b])


def _engine_setup(seed, **kw):
    """the set-up of tests/test_prssm_gpu.py's 'conv' case with the recogniser's parameters and u, y drawn from
    default_rng(seed) as float32 values, and the margin of that draw"""
    from test_oracle import _prssm_setup
    w, cfg, p, u, y, noise = _prssm_setup('conv', **kw)
    fx = _fixture(seed, w.B, w.recog_len, w.dim_u, w.dim_y, w.dim_x)
    rng = np.random.default_rng(seed + 1)
    u, y = _f32(rng.standard_normal(u.shape)), _f32(rng.standard_normal(y.shape))
    fx.update(u=u, y=y, T=w.T)
    for n, k in zip(CONV_NAMES, ('K', 'bc', 'Wd', 'bd')):
        assert p[n].shape == fx[k].shape
        p[n] = fx[k]
    return w, cfg, p, u, y, noise, _margin(fx)


def _raise(*a, **k):
    raise AssertionError('the tensor-library conv recogniser ran')


def _fused_and_torch(monkeypatch, cfg, p, u, y, noise, dtype):
    params = {k: torch.tensor(v, device=DEV) for k, v in p.items()}
    with monkeypatch.context() as m:
        m.delenv('CBFSSM_TORCH_CONV', raising=False)
        m.setattr(train_half, 'conv_recognition', _raise)
        eng = HipHalfGrad(cfg, DEV, variant='prssm', dtype=dtype)
        assert eng.fused_conv
        loss_f, _, _ = eng.forward(params, u, y, noise, True)
        loss, grads, _ = eng.loss_and_grads(params, u, y, noise, True)
        torch.cuda.synchronize()
    assert float(loss_f) == pytest.approx(float(loss), rel=1e-12)
    assert set(grads) == set(half_param_names(cfg, 'prssm'))
    tail = torch.cat([grads[k].reshape(-1) for k in CONV_NAMES])
    assert torch.equal(grads.flat[grads.flat.numel() - tail.numel():], tail)
    assert all(grads[k].untyped_storage().data_ptr() == grads.flat.untyped_storage().data_ptr() for k in CONV_NAMES)
    with monkeypatch.context() as m:
        m.setenv('CBFSSM_TORCH_CONV', '1')
        ref = HipHalfGrad(cfg, DEV, variant='prssm', dtype=dtype)
    assert not ref.fused_conv
    loss_r, grads_r, _ = ref.loss_and_grads(params, u, y, noise, True)
    rel = abs(float(loss) - float(loss_r)) / abs(float(loss_r))
    errs = {k: float((grads[k] - grads_r[k]).abs().max() / (grads_r[k].abs().max() + 1e-300)) for k in grads_r}
    return rel, errs


SMALL = dict(T=20, B=2, S=5, M=33, recog_len=16, dim_x=4, dim_u=1, dim_y=1)


@pytest.mark.parametrize('name,kw', [('small', SMALL), ('actuator', dict(SMALL, B=64, T=100, S=50, M=50))])
def test_engine_takes_the_fused_path_and_matches_the_tensor_library(monkeypatch, name, kw):
    w, cfg, p, u, y, noise, margin = _engine_setup(3, **kw)
    print('CONV_RECOG_RECORD engine %s margin=%.1f' % (name, margin))
    assert margin >= MARGIN, margin
    rel, errs = _fused_and_torch(monkeypatch, cfg, p, u, y, noise, 'float64')
    print('CONV_RECOG_RECORD engine %s float64 loss rel=%.3e worst grad err=%.3e (%s)'
          % (name, rel, max(errs.values()), max(errs, key=errs.get)))
    assert rel <= 1e-6, rel                                  # the project's tolerances for this float32 recogniser
    assert all(e <= 1e-3 for e in errs.values()), errs       # (tests/test_prssm_gpu.py)


def test_engine_float32_time_loops(monkeypatch):
    w, cfg, p, u, y, noise, margin = _engine_setup(3, **SMALL)
    assert margin >= MARGIN, margin
    rel, errs = _fused_and_torch(monkeypatch, cfg, p, u, y, noise, 'float32')
    print('CONV_RECOG_RECORD engine small float32 loss rel=%.3e worst grad err=%.3e (%s)'
          % (rel, max(errs.values()), max(errs, key=errs.get)))
    assert rel <= 2e-3, rel                                  # the float32 passes amplify the last-bit difference in x_0
    assert all(e <= 1e-2 for e in errs.values()), errs


def test_engine_keeps_the_tensor_library_beyond_the_kernel_limits(monkeypatch):
    monkeypatch.delenv('CBFSSM_TORCH_CONV', raising=False)
    w, cfg, p, u, y, noise, _ = _engine_setup(3, **dict(SMALL, T=72, recog_len=70))
    eng = HipHalfGrad(cfg, DEV, variant='prssm')
    assert eng.conv and not eng.fused_conv
    params = {k: torch.tensor(v, device=DEV) for k, v in p.items()}
    loss, grads, _ = eng.loss_and_grads(params, u, y, noise, True)
    assert np.isfinite(float(loss)) and set(grads) == set(half_param_names(cfg, 'prssm'))
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert float(grads['recog.conv_kernel'].abs().max()) > 0


def test_graph_replay_equals_eager_steps_bit_for_bit(monkeypatch):
    """every launch of the step is deterministic with fixed-order reductions: three replays of the captured step leave the
    parameters and losses of three eager steps"""
    monkeypatch.delenv('CBFSSM_TORCH_CONV', raising=False)
    w, cfg, p, u, y, noise, _ = _engine_setup(3, **SMALL)
    res = {}
    for graph in (True, False):
        eng = HipHalfGrad(cfg, DEV, variant='prssm')
        assert eng.fused_conv
        opt = TFAdam({k: torch.tensor(p[k], device=DEV) for k in half_param_names(cfg, 'prssm')}, 0.01)
        step = HipHalfTrainStep(eng, opt, graph=graph)
        assert step.use_graph == graph
        losses = [float(step.step(u, y, noise, True)) for _ in range(3)]
        torch.cuda.synchronize()
        res[graph] = (losses, opt.flat.clone())
    assert res[True][0] == res[False][0]
    assert torch.equal(res[True][1], res[False][1])
    assert res[True][0][2] != res[True][0][0]
