"""The GRU recognition model's two HIP kernels through the C ABI (cbfssm_gru_recog_f64 / _bwd_f64; reference
cbfssm/model/cbfssmhalf.py:82-93) against the committed float64 restatement (oracle.cbfssm_torch_ref.gru_recognition) and its
autograd, at the kernels' stated limits, the long windows of the real workloads, the special shapes and both sides of the
two-stage slab reduction; then the engine's CBFSSM_TORCH_GRU=1 cross-check path and the captured train step.

The rule is derived per case, not fixed in advance.  The same oracle is run in float32 on the same (float32-valued)
inputs; the relative error of a tensor of that run against the float64 run, divided by 2^-24, is the tensor's
amplification A: how many unit round-offs of the arithmetic the function turns into relative error of the result.  A
float64 kernel must then satisfy, element-wise,

    |got - ref| <= 16 * max(A, 1) * 2^-53 * max|ref|

for x_0, every kept activation block and each of the six gradient tensors (the x rows and the h rows of the two kernels
are blocks of their own, each against its own largest reference entry).  16 covers another operation order inside the
wave (fma chains), the factor 3 by which A tracks the float64 oracle's own error against an 80-bit evaluation
(tests/test_gru_recog_abi.py measures that on the CPU) and the device's exp / tanh being 1-2 ulp where libm is at most 1.
x_0 and the activations take the A of x_0; a gradient block takes the larger of that and its own A, because the
conditioning of the reverse sweep is not the forward's (a gate at pre-activation -40 leaves x_0 alone but puts exp(-40),
with a relative error of 40 round-offs, into every gate gradient).  Condition, asserted first: every A of the case is
<= 64, and the relative bound stays below 1e-12, so the test cannot go vacuous.

Every test prints its figures before it asserts (lines starting with GRU_RECOG_RECORD: run with -s to keep them;
profiles/gru_recog/ holds one such run)."""
import functools

import numpy as np
import pytest
import torch

from cbfssm.hip import lib, ops
from cbfssm.hip import train_half
from cbfssm.hip.train import TFAdam
from cbfssm.hip.train_half import RECOG_NAMES, HipHalfGrad, HipHalfTrainStep, half_param_names

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
H = 16                    # GRUCell(16), cbfssmhalf.py:84
EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53
FACTOR, A_MAX, CAP = 16.0, 64.0, 1e-12
NAMES = ('Wg', 'bg', 'Wc', 'bc', 'Wd', 'bd')                 # the flat vector's order (include/cbfssm_hip.h)
ORACLE_NAMES = ('gate_kernel', 'gate_bias', 'cand_kernel', 'cand_bias', 'dense_kernel', 'dense_bias')
GUARD, SENTINEL = 8, -7.25                                   # guard words on both sides of every output buffer


def _f32(a):
    """rounded to float32 and widened again: the casts of the float32 run are then exact, not part of the comparison"""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _fixture(seed, B, R, dim_u, dim_y, dim_x, T=None, saturate=None):
    """one default_rng(seed); draws in the order gate kernel, gate bias, candidate kernel, candidate bias, dense kernel, dense
    bias, u, y, gx0: weights 0.3 N(0,1), biases 0.1 N(0,1) (gate bias + 1), T = R + 3 unless given; gx0 stays float64,
    everything else is a float32 value.  At these scales the float64 oracle is 2-5 ulp from an 80-bit evaluation; at weights
    1.5 N(0,1) and R >= 50 the recurrence is chaotic and the oracle itself is 1e4-1e7 ulp off.
    saturate: the gate bias becomes +-saturate; unit j has r at (-1)^j and u at (-1)^(j // 2) times it: all four pairs occur,
    among them r = 1 with u = exp(-40) (the state follows the candidate, r o h is of order one)."""
    rng = np.random.default_rng(seed)
    n_in, T = dim_u + dim_y, (R + 3 if T is None else T)
    fx = {'Wg': _f32(0.3 * rng.standard_normal((n_in + H, 2 * H))), 'bg': _f32(1.0 + 0.1 * rng.standard_normal(2 * H)),
          'Wc': _f32(0.3 * rng.standard_normal((n_in + H, H))), 'bc': _f32(0.1 * rng.standard_normal(H)),
          'Wd': _f32(0.3 * rng.standard_normal((H, dim_x))), 'bd': _f32(0.1 * rng.standard_normal(dim_x)),
          'u': _f32(rng.standard_normal((B, T, dim_u))), 'y': _f32(rng.standard_normal((B, T, dim_y)))}
    fx['gx0'] = rng.standard_normal((B, dim_x))
    if saturate is not None:
        j = np.arange(H)
        fx['bg'] = _f32(fx['bg'] - 1.0 + saturate * (1.0 - 2.0 * np.concatenate((j % 2, (j // 2) % 2))))
    fx.update(B=B, R=R, T=T, dim_u=dim_u, dim_y=dim_y, dim_x=dim_x, n_in=n_in)
    return fx


# name -> (seed, B, R, dim_u, dim_y, dim_x, T or None, saturate or None): the smallest shapes that reach each edge
CASES = {
    'one-step-no-u': (1, 3, 1, 0, 1, 1, None, None),          # one step, null u pointer, one output
    'both-limits': (2, 5, 16, 16, 16, 16, None, None),        # n_in = 32 and dim_x = 16: every accumulator row in use
    'all-from-y': (3, 4, 3, 0, 32, 16, None, None),           # 32 inputs, all from y
    'all-from-u': (4, 4, 3, 31, 1, 2, None, None),            # 32 inputs, almost all from u
    'sarcos-long': (5, 2, 64, 7, 7, 14, None, None),          # long window at the Sarcos widths
    'c5-window': (6, 9, 50, 2, 2, 4, None, None),             # the C5 window
    'odd': (7, 33, 5, 3, 2, 6, None, None),                   # n_in + 16 = 21 rows: no multiple of 2 or 4
    'whole-sequence': (8, 6, 7, 2, 1, 3, 7, None),            # recog_len = T: the T stride of gru_input
    'B127': (9, 127, 4, 8, 15, 16, None, None),               # the widest shape the models reach (D = 24), on both
    'B128': (9, 128, 4, 8, 15, 16, None, None),               # sides of the two-stage reduction (nwg >= 128)
    'B129': (9, 129, 4, 8, 15, 16, None, None),
    'saturated': (10, 4, 3, 2, 1, 3, None, 40.0),             # gate pre-activations of about +-40
}
SHAPE_CASES = [k for k in CASES if k != 'saturated']


def _restate(fx, dtype=np.float64):
    """the oracle's eight lines in numpy at `dtype`, returning the intermediates the kernel keeps:
    (x0 (B, dim_x), act (B, R, 64): h before the step | r | u | c, h after the last step (B, 16))"""
    c = {k: fx[k].astype(dtype) for k in NAMES + ('u', 'y')}
    B, R, one = fx['B'], fx['R'], dtype(1)
    uy = np.concatenate((c['u'], c['y']), axis=2)[:, :R, :][:, ::-1, :]
    h = np.zeros((B, H), dtype=dtype)
    act = np.zeros((B, R, 4, H), dtype=dtype)
    for t in range(R):
        x = uy[:, t, :]
        gates = one / (one + np.exp(-(np.concatenate((x, h), axis=1) @ c['Wg'] + c['bg'])))
        r, z = gates[:, :H], gates[:, H:]
        cand = np.tanh(np.concatenate((x, r * h), axis=1) @ c['Wc'] + c['bc'])
        act[:, t, 0], act[:, t, 1], act[:, t, 2], act[:, t, 3] = h, r, z, cand
        h = z * h + (one - z) * cand
    return h @ c['Wd'] + c['bd'], act.reshape(B, R, 4 * H), h


def _oracle(fx, dtype=torch.float64):
    """(x0, the six gradients of (x0 * gx0).sum()) of oracle.cbfssm_torch_ref.gru_recognition at `dtype`, as float64 arrays"""
    from oracle import cbfssm_torch_ref as tref
    rp = {o: torch.tensor(fx[k], dtype=dtype, requires_grad=True) for k, o in zip(NAMES, ORACLE_NAMES)}
    x0 = tref.gru_recognition(rp, torch.tensor(fx['u'], dtype=dtype), torch.tensor(fx['y'], dtype=dtype), fx['R'])
    g = torch.autograd.grad((x0 * torch.tensor(fx['gx0'], dtype=dtype)).sum(), list(rp.values()))
    return x0.detach().numpy().astype(np.float64), {k: t.numpy().astype(np.float64) for k, t in zip(NAMES, g)}


def _blocks(fx, grads):
    """the gradient blocks that are judged on their own: the x rows (i < n_in) and the h rows of the gate and candidate
    kernels separately, the other four tensors whole"""
    out, n_in = {}, fx['n_in']
    for k in NAMES:
        if k in ('Wg', 'Wc'):
            out['g%s.x-rows' % k], out['g%s.h-rows' % k] = grads[k][:n_in], grads[k][n_in:]
        else:
            out['g' + k] = grads[k]
    return out


def _rel(a, ref):
    scale = np.abs(ref).max()
    return float(np.abs(a - ref).max() / scale) if scale else 0.0


def _amplification(fx, x0, grads):
    """{'x0': A, block: A}: the float32 oracle's relative error against the float64 one in units of 2^-24"""
    x0_32, g32 = _oracle(fx, torch.float32)
    A = {'x0': _rel(x0_32, x0) / EPS32}
    b32, b64 = _blocks(fx, g32), _blocks(fx, grads)
    A.update({k: _rel(b32[k], b64[k]) / EPS32 for k in b64})
    return A


@functools.lru_cache(maxsize=None)
def _case(name):
    """fixture and float64 references of a case, computed once and shared by the tests (never written to)"""
    seed, B, R, dim_u, dim_y, dim_x, T, sat = CASES[name]
    fx = _fixture(seed, B, R, dim_u, dim_y, dim_x, T, sat)
    x0, grads = _oracle(fx)
    x0_r, act, hR = _restate(fx)
    A = _amplification(fx, x0, grads)
    for v in [x0, act, hR] + list(grads.values()) + [a for a in fx.values() if isinstance(a, np.ndarray)]:
        v.setflags(write=False)
    return {'name': name, 'fx': fx, 'x0': x0, 'grads': grads, 'x0_restated': x0_r, 'act': act, 'hR': hR, 'A': A}


def _rule(A):
    """the relative bound of a tensor with amplification A"""
    return FACTOR * max(A, 1.0) * EPS64


def _check_condition(case):
    """asserted before anything is compared: the fixture is well conditioned and its bound is not vacuous"""
    A = case['A']
    print('GRU_RECOG_RECORD case=%s A: %s' % (case['name'], ' '.join('%s=%.2f' % kv for kv in A.items())))
    assert max(A.values()) <= A_MAX, (case['name'], A)
    assert _rule(max(A.values())) < CAP


def _judge(case, what, got, ref, A, bad):
    """element-wise |got - ref| <= 16 max(A, 1) 2^-53 max|ref|; prints the achieved err / bound"""
    scale = float(np.abs(ref).max())
    if scale == 0.0:                                         # (the h rows at R = 1): exactly zero from the kernel too
        ok = bool(np.all(got == 0.0))
        print('GRU_RECOG_RECORD case=%s tensor=%s reference is zero, kernel %s' % (case['name'], what, 'zero' if ok else 'NOT zero'))
    else:
        bound = _rule(A) * scale
        err = float(np.abs(got - ref).max())
        ok = bool(np.all(np.isfinite(got))) and bool(np.all(np.abs(got - ref) <= bound))
        print('GRU_RECOG_RECORD case=%s tensor=%s A=%.2f max|ref|=%.3e err=%.3e bound=%.3e err/bound=%.4f'
              % (case['name'], what, A, scale, err, bound, err / bound))
    if not ok:
        bad.append(what)


def _guarded(n, fill=float('nan')):
    t = torch.full((n + 2 * GUARD,), fill, dtype=torch.float64, device=DEV)
    t[:GUARD] = SENTINEL
    t[n + GUARD:] = SENTINEL
    return t


def _guards_untouched(t):
    o = t.cpu().numpy()
    return bool(np.all(o[:GUARD] == SENTINEL) and np.all(o[-GUARD:] == SENTINEL))


def _inputs(fx):
    """(u or None, y, the flat parameter vector) on the device; dim_u = 0 passes a null u pointer"""
    u = torch.tensor(fx['u'], device=DEV).contiguous() if fx['dim_u'] else None
    prm = torch.tensor(np.concatenate([fx[k].reshape(-1) for k in NAMES]), device=DEV)
    return u, torch.tensor(fx['y'], device=DEV).contiguous(), prm


def _dims(fx):
    return fx['B'], fx['T'], fx['dim_u'], fx['dim_y'], fx['dim_x'], fx['R']


def _forward(fx, keep=True):
    """(x0 (B, dim_x), the act buffer on the device or None) of cbfssm_gru_recog_f64; both buffers start as NaN between
    guard words: every entry must be written, nothing outside"""
    l = lib.load()
    B, R, dx = fx['B'], fx['R'], fx['dim_x']
    u, y, prm = _inputs(fx)
    nact = int(l.cbfssm_gru_recog_act_elems(B, R))
    assert nact == B * R * 64 + B * H
    x0 = _guarded(B * dx)
    act = _guarded(nact) if keep else None
    rc = l.cbfssm_gru_recog_f64(*_dims(fx), ops._ptr(u), ops._ptr(y), ops._ptr(prm), ops._ptr(x0[GUARD:]),
                                ops._ptr(act[GUARD:]) if keep else None, ops._stream())
    lib.check(rc, 'cbfssm_gru_recog_f64')
    torch.cuda.synchronize()
    assert _guards_untouched(x0) and (act is None or _guards_untouched(act))
    x0 = x0[GUARD:GUARD + B * dx].cpu().numpy().reshape(B, dx)
    assert np.all(np.isfinite(x0))
    if keep:
        act = act[GUARD:GUARD + nact].clone()
        assert bool(torch.isfinite(act).all())
    return x0, act


def _backward(fx, act):
    """(slabs (B, P), their fixed-order sum (P,)) of cbfssm_gru_recog_bwd_f64 + cbfssm_reduce_partials_f64.  gpart starts as
    NaN: the kernel writes and does not add, so every entry of the B slabs comes back finite, and the scratch slabs behind
    them keep their bits until the reduction uses them."""
    l = lib.load()
    B = fx['B']
    P = int(l.cbfssm_gru_recog_param_elems(fx['dim_u'], fx['dim_y'], fx['dim_x']))
    assert P == (fx['n_in'] + H) * 48 + 48 + H * fx['dim_x'] + fx['dim_x']
    u, y, prm = _inputs(fx)
    gx0 = torch.tensor(fx['gx0'], device=DEV)
    gpart = _guarded((B + 32) * P)                           # + CBFSSM_REDUCE_SPLIT scratch slabs
    before = gpart.cpu().numpy().view(np.int64).copy()
    rc = l.cbfssm_gru_recog_bwd_f64(*_dims(fx), ops._ptr(u), ops._ptr(y), ops._ptr(prm), ops._ptr(act), ops._ptr(gx0),
                                    ops._ptr(gpart[GUARD:]), ops._stream())
    lib.check(rc, 'cbfssm_gru_recog_bwd_f64')
    torch.cuda.synchronize()
    after = gpart.cpu().numpy()
    slabs = after[GUARD:GUARD + B * P].reshape(B, P).copy()
    assert np.all(np.isfinite(slabs)), 'an entry of a slab was not written'
    assert np.array_equal(after.view(np.int64)[GUARD + B * P:], before[GUARD + B * P:]), 'the kernel wrote behind its B slabs'
    assert _guards_untouched(gpart)
    out = _guarded(P)
    ops.reduce_partials(gpart[GUARD:GUARD + (B + 32) * P], P, B, out[GUARD:GUARD + P], ops._stream())
    torch.cuda.synchronize()
    assert _guards_untouched(gpart) and _guards_untouched(out)
    assert np.array_equal(gpart[GUARD:GUARD + B * P].cpu().numpy().reshape(B, P), slabs), 'the reduction changed its inputs'
    return slabs, out[GUARD:GUARD + P].cpu().numpy()


def _split(fx, flat):
    out, o = {}, 0
    for k in NAMES:
        out[k] = flat[o:o + fx[k].size].reshape(fx[k].shape)
        o += fx[k].size
    assert o == flat.size
    return out


def _check_forward(case, bad):
    """x0 against the oracle; the kept activations against the restatement, whose x0 must first equal the oracle's"""
    fx, A = case['fx'], case['A']['x0']
    B, R = fx['B'], fx['R']
    assert np.abs(case['x0_restated'] - case['x0']).max() <= 4 * 2.0 ** -52 * np.abs(case['x0']).max()
    x0, act = _forward(fx)
    _judge(case, 'x0', x0, case['x0'], A, bad)
    act = act.cpu().numpy()
    steps, hR = act[:B * R * 64].reshape(B, R, 4, H), act[B * R * 64:].reshape(B, H)
    ref = case['act'].reshape(B, R, 4, H)
    for j, blk in enumerate(('h', 'r', 'u', 'c')):           # (R = 1: h before the only step is the zero start, exactly)
        _judge(case, 'act.' + blk, steps[:, :, j], ref[:, :, j], A, bad)
    _judge(case, 'act.h_final', hR, case['hR'], A, bad)
    x0_nokeep, _ = _forward(fx, keep=False)
    assert np.array_equal(x0_nokeep, x0), 'x0 without kept activations differs'
    return act


def _check_backward(case, bad):
    """the six gradient tensors after the fixed-order reduction; x rows and h rows of the two kernels separately"""
    fx, n_in = case['fx'], case['fx']['n_in']
    _, act = _forward(fx)
    _, total = _backward(fx, act)
    got = _split(fx, total)
    ref = _blocks(fx, case['grads'])
    for k, g in _blocks(fx, got).items():
        _judge(case, k, g, ref[k], max(case['A']['x0'], case['A'][k]), bad)
    if fx['R'] == 1:                                         # h = 0 before the only step: no gradient reaches the h rows
        assert not case['grads']['Wg'][n_in:].any() and not case['grads']['Wc'][n_in:].any()
        assert not got['Wg'][n_in:].any() and not got['Wc'][n_in:].any()


@pytest.mark.parametrize('name', SHAPE_CASES)
def test_forward_against_the_float64_oracle(name):
    case = _case(name)
    _check_condition(case)
    bad = []
    _check_forward(case, bad)
    assert not bad, (name, bad)


@pytest.mark.parametrize('name', SHAPE_CASES)
def test_gradients_against_float64_autograd(name):
    case = _case(name)
    _check_condition(case)
    bad = []
    _check_backward(case, bad)
    assert not bad, (name, bad)


def test_saturated_gates():
    """gate pre-activations of about +-40: r and u are 1 exactly or about exp(-40); x0 and every gradient stay finite and inside
    the same rule (the gate gradients are of order exp(-40) and take their own amplification, about 40 round-offs).
    Measured: the x rows of the gate-kernel gradient at 0.76 of their bound, every other block below 0.45 -- the kernels
    start a gate column's fma chain at the bias, which rounds every partial sum at ulp(40) (profiles/gru_recog/)."""
    case = _case('saturated')
    _check_condition(case)
    fx = case['fx']
    pre = np.concatenate((fx['u'], fx['y']), axis=2)[:, :fx['R']] @ fx['Wg'][:fx['n_in']] + fx['bg']
    print('GRU_RECOG_RECORD case=saturated |gate pre-activation of the input part| in [%.1f, %.1f]' % (np.abs(pre).min(), np.abs(pre).max()))
    assert np.abs(pre).min() > 30.0
    gates = case['act'].reshape(fx['B'], fx['R'], 4, H)[:, :, 1:3]
    assert (gates == 1.0).any() and (gates < 1e-15).any()
    bad = []
    _check_forward(case, bad)
    _check_backward(case, bad)
    assert not bad, bad


def _run(fx):
    x0, act = _forward(fx)
    slabs, total = _backward(fx, act)
    return x0, act.cpu().numpy(), slabs, total


def test_reproducible_and_independent_of_the_batch():
    fx = _case('odd')['fx']
    first, second = _run(fx), _run(fx)
    assert all(np.array_equal(a, b) for a, b in zip(first, second))
    x0, _, slabs, _ = first
    for b in (0, 17, 32):                                   # the same sequence alone: bitwise the slab it has inside the batch
        one = dict(fx, B=1, u=fx['u'][b:b + 1], y=fx['y'][b:b + 1], gx0=fx['gx0'][b:b + 1])
        x1, _, s1, t1 = _run(one)
        assert np.array_equal(s1[0], slabs[b]) and np.array_equal(t1, slabs[b])
        assert np.array_equal(x1[0], x0[b])


# ---- the engine: the fused kernels against the tensor-library restatement, and the captured step -----------------------
def _engine_setup(variant, **kw):
    from test_oracle import _half_setup, _prssm_setup
    return (_prssm_setup if variant == 'prssm' else _half_setup)('rnn', **kw)


def _raise(*a, **k):
    raise AssertionError('the tensor-library GRU recogniser ran')


TINY = dict(T=6, B=2, S=3, M=6, recog_len=3)
WIDE = dict(dim_x=16, dim_u=8, dim_y=15, M=20, T=6, recog_len=6, B=3, S=3)


@pytest.mark.parametrize('variant', ['half', 'prssm'])
@pytest.mark.parametrize('name,kw', [('tiny', TINY), ('wide', WIDE)])
def test_engine_fused_kernels_equal_the_tensor_library_path(monkeypatch, name, kw, variant):
    """HipHalfGrad with the two launches against the same engine under CBFSSM_TORCH_GRU=1 (the tensor library's autograd
    through train_half.gru_recognition): the loss to rel 1e-12, every gradient within 1e-11 of its tensor's largest entry"""
    w, cfg, p, u, y, noise = _engine_setup(variant, **kw)
    params = {k: torch.tensor(v, device=DEV) for k, v in p.items()}
    with monkeypatch.context() as m:
        m.delenv('CBFSSM_TORCH_GRU', raising=False)
        m.setattr(train_half, 'gru_recognition', _raise)
        eng = HipHalfGrad(cfg, DEV, variant=variant)
        assert eng.fused_gru
        l1, g1, _ = eng.loss_and_grads(params, u, y, noise, True)
        l1, g1 = float(l1), {k: v.clone() for k, v in g1.items()}
    monkeypatch.setenv('CBFSSM_TORCH_GRU', '1')
    eng2 = HipHalfGrad(cfg, DEV, variant=variant)
    assert not eng2.fused_gru
    l2, g2, _ = eng2.loss_and_grads(params, u, y, noise, True)
    l2 = float(l2)
    assert set(g1) == set(g2) == set(half_param_names(cfg, variant)) and set(RECOG_NAMES) <= set(g1)
    errs = {k: float((g1[k] - g2[k]).abs().max() / (g2[k].abs().max() + 1e-300)) for k in g2}
    print('GRU_RECOG_RECORD engine %s %s loss rel=%.3e worst grad err=%.3e (%s)'
          % (name, variant, abs(l1 - l2) / abs(l2), max(errs.values()), max(errs, key=errs.get)))
    assert abs(l1 - l2) <= 1e-12 * abs(l2), (l1, l2)
    assert all(float(g2[k].abs().max()) > 0 for k in RECOG_NAMES)
    assert all(e <= 1e-11 for e in errs.values()), errs


def test_graph_replay_equals_eager_steps_bit_for_bit(monkeypatch):
    """every launch of the step is deterministic with fixed-order reductions: three replays of the captured step leave the
    parameters and losses of three eager steps"""
    monkeypatch.delenv('CBFSSM_TORCH_GRU', raising=False)
    w, cfg, p, u, y, noise = _engine_setup('half', T=9, B=3, S=4, M=12, recog_len=4)
    res = {}
    for graph in (True, False):
        eng = HipHalfGrad(cfg, DEV)
        assert eng.fused_gru
        opt = TFAdam({k: torch.tensor(p[k], device=DEV) for k in half_param_names(cfg)}, 0.01)
        step = HipHalfTrainStep(eng, opt, graph=graph)
        assert step.use_graph == graph
        losses = [float(step.step(u, y, noise, True)) for _ in range(3)]
        torch.cuda.synchronize()
        res[graph] = (losses, opt.flat.clone())
    assert res[True][0] == res[False][0]
    assert torch.equal(res[True][1], res[False][1])
    assert res[True][0][2] != res[True][0][0]
