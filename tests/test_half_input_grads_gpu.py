"""d loss / d u and d loss / d y of the forward-only variants (HipHalfGrad.loss_and_grads(..., input_grads=True), variants 'half'
and 'prssm', the three recognisers; cbfssm.hip.autograd.elbo_loss on such an engine) against reverse-mode autodiff of the
float64 restatement (oracle/cbfssm_torch_ref.half_elbo_step / prssm_elbo_step with u and y requiring grad), and the new entry
points through the C ABI.

Tolerances, all taken from the project:
  float64 paths (rnn, output, the time-loop part): the rule of tests/test_hip_grad.py through input_grads_cases.within_rule,
      every entry within 1e-6 of the largest entry of its tensor -- on the window rows t < recog_len and on the rows behind
      them separately, each against its own largest reference entry, and where D > 16 on the u channels with GP-input row
      j >= 16 on their own; the parameter gradients of the same call by the rule of tests/test_prssm_gpu.py (1e-6; 1e-3 with
      the float32 conv recogniser), the loss to rel 1e-9 (1e-6 with the conv recogniser).
  conv window rows: the rule of tests/test_conv_recog_gpu.py::test_gradients_against_float64_autograd,
      e_kernel <= 4 e_ref + 2^-23 with e = max|g - g_truth| / max|g_truth|, g_truth from the float64 evaluation of the conv
      recogniser, e_ref the float32 oracle's own error; fixtures whose relu masks and pooling winners are >= 64 rounding
      bounds from flipping (asserted first, on the CPU).
  GRU gwin at the ABI level: tests/test_gru_recog_gpu.py::_judge, |got - ref| <= 16 max(A, 1) 2^-53 max|ref| element-wise.

Every test prints its figures before it asserts (lines starting with HALF_IN_RECORD: run with -s to keep them;
profiles/half_input_gradients/ holds one such run)."""
import ctypes as C

import numpy as np
import pytest
import torch

from cbfssm.hip import lib, ops
from cbfssm.hip.train_half import HipHalfGrad, half_param_names

import half_input_grads_cases as hc
from half_input_grads_cases import within_rule

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _params(p, grad=False):
    return {k: torch.tensor(v, device=DEV, requires_grad=grad) for k, v in p.items()}


def _conv_rule(tag, g, g_ref, g_truth):
    """e_kernel <= 4 e_ref + 2^-23 (tests/test_conv_recog_gpu.py), e = max|g - g_truth| / max|g_truth|"""
    scale = np.abs(g_truth).max()
    e_ker, e_ref = np.abs(g - g_truth).max() / scale, np.abs(g_ref - g_truth).max() / scale
    bound = 4 * e_ref + 2.0 ** -23
    print('%-40s max|truth| %.3e e_kernel %.3e e_ref %.3e err/bound %.4f' % (tag, scale, e_ker, e_ref, e_ker / bound))
    assert e_ker <= bound, (tag, e_ker, e_ref)


def _judge_engine(name, cond, cfg, w, loss, grads, tag=''):
    """loss, parameter gradients, d loss / d u and d loss / d y of one engine call against the oracle of the case"""
    variant, recog = hc.CASES[name][:2]
    truth = hc.oracle(name, cond, True) if recog == 'conv' else None
    _judge_reference(name, variant, hc.oracle(name, cond), cond, cfg, w, loss, grads, tag=tag, truth=truth)


def _judge_reference(name, variant, ref, cond, cfg, w, loss, grads, tag='', truth=None):
    """the same against a reference handed in (half_input_grads_cases.oracle_run of any set-up: the tile-grid rows of
    tests/test_input_grads_tile_grid_gpu.py); truth: the reference with the conv recogniser in float64, conv cases only"""
    conv = truth is not None
    loss_ref, gref, gu_ref, gy_ref = ref
    hc.assert_reference_structure(name, cfg, gu_ref, gy_ref)
    gu, gy = grads['u'].cpu().numpy(), grads['y'].cpu().numpy()
    assert gu.shape == gu_ref.shape and gy.shape == gy_ref.shape
    R = hc.window_rows(cfg, w.T)
    tag = 'HALF_IN_RECORD %s%s cond=%d ' % (tag, name, cond)
    perr = {k: float(np.abs(grads[k].cpu().numpy() - gref[k]).max() / (np.abs(gref[k]).max() + 1e-300)) for k in gref}
    # printed before anything is asserted
    print('%sloss rel %.2e worst parameter gradient %.2e (%s)' % (tag, abs(float(loss) - loss_ref) / abs(loss_ref),
                                                                max(perr.values()), max(perr, key=perr.get)))
    for nm, g, r in (('u', gu, gu_ref), ('y', gy, gy_ref)):
        for what, sl in (('window', slice(0, R)), ('rest', slice(R, None))):
            if r[:, sl].size and np.abs(r[:, sl]).max() > 0:
                print('%s%s %s max|ref| %.3e err/max %.2e' % (tag, nm, what, np.abs(r[:, sl]).max(),
                                                              np.abs(g[:, sl] - r[:, sl]).max() / np.abs(r[:, sl]).max()))
    assert np.isfinite(gu).all() and np.isfinite(gy).all()
    assert float(loss) == pytest.approx(loss_ref, rel=1e-6 if conv else 1e-9)
    assert set(perr) == set(half_param_names(cfg, variant))
    assert all(e < (1e-3 if conv else 1e-6) for e in perr.values()), perr
    if w.T - 1 >= R and w.dim_u:
        assert not gu[:, w.T - 1].any(), 'd loss / d u must be exactly zero at t = T - 1: the last input feeds nothing'
    if conv:
        _, _, gu_t, gy_t = truth
        _conv_rule(tag + 'u window rows', gu[:, :R], gu_ref[:, :R], gu_t[:, :R])
        _conv_rule(tag + 'y window rows', gy[:, :R], gy_ref[:, :R], gy_t[:, :R])
        within_rule(tag + 'u rows t>=R', gu[:, R:w.T - 1], gu_ref[:, R:w.T - 1])
        within_rule(tag + 'y rows t>=R', gy[:, R:], gy_ref[:, R:])
    else:
        hc.rows_within_rule(tag + 'd loss/d u', gu, gu_ref, R)
        hc.rows_within_rule(tag + 'd loss/d y', gy, gy_ref, R)
        if w.D > 16:        # the u channels in the second 16-row block of gp_f's input (row dim_x + k), on their own
            ku = max(0, 16 - w.dim_x)
            assert ku < w.dim_u
            hc.rows_within_rule(tag + 'u rows j>=16 of gp_f', gu, gu_ref, R, sel=slice(ku, None))


def _run(name, cond, **over):
    variant, w, cfg, p, u, y, noise = hc.setup(name)
    cfg = dict(cfg, **over)
    eng = HipHalfGrad(cfg, DEV, variant=variant)
    loss, grads, terms = eng.loss_and_grads(_params(p), u, y, noise, condition=cond, input_grads=True)
    assert float(terms['info']) == 0.0
    return eng, cfg, w, loss, grads


@pytest.mark.parametrize('name,cond', [(n, c) for n in sorted(hc.CASES) for c in hc.CONDS(n)])
def test_input_gradients_match_oracle(monkeypatch, name, cond):
    for k in ('CBFSSM_TORCH_GRU', 'CBFSSM_TORCH_CONV', 'CBFSSM_GP_FORM'):
        monkeypatch.delenv(k, raising=False)
    eng, cfg, w, loss, grads = _run(name, cond)
    recog = hc.CASES[name][1]
    assert eng.stash == (w.M > 112) and eng.fused_gru == (recog == 'rnn') and eng.fused_conv == (recog == 'conv')
    assert set(grads) == set(half_param_names(cfg, eng.variant)) | {'u', 'y'}
    _judge_engine(name, cond, cfg, w, loss, grads)


@pytest.mark.parametrize('name', ['half-rnn', 'prssm-rnn'])
def test_two_triangular_gp_form(monkeypatch, name):
    monkeypatch.setenv('CBFSSM_GP_FORM', 'tri')
    eng, cfg, w, loss, grads = _run(name, True)
    assert eng.pack_f.gp_form() == 'tri'
    _judge_engine(name, True, cfg, w, loss, grads, tag='tri ')


@pytest.mark.parametrize('name,env', [('half-rnn', 'CBFSSM_TORCH_GRU'), ('prssm-conv', 'CBFSSM_TORCH_CONV')])
def test_tensor_library_recognisers_deliver_the_window_adjoint(monkeypatch, name, env):
    """the cross-check recognisers (the window's adjoint from the tensor library's autograd) by the rules of the fused path,
    and against the fused path itself"""
    monkeypatch.delenv(env, raising=False)
    _, _, _, _, g_fused = _run(name, True)
    gu_f, gy_f = g_fused['u'].clone(), g_fused['y'].clone()
    monkeypatch.setenv(env, '1')
    eng, cfg, w, loss, grads = _run(name, True)
    assert not eng.fused_gru and not eng.fused_conv
    _judge_engine(name, True, cfg, w, loss, grads, tag='tensor-library ')
    # against the fused path itself: window rows and the rows behind them, each within 1e-6 of its own largest entry (the
    # rule of tests/test_hip_grad.py; both codings of the conv are float32, each also inside the conv rule above)
    R = hc.window_rows(cfg, w.T)
    for nm, a, b in (('u', grads['u'], gu_f), ('y', grads['y'], gy_f)):
        hc.rows_within_rule('HALF_IN_RECORD tensor-library %s vs fused d loss/d %s' % (name, nm), a.cpu().numpy(),
                            b.cpu().numpy(), R)


@pytest.mark.parametrize('name', ['half-rnn-stash', 'prssm-rnn-stash'])
def test_stash_mode_time_chunks_write_their_own_range_only(monkeypatch, name):
    """adjoint_stash_gib = 3e-4 holds four steps per launch: several time-chunked launches, the bits of the single-chunk run"""
    calls = {'n': 0}
    f0 = ops.TimeLoops.half_forward_pass_bwd

    def counted(self, *a, **k):
        calls['n'] += 1
        return f0(self, *a, **k)
    monkeypatch.setattr(ops.TimeLoops, 'half_forward_pass_bwd', counted)
    eng, _, _, _, g1 = _run(name, True)
    assert eng.stash
    chunked = calls['n']
    u1, y1 = g1['u'].clone(), g1['y'].clone()
    calls['n'] = 0
    eng0, _, _, _, g0 = _run(name, True, adjoint_stash_gib=4.0)
    print('HALF_IN_RECORD %s adjoint launches: single-chunk %d, small budget %d' % (name, calls['n'], chunked))
    assert calls['n'] == 1 and chunked >= 2
    assert float(u1.abs().max()) > 0 and float(y1.abs().max()) > 0
    assert torch.equal(u1, g0['u']) and torch.equal(y1, g0['y'])


@pytest.mark.parametrize('name', ['half-rnn', 'prssm-conv', 'half-output'])
def test_repeat_and_chain_group_switches_are_bitwise_invisible(monkeypatch, name):
    variant, w, cfg, p, u, y, noise = hc.setup(name, B=3, S=13)          # 39 chains = 3 groups of 16, the last one ragged
    params = _params(p)
    eng = HipHalfGrad(cfg, DEV, variant=variant)
    _, g0, _ = eng.loss_and_grads(params, u, y, noise, input_grads=True)
    u0, y0 = g0['u'].clone(), g0['y'].clone()
    assert float(u0.abs().max()) > 0.0 and float(y0.abs().max()) > 0.0
    _, g1, _ = eng.loss_and_grads(params, u, y, noise, input_grads=True)
    assert torch.equal(u0, g1['u']) and torch.equal(y0, g1['y'])
    for env, val in (('CBFSSM_NO_SPLIT', '1'), ('CBFSSM_SPLIT_MAIN', '1'), ('CBFSSM_SPLIT_MAIN', '2')):
        with monkeypatch.context() as m:
            m.setenv(env, val)
            _, g2, _ = HipHalfGrad(cfg, DEV, variant=variant).loss_and_grads(params, u, y, noise, input_grads=True)
            assert torch.equal(u0, g2['u']) and torch.equal(y0, g2['y']), (env, val)


@pytest.mark.parametrize('name', ['half-rnn', 'prssm-conv', 'prssm-rnn-stash'])
def test_default_call_is_untouched_by_a_call_with_input_gradients(name):
    variant, w, cfg, p, u, y, noise = hc.setup(name)
    eng = HipHalfGrad(cfg, DEV, variant=variant)
    l0, g0, _ = eng.loss_and_grads(_params(p), u, y, noise)
    assert set(g0) == set(half_param_names(cfg, variant))
    l0, g0 = float(l0), {k: v.clone() for k, v in g0.items()}
    eng.loss_and_grads(_params(p), u, y, noise, input_grads=True)
    l1, g1, _ = eng.loss_and_grads(_params(p), u, y, noise, input_grads=False)
    assert float(l1) == l0 and set(g1) == set(g0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k


@pytest.mark.parametrize('name', ['half-rnn', 'half-rnn-stash'])
def test_workspace_buffers_are_reused_across_condition_values_and_inputs(name):
    """one engine keeps gin_f, gyo, gwin and the two results with its workspace: a call with condition=True, one with other
    inputs, then condition=False must return the bits of a fresh engine (the adjoint writes zeros into gyo on the steps
    that do not condition; nothing is left over from the call before)"""
    variant, w, cfg, p, u, y, noise = hc.setup(name)
    params = _params(p)
    _, g_fresh, _ = HipHalfGrad(cfg, DEV, variant=variant).loss_and_grads(params, u, y, noise, condition=False, input_grads=True)
    u0, y0 = g_fresh['u'].clone(), g_fresh['y'].clone()
    eng = HipHalfGrad(cfg, DEV, variant=variant)
    _, g_true, _ = eng.loss_and_grads(params, u, y, noise, condition=True, input_grads=True)
    assert not torch.equal(g_true['y'], y0)                 # (conditioning matters for this set-up)
    eng.loss_and_grads(params, 1.5 * np.asarray(u) + 0.25, 0.5 * np.asarray(y) - 0.1, noise, condition=True, input_grads=True)
    _, g1, _ = eng.loss_and_grads(params, u, y, noise, condition=False, input_grads=True)
    assert torch.equal(g1['u'], u0) and torch.equal(g1['y'], y0)


# ---- the reduction through the ABI --------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['gwin', 'gx0'])
def test_reduction_reads_only_what_its_formulas_name(mode):
    """every buffer NaN except the entries the formulas read (row 0 of gyo, the hidden dims of gx0, the pack outside its
    1/lengthscale section are all NaN): no NaN comes out, the result is the formula's, two calls are bitwise identical"""
    from test_gru_recog_gpu import GUARD, _guarded, _guards_untouched
    l = lib.load()
    B, S, T, dx, du, dy, M, R, cL = 3, 5, 7, 4, 2, 3, 12, 4, 0.37
    N = B * S
    rng = np.random.default_rng(12)
    prob = lib.make_problem(B, S, T, dx, du, dy, M, 1, 1.0, False, half=True)
    lay = lib.pack_layout(M, dx + du, dx)
    invl = rng.uniform(0.5, 2.0, dx + du)
    pack = np.full(int(lay.total), np.nan)
    pack[int(lay.invl):int(lay.invl) + dx + du] = invl
    gin_f = rng.standard_normal((T - 1, du, N))
    gyo = rng.standard_normal((T, dy, N))
    gyo[0] = np.nan
    gx0 = np.full((N, dx), np.nan)
    gx0[:, :dy] = rng.standard_normal((N, dy))
    gwin = rng.standard_normal((B, R, du + dy))
    if mode == 'gwin':
        gx0[:] = np.nan
    else:
        gwin[:] = np.nan
    var_y, y, x = rng.uniform(0.1, 1.0, dy), rng.standard_normal((B, T, dy)), rng.standard_normal((T, N, dx))
    x[:, :, dy:] = np.nan                                    # the hidden dims of the trajectory are not read either
    d = {k: torch.tensor(v, device=DEV) for k, v in dict(pack=pack, gin_f=gin_f, gyo=gyo, gx0=gx0, gwin=gwin, var_y=var_y, y=y,
                                                         x=x).items()}
    outs = []
    for _ in range(2):
        gu, gy = _guarded(B * T * du), _guarded(B * T * dy)
        rc = l.cbfssm_half_input_grads_f64(C.byref(prob), C.byref(lay), ops._ptr(d['pack']), ops._ptr(d['var_y']), ops._ptr(d['y']),
                                           ops._ptr(d['x']), ops._ptr(d['gin_f']), ops._ptr(d['gyo']),
                                           ops._ptr(d['gx0']) if mode == 'gx0' else None,
                                           ops._ptr(d['gwin']) if mode == 'gwin' else None, R, cL,
                                           ops._ptr(gu[GUARD:]), ops._ptr(gy[GUARD:]), ops._stream())
        lib.check(rc, 'cbfssm_half_input_grads_f64')
        torch.cuda.synchronize()
        assert _guards_untouched(gu) and _guards_untouched(gy)
        outs.append((gu[GUARD:-GUARD].cpu().numpy().reshape(B, T, du), gy[GUARD:-GUARD].cpu().numpy().reshape(B, T, dy)))
    (gu, gy), (gu2, gy2) = outs
    assert np.isfinite(gu).all() and np.isfinite(gy).all(), 'an entry was not written, or a NaN was read'
    assert np.array_equal(gu, gu2) and np.array_equal(gy, gy2)
    ru, ry = np.zeros((B, T, du)), np.zeros((B, T, dy))
    ru[:, :T - 1] = (gin_f.reshape(T - 1, du, B, S).sum(3) * invl[dx:, None]).transpose(2, 0, 1)
    ry[:, 1:] = gyo[1:].reshape(T - 1, dy, B, S).sum(3).transpose(2, 0, 1)
    ry += cL * (y[:, :, None, :] - x[:, :, :dy].reshape(T, B, S, dy).transpose(1, 0, 2, 3)).sum(2) / var_y
    if mode == 'gwin':
        ru[:, :R] += gwin[:, :, :du]
        ry[:, :R] += gwin[:, :, du:]
    else:
        ry[:, 0] += gx0[:, :dy].reshape(B, S, dy).sum(1)
    # float64 sums of S = 5 terms of order one in another order: a few ulp of the largest term
    assert np.abs(gu - ru).max() <= 16 * 2.0 ** -52 * np.abs(ru).max()
    assert np.abs(gy - ry).max() <= 16 * 2.0 ** -52 * max(np.abs(ry).max(), cL * S * 4.0 / var_y.min())


# ---- the recognition kernels' window adjoint through the ABI ------------------------------------------------------------
def _gru_shape_cases():
    from test_gru_recog_gpu import SHAPE_CASES
    return SHAPE_CASES


@pytest.mark.parametrize('name', _gru_shape_cases())
def test_gru_window_adjoint_against_float64_autograd(name):
    import test_gru_recog_gpu as tg
    case, ref, A_win = hc.gru_window_case(name)
    fx = case['fx']
    B, R, n_in = fx['B'], fx['R'], fx['n_in']
    A = max(case['A']['x0'], A_win)
    print('GRU_RECOG_RECORD case=%s A(gwin)=%.2f A(x0)=%.2f' % (name, A_win, case['A']['x0']))
    assert A <= tg.A_MAX and tg._rule(A) < tg.CAP           # the fixture is well conditioned and the bound not vacuous
    for t in range(R):
        assert np.abs(ref[:, t]).max() > 0.0, ('the reference window adjoint is all zero at row', t)
    l = lib.load()
    _, act = tg._forward(fx)
    slabs0, _ = tg._backward(fx, act)                        # cbfssm_gru_recog_bwd_f64 on the same inputs
    P = slabs0.shape[1]
    u, y, prm = tg._inputs(fx)
    gx0 = torch.tensor(fx['gx0'], device=DEV)
    gpart, gwin = tg._guarded((B + 32) * P), tg._guarded(B * R * n_in)
    before = gpart.cpu().numpy().view(np.int64).copy()
    rc = l.cbfssm_gru_recog_bwd_in_f64(*tg._dims(fx), ops._ptr(u), ops._ptr(y), ops._ptr(prm), ops._ptr(act), ops._ptr(gx0),
                                       ops._ptr(gpart[tg.GUARD:]), ops._ptr(gwin[tg.GUARD:]), ops._stream())
    lib.check(rc, 'cbfssm_gru_recog_bwd_in_f64')
    torch.cuda.synchronize()
    assert tg._guards_untouched(gpart) and tg._guards_untouched(gwin)
    after = gpart.cpu().numpy()
    assert np.array_equal(after.view(np.int64)[tg.GUARD + B * P:], before[tg.GUARD + B * P:]), 'wrote behind the B slabs'
    slabs = after[tg.GUARD:tg.GUARD + B * P].reshape(B, P)
    got = gwin[tg.GUARD:-tg.GUARD].cpu().numpy().reshape(B, R, n_in)
    bad = []
    tg._judge(case, 'gwin', got, ref, A, bad)
    assert np.isfinite(got).all(), 'an entry of gwin was not written'
    assert np.array_equal(slabs.view(np.int64), slabs0.view(np.int64)), 'the weight-gradient slabs differ from the plain call'
    assert not bad, (name, bad)


def _conv_grad_cases():
    from test_conv_recog_gpu import GRAD_CASES
    return GRAD_CASES


@pytest.mark.parametrize('shape,seed', _conv_grad_cases(), ids=['-'.join(map(str, s)) + '-seed%d' % sd for s, sd in _conv_grad_cases()])
def test_conv_window_adjoint_against_float64_autograd(shape, seed):
    import test_conv_recog_gpu as tc
    from test_gru_recog_gpu import GUARD, _guarded, _guards_untouched
    fx = tc._fixture(seed, *shape)
    margin = tc._margin(fx)
    print('CONV_RECOG_RECORD gwin shape=%s seed=%d margin=%.1f' % (shape, seed, margin))
    assert margin >= tc.MARGIN, (shape, seed, margin)
    g_truth, g_ref = hc.conv_window_reference(fx)
    # an odd recog_len leaves an odd last conv position, which the pooling drops: the last window row feeds nothing else, its
    # adjoint is exactly zero (asserted on the kernel below); every other row is informative
    dead = [fx['R'] - 1] if fx['R'] % 2 else []
    for t in range(fx['R']):
        assert (np.abs(g_truth[:, t]).max() > 0.0) == (t not in dead), ('the reference window adjoint at row', t)
    l = lib.load()
    B, R, n_in = fx['B'], fx['R'], fx['n_in']
    slabs0, _ = tc._kernel_grads(fx)                         # cbfssm_conv_recog_bwd_f32 on the same inputs
    E = slabs0.shape[1]
    u, y, prm = torch.tensor(fx['u'], device=DEV), torch.tensor(fx['y'], device=DEV), tc._flat_params(fx)
    gx0 = torch.tensor(fx['gx0'], device=DEV)
    gpart, gwin = _guarded((B + 32) * E), _guarded(B * R * n_in)
    rc = l.cbfssm_conv_recog_bwd_in_f32(B, fx['T'], fx['dim_u'], fx['dim_y'], fx['dim_x'], R, ops._ptr(u), ops._ptr(y),
                                        ops._ptr(prm), ops._ptr(gx0), ops._ptr(gpart[GUARD:]), ops._ptr(gwin[GUARD:]),
                                        ops._stream())
    lib.check(rc, 'cbfssm_conv_recog_bwd_in_f32')
    torch.cuda.synchronize()
    assert _guards_untouched(gpart) and _guards_untouched(gwin)
    slabs = gpart[GUARD:GUARD + B * E].cpu().numpy().reshape(B, E)
    got = gwin[GUARD:-GUARD].cpu().numpy().reshape(B, R, n_in)
    scale = np.abs(g_truth).max()
    e_ker, e_ref = np.abs(got - g_truth).max() / scale, np.abs(g_ref - g_truth).max() / scale
    print('CONV_RECOG_RECORD gwin shape=%s seed=%d e_kernel=%.3e e_ref=%.3e err/bound=%.4f'
          % (shape, seed, e_ker, e_ref, e_ker / (4 * e_ref + 2.0 ** -23)))
    assert np.isfinite(got).all(), 'an entry of gwin was not written'
    assert not got[:, dead].any(), 'the row behind the dropped conv position must be exactly zero'
    assert np.array_equal(slabs.view(np.int64), slabs0.view(np.int64)), 'the weight-gradient slabs differ from the plain call'
    assert e_ker <= 4 * e_ref + 2.0 ** -23, (e_ker, e_ref)


# ---- autograd ------------------------------------------------------------------------------------------------------------
def _front(fr, u, y):
    return u * fr['gain'] + fr['bias_u'], y + fr['bias_y']


@pytest.mark.parametrize('name,cond', [('half-rnn', True), ('half-rnn', False), ('prssm-conv', True)])
def test_autograd_trains_a_gain_and_bias_in_front_of_the_model(name, cond):
    """the front end of tests/test_input_grads_gpu.py.  With the conv recogniser the window part dominates the front end's
    gradients and is float32: those are judged by the conv rule (truth: the oracle with the conv evaluated in float64)"""
    from cbfssm.hip.autograd import elbo_loss
    variant, w, cfg, p, u, y, noise = hc.setup(name)
    conv = hc.CASES[name][1] == 'conv'
    rng = np.random.default_rng(5)
    fr = {'gain': 1.0 + 0.2 * rng.standard_normal(w.dim_u), 'bias_u': 0.1 * rng.standard_normal(w.dim_u),
          'bias_y': 0.05 * rng.standard_normal(w.dim_y)}
    loss_ref, gref, _, _, gfr_ref = hc.oracle_run(variant, cfg, p, u, y, noise, cond, front=(fr, _front))
    eng = HipHalfGrad(cfg, DEV, variant=variant)
    params = _params(p, grad=True)
    frt = {k: torch.tensor(v, device=DEV, requires_grad=True) for k, v in fr.items()}
    ut, yt = torch.tensor(np.asarray(u), device=DEV), torch.tensor(np.asarray(y), device=DEV)
    u2, y2 = _front(frt, ut, yt)
    loss = elbo_loss(eng, params, u2, y2, noise, cond)
    loss.backward()
    got = {k: frt[k].grad.cpu().numpy() for k in fr}
    perr = {k: float(np.abs(params[k].grad.cpu().numpy() - gref[k]).max() / (np.abs(gref[k]).max() + 1e-300)) for k in gref}
    print('HALF_IN_RECORD autograd %s cond=%d loss rel %.2e worst parameter gradient %.2e'
          % (name, cond, abs(float(loss.detach()) - loss_ref) / abs(loss_ref), max(perr.values())))
    assert float(loss.detach()) == pytest.approx(loss_ref, rel=1e-6 if conv else 1e-9)
    if conv:
        with hc.float64_conv():
            _, _, _, _, gfr_truth = hc.oracle_run(variant, cfg, p, u, y, noise, cond, front=(fr, _front))
        for k in fr:
            _conv_rule('HALF_IN_RECORD autograd %s %s' % (name, k), got[k], gfr_ref[k], gfr_truth[k])
    else:
        for k in fr:
            within_rule('HALF_IN_RECORD autograd %s cond=%d %s' % (name, cond, k), got[k], gfr_ref[k])
    assert all(e < (1e-3 if conv else 1e-6) for e in perr.values()), perr


@pytest.mark.parametrize('name', ['half-rnn', 'prssm-conv'])
def test_autograd_without_input_grads_is_the_default_call_bit_for_bit(name):
    from cbfssm.hip.autograd import elbo_loss
    variant, w, cfg, p, u, y, noise = hc.setup(name)
    eng = HipHalfGrad(cfg, DEV, variant=variant)
    l0, g0, _ = eng.loss_and_grads(_params(p), u, y, noise)
    assert 'u' not in g0 and 'y' not in g0
    l0, g0 = float(l0), {k: v.clone() for k, v in g0.items()}
    params = _params(p, grad=True)
    ut = torch.tensor(np.asarray(u), device=DEV, requires_grad=True)
    yt = torch.tensor(np.asarray(y), device=DEV)
    loss = elbo_loss(eng, params, ut, yt, noise, True, input_grads=False)
    loss.backward()
    assert float(loss.detach()) == l0 and ut.grad is None
    for k in eng.names:
        assert torch.equal(params[k].grad, g0[k]), k


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refused_cases_raise_the_documented_error():
    from cbfssm.model import CBFSSMHALF, PRSSM
    from cbfssm.model.session import Session
    variant, w, cfg, p, u, y, noise = hc.setup('half-rnn')
    eng32 = HipHalfGrad(cfg, DEV, dtype='float32')
    with pytest.raises(NotImplementedError, match='float64'):
        eng32.loss_and_grads(_params(p), u, y, noise, input_grads=True)
    engd = HipHalfGrad(cfg, DEV, dist=object())
    with pytest.raises(NotImplementedError, match='process group'):
        engd.loss_and_grads(_params(p), u, y, noise, input_grads=True)
    # the model-level fetches of the forward-only variants stay refused
    for cls, extra in ((CBFSSMHALF, {}), (PRSSM, {'recog_model': 'output'})):
        c2 = dict(cfg, batch_size=w.B, shuffle=1, seed=3, **extra)
        model = cls(c2)
        with model.graph.as_default(), Session(DEV) as sess:
            model.load_ds(sess, np.asarray(u), np.asarray(y))
            with pytest.raises(NotImplementedError, match='no input gradients'):
                sess.run(model.grad_sample_in, {model.condition: True})
