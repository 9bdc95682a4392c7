"""A reused engine on poisoned workspaces gives the bits of a fresh engine.

Every device buffer of ops.HipElbo, train.HipElboGrad / HipTrainStep and train_half.HipHalfGrad / HipHalfTrainStep is
allocated with torch.zeros and kept for the life of the engine, and every parity test starts from a fresh engine: what a
kernel reads without having written it is an exact zero there.  Production uses one engine for thousands of steps on
different data, with a ragged last batch and a test pass viewing into the same tile pool, `condition` flipping on one
workspace, graphs replaying on fixed addresses, and NaN everywhere after one diverged step.

One case, target call X:
    1. fresh engine, run X, clone the public outputs: loss, the six terms (`info` among them), x, pred_mean, pred_var,
       int_mean, int_var and every gradient (u / y where requested)
    2. another fresh engine, a dirtying sequence D on other data
    3. workspace_poison.poison(engine, word): the whole storage of every float tensor the engine reaches that is not
       optimiser state
    4. run X: every output torch.equal to step 1, for both words (NaN, and a value finite and huge as float64 and float32)
Bit equality is the rule tests/test_workspace_gpu.py already holds for a small batch behind a large one: fixed-order
reductions, no atomics.  Both sides run the same code path: cfg['gp_form'] is pinned (CBFSSM_GP_FORM for the forward-only
engines, which take the form from the environment), the tile budget is the default, the environment switches are the same.

Dirtying sequences: s1 same shape, other inputs, noise and parameters; s2 a (B + 2, T + 3) call first (tile-pool and stash
views into a larger buffer); s3 the same shape with `condition` flipped; s4 forward() (the eval workspace) and
loss_and_grads(input_grads=True) before a plain X, and plain calls before an X with input_grads=True.  Once the other
order of s2: X's shape, then the larger one, so that X runs on the retired buffers of a grown pool.

Rows by name from tests/tile_grid.py (padding rows, a ragged last chain group; one per tile height), so the fresh result
is the one tests/test_tile_grid_gpu.py holds against the oracle.  Before comparing, every case asserts that the poison
report names the buffers its engine's constructors allocate: a walker that finds nothing fails here.  Nothing skips.
Outcome, poisoned bytes and timings: profiles/workspace_poison/README.md."""
import dataclasses

import numpy as np
import pytest
import torch

from cbfssm import synthetic as syn
from cbfssm.hip import ops, train
from cbfssm.hip.train_half import HipHalfGrad, HipHalfTrainStep, half_param_names
import tile_grid as tg
import workspace_poison as wp

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

ROWS = ['nb1_mid_dk6', 'nb2_mid_dk2', 'nb4_mid_dk4', 'nb7_kt3_dk2', 'nb7_kt0_dk2', 'nb10_first_dk2', 'nb13_mid_dk2',
        'nb16_mid_dk4', 'nb20_first_dk2']
STASH_ROWS = [n for n in ROWS if tg.CASE_KW[n]['M'] > 112]
NON_STASH, STASH = 'nb7_kt3_dk2', 'nb13_mid_dk2'          # the rows that take every dirtying sequence
CLASS_ROWS = ['nb4_mid_dk4', 'nb7_kt3_dk2', 'nb13_mid_dk2']            # one per height class: <= 4, 7, >= 10 row blocks
F32_ROWS = ['nb7_kt3_dk2', 'nb13_mid_dk2', 'nb16_mid_dk4']             # <= 7, 10-13, >= 16 row blocks (two passes above M = 208)
assert all(n in tg.CASE_KW for n in ROWS)

WS_OUT = ('x', 'pred_mean', 'pred_var', 'int_mean', 'int_var')
_SHOWN = set()


@pytest.fixture(autouse=True)
def _pinned_form(monkeypatch):
    """engines that take the GP form from the environment (HipHalfGrad in float64) run the dense form on both sides: the
    automatic form lags two read-backs behind and would depend on the dirtying calls"""
    monkeypatch.setenv('CBFSSM_GP_FORM', 'dense')
    for k in ('CBFSSM_NO_SAVE_K', 'CBFSSM_SPLIT_MAIN', 'CBFSSM_F32_NO_TILES', 'CBFSSM_A2S_MAX_GB', 'CBFSSM_NO_SPLIT',
              'CBFSSM_TORCH_TAIL', 'CBFSSM_TORCH_GRU', 'CBFSSM_TORCH_CONV', 'CBFSSM_HIP_GRAPH'):
        monkeypatch.delenv(k, raising=False)


# ---- data -------------------------------------------------------------------------------------------------------------
def _dev(p):
    return {k: torch.tensor(v, device=DEV) for k, v in p.items()}


def _other(w, p, dB=0, dT=0, seed=11, half=False):
    """other inputs, noise and parameters at the shape (B + dB, T + dT)"""
    w2 = dataclasses.replace(w, B=w.B + dB, T=w.T + dT)
    u, y = syn.make_inputs(w2, seed=seed)
    noise = syn.make_noise(w2, seed=seed + 1)
    if half:
        noise = {'eps_f': noise['eps_f']}
    rng = np.random.default_rng(seed + 2)
    p2 = {k: np.ascontiguousarray(v + 0.05 * rng.standard_normal(np.shape(v))) for k, v in p.items()}
    return _dev(p2), u, y, noise


# ---- the protocol --------------------------------------------------------------------------------------------------------
def _same(ref, got, what):
    assert set(ref) == set(got), what
    for k in ref:
        assert torch.equal(ref[k], got[k]), '%s: %s differs from the fresh engine (%d of %d elements, fresh |max| %.3e, got %s)' % (
            what, k, int((ref[k] != got[k]).sum()), ref[k].numel(), float(ref[k].abs().max()) if ref[k].numel() else 0.0,
            got[k].reshape(-1)[:4].tolist())


def _guard(rep, expect, what):
    """the poison report names every buffer the constructors allocate for this engine kind and mode"""
    paths = rep.poisoned_paths()
    missing = [e for e in expect if not any(p.endswith(e) for p in paths)]
    assert not missing, '%s: the walk did not reach %s; it reached %s' % (what, missing, sorted(paths))
    assert not rep.kept() or all(g.kept_by for g in rep.kept())
    kind = what.split(' ')[0]
    if kind not in _SHOWN:                                    # (pytest -s: one full report per engine kind for the write-up)
        _SHOWN.add(kind)
        print('\n--- poison report, %s: %d storages, %d bytes' % (what, len(rep.poisoned()), rep.poisoned_bytes()))
        print('\n'.join(rep.lines()))


def _reuse(what, make, target, dirty, expect):
    ref = target(make())
    assert float(ref['info']) == 0.0, what
    for k, v in ref.items():
        assert torch.isfinite(v).all(), (what, k)
    for wname, word in wp.WORDS.items():
        eng = make()
        dirty(eng)
        rep = wp.poison(eng, word)
        _guard(rep, expect(eng), what)
        _same(ref, target(eng), '%s, %s after %d poisoned bytes' % (what, wname, rep.poisoned_bytes()))


# ---- what the constructors allocate (ops.GPPack, ops.ElboWorkspace, train.HipElboGrad.__init__ / _workspace / _input_buffers /
# _adjoint / _adjoint_stash, train.StashContract, train_half.HipHalfGrad._workspace / _input_buffers / _adjoint / _param_grads,
# train_half.KernelRecogniser.forward)
ELBO_WS = ['.y2', '.x', '.ent_part', '.kl_part', '.ll_part', '.pred_mean', '.pred_var', '.int_mean', '.int_var', '.out']


def _expect_elbo(eng):
    return ['pack_f.buf', 'pack_b.buf'] + ELBO_WS + (['pack_f.buf32', 'pack_b.buf32'] if eng.f32 else [])


def _expect_grad(eng, ig=False, evalws=False, tiles=True):
    e = ['pack_f.buf', 'pack_b.buf', '.red', '.cflat', '.gflat', '.tail_work'] + ELBO_WS
    e += ['.h_all', '.fmv_b', '.fmv_f', '.gy2', '.gpart_f', '.gpart_b']
    if tiles:
        e += ['tile_pool.bufs[0]', 'tile_pool.bufs[1]', '.a2s_f', '.a2s_b']
    if eng.f32:
        e += ['pack_f.buf32', 'pack_b.buf32'] + (['._tmp32'] if eng.repack32 else [])
    elif eng.stash:
        e += ['.gx_carry'] + ['._stash_buf[%d]' % i for i in range(4)]
        e += ['._contract[0].work', '._contract[1].work', '._contract[0].image', '._contract[1].image']
    if ig:
        e += ['.in_bufs[0]', '.in_bufs[1]', '.in_bufs[2]', '.grad_u', '.grad_y']
    if evalws:
        e += ["_ws[('eval', %d, %d)].x" % k[1:] for k in eng._ws if k[0] == 'eval']
        assert any(k[0] == 'eval' for k in eng._ws)
    return e


def _expect_half(eng, ig=False):
    e = ['pack_f.buf', '.x', '.fmv_f', '.a2s_f', 'tile_pool.bufs[0]', '.kl_part', '.ll_part', '.pred_mean', '.pred_var',
         '.int_mean', '.int_var', '.out', '.gx0', '.gx_carry', '.gpart_f', '.red', '.tail_work']
    if eng.variant == 'prssm':
        e += ['pack_kl.buf']
    if eng.rnn:
        e += ['.x0', '.act', '.gpart']
    if eng.conv:
        e += ['.x0', '.gpart']
    if eng.f32:
        e += ['pack_f.buf32'] + (['._tmp32'] if eng.repack32 else [])
    elif eng.stash:
        e += ['._stash_buf[0]', '._stash_buf[1]', '._contract.work', '._contract.image']
    if ig:
        e += ['.in_bufs[0]', '.in_bufs[2]', '.gwin', '.grad_u', '.grad_y']
    return e


# ---- HipElbo.run ---------------------------------------------------------------------------------------------------------------
def _elbo_out(ws):
    torch.cuda.synchronize()
    out = {k: getattr(ws, k).clone() for k in WS_OUT}
    for i, k in enumerate(('loglik', 'kl_x', 'entropy', 'kl_z_f', 'kl_z_b', 'elbo', 'loss', 'info')):
        out[k] = ws.out[i].clone()
    return out


def _elbo_case(name, form, dtype, seq, condition=True):
    w, cfg, p, u, y, noise = tg.setup(tg.CASE_KW[name])
    cfg['gp_form'] = form

    def make():
        return ops.HipElbo(cfg, DEV, dtype=dtype)

    def target(eng):
        eng.prepare(p)
        return _elbo_out(eng.run(u, y, noise, condition=condition))

    def dirty(eng):
        dB, dT = (2, 3) if seq == 's2' else (0, 0)
        p2, u2, y2, n2 = _other(w, p, dB, dT)
        eng.prepare(p2)
        eng.run(u2, y2, n2, condition=condition)
        if seq == 's2':
            p3, u3, y3, n3 = _other(w, p, seed=21)
            eng.prepare(p3)
            eng.run(u3, y3, n3, condition=condition)          # the target's workspace exists and is dirty too
        if seq == 's3':
            eng.run(u2, y2, n2, condition=not condition)

    _reuse('HipElbo %s %s %s %s' % (name, form, dtype, seq), make, target, dirty, _expect_elbo)


@pytest.mark.parametrize('form', ['dense', 'tri'])
@pytest.mark.parametrize('name', ROWS)
def test_elbo_run_f64(name, form):
    _elbo_case(name, form, 'float64', 's1')


@pytest.mark.parametrize('seq', ['s2', 's3'])
@pytest.mark.parametrize('name', [NON_STASH, STASH])
def test_elbo_run_f64_after_a_larger_shape_and_a_flipped_condition(name, seq):
    _elbo_case(name, 'dense', 'float64', seq)


@pytest.mark.parametrize('name', F32_ROWS)
def test_elbo_run_f32(name):
    _elbo_case(name, 'tri', 'float32', 's1')


def test_elbo_run_bf16_operands():
    _elbo_case(NON_STASH, 'dense', 'bfloat16', 's1')


# ---- HipElboGrad.loss_and_grads ---------------------------------------------------------------------------------------------------
def _grad_out(eng, res):
    loss, grads, terms = res
    torch.cuda.synchronize()
    out = {'loss': loss.clone()}
    out.update({k: v.clone() for k, v in terms.items()})
    assert set(terms) == {'loglik', 'kl_x', 'entropy', 'kl_z_f', 'kl_z_b', 'info'}
    out.update({'grad.' + k: v.clone() for k, v in grads.items()})
    out.update({k: getattr(eng.last_ws, k).clone() for k in WS_OUT})
    return out


def _grad_case(name, form='dense', dtype='float64', seq='s1', ig=False, cfg_extra=None, kw_extra=None, tiles=True, check=None, before=None):
    w, cfg, p, u, y, noise = tg.setup(dict(tg.CASE_KW[name], **(kw_extra or {})))
    cfg['gp_form'] = form
    cfg.update(cfg_extra or {})
    params = _dev(p)

    def make():
        return train.HipElboGrad(cfg, DEV, dtype=dtype)

    def target(eng):
        if before:
            before()
        out = _grad_out(eng, eng.loss_and_grads(params, u, y, noise, condition=True, input_grads=ig))
        assert set(k for k in out if k.startswith('grad.')) == {'grad.' + k for k in train.PARAM_NAMES + (('u', 'y') if ig else ())}
        assert eng.pack_f.gp_form() == form and eng.pack_b.gp_form() == form
        if check:
            check(eng)
        return out

    def dirty(eng):
        dB, dT = (2, 3) if seq == 's2' else (0, 0)
        p2, u2, y2, n2 = _other(w, p, dB, dT)
        if seq == 'grow':
            # the target's shape first, then a larger one: the pool grows and retires the buffers the first workspace views
            p3, u3, y3, n3 = _other(w, p, 2, 3, seed=21)
            eng.loss_and_grads(p2, u2, y2, n2, condition=True)
            with pytest.warns(UserWarning, match='pool grows'):
                eng.loss_and_grads(p3, u3, y3, n3, condition=True)
            assert len(eng.tile_pool.retired) == 1
            return
        if seq == 's4':
            # the eval workspace, then the other kind of gradient call than X
            eng.forward(p2, u2, y2, n2, condition=True)
            eng.loss_and_grads(p2, u2, y2, n2, condition=True, input_grads=not ig)
            if ig:
                return
        eng.loss_and_grads(p2, u2, y2, n2, condition=True, input_grads=ig)
        if seq == 's2':
            p3, u3, y3, n3 = _other(w, p, seed=21)
            eng.loss_and_grads(p3, u3, y3, n3, condition=True, input_grads=ig)
        if seq == 's3':
            eng.loss_and_grads(p2, u2, y2, n2, condition=False, input_grads=ig)

    def expect(eng):
        # (s4 before an X with input gradients ran plain calls only: the input buffers do not exist yet)
        e = _expect_grad(eng, ig=ig and seq != 's4' or (seq == 's4' and not ig), evalws=seq == 's4', tiles=tiles)
        return e + (['tile_pool.retired[0][0]', 'tile_pool.retired[0][1]'] if seq == 'grow' else [])

    _reuse('HipElboGrad %s %s %s %s ig=%d %s' % (name, form, dtype, seq, ig, sorted((cfg_extra or {}).items())),
           make, target, dirty, expect)


@pytest.mark.parametrize('name', ROWS)
def test_grads_f64_dense(name):
    _grad_case(name)


@pytest.mark.parametrize('name', CLASS_ROWS)
def test_grads_f64_tri(name):
    _grad_case(name, form='tri')


@pytest.mark.parametrize('name', CLASS_ROWS)
def test_grads_f64_with_input_gradients(name):
    _grad_case(name, ig=True)


@pytest.mark.parametrize('seq,ig', [('s2', False), ('s3', False), ('s4', False), ('s4', True)])
@pytest.mark.parametrize('name', [NON_STASH, STASH])
def test_grads_f64_after_other_shapes_conditions_and_calls(name, seq, ig):
    _grad_case(name, seq=seq, ig=ig)


def test_grads_f64_on_the_retired_buffers_of_a_grown_pool():
    """the workspace of X keeps its views into the pool's first buffers after a larger shape made the pool grow"""
    _grad_case(NON_STASH, seq='grow')


def test_grads_f64_recomputed_kernel_tiles(monkeypatch):
    """CBFSSM_NO_SAVE_K=1: the records hold the A2 tile only (M <= 112)"""
    monkeypatch.setenv('CBFSSM_NO_SAVE_K', '1')
    _grad_case(NON_STASH)


def test_grads_f64_two_streams(monkeypatch):
    """CBFSSM_SPLIT_MAIN=1: the chain groups in two pieces on two streams (21 chains: one group each)"""
    monkeypatch.setenv('CBFSSM_SPLIT_MAIN', '1')
    seen = []
    _grad_case(NON_STASH, check=lambda eng: seen.append(getattr(eng, '_s1', None) is not None))
    assert len(seen) == 3 and all(seen)                        # the side stream exists: the split ran


@pytest.mark.parametrize('name', STASH_ROWS)
def test_grads_f64_stash_in_time_chunks(name, monkeypatch):
    """adjoint_stash_gib = 1e-9 holds one step / one segment per launch: T - 1 launches of the forward-pass adjoint and one
    launch per segment of the backward runs (HipElboGrad._adjoint_stash's arithmetic, restated), at least three per
    direction.  The rows with T = 6 have two segments: they run at T = 7 here."""
    kw = tg.CASE_KW[name]
    T, R, N = max(kw['T'], 7), kw['recog_len'], kw['B'] * kw['S']
    counts = {'f': 0, 'b': 0}
    f0, b0 = ops.TimeLoops.forward_pass_bwd, ops.TimeLoops.backward_pass_bwd

    def fcount(self, q, st, chunk=None):
        counts['f'] += 1
        return f0(self, q, st, chunk)

    def bcount(self, q, st, chunk=None):
        counts['b'] += 1
        return b0(self, q, st, chunk)
    monkeypatch.setattr(ops.TimeLoops, 'forward_pass_bwd', fcount)
    monkeypatch.setattr(ops.TimeLoops, 'backward_pass_bwd', bcount)

    def check(eng):
        groups, Mp, P = (N + 15) // 16, eng.pack_f.layout.Mp, 2 * R
        per_f = max(1, max(groups * 16, eng.stash_bytes // (4 * Mp * 8)) // (groups * 16))
        per_b = max(1, max(groups * 16 * 2 * P, eng.stash_bytes // (4 * Mp * 8)) // (groups * 2 * P * 16))
        nseg = (T - 1 + R) // (2 * R) + 1
        assert per_f == 1 and per_b == 1
        assert T - 1 >= 3 and nseg >= 3
        assert (counts['f'], counts['b']) == (T - 1, nseg), counts
    _grad_case(name, cfg_extra={'adjoint_stash_gib': 1e-9}, kw_extra={'T': T}, check=check, before=lambda: counts.update(f=0, b=0))


@pytest.mark.parametrize('tiles', [True, False])
@pytest.mark.parametrize('name', F32_ROWS)
def test_grads_f32_tri(name, tiles, monkeypatch):
    """the float32 adjoint with its kept [A2 | K] records (float32 words in the float64 tile pool) and recomputing
    (CBFSSM_F32_NO_TILES=1); nb16_mid_dk4 is the two-pass case (M > 208)"""
    if not tiles:
        monkeypatch.setenv('CBFSSM_F32_NO_TILES', '1')
    _grad_case(name, form='tri', dtype='float32', tiles=tiles)


# ---- HipHalfGrad.loss_and_grads ------------------------------------------------------------------------------------------------------
SMALL_RNN = dict(T=11, B=3, S=4, M=12, recog_len=3)
HALF_ROWS = {
    # the small cases of tests/test_half_gpu.py and tests/test_prssm_gpu.py
    'half-rnn': ('half', 'rnn', SMALL_RNN, {}),
    'half-output': ('half', 'output', dict(T=9, B=2, S=7, M=20, recog_len=4, k_factor=20.), {}),
    'half-rnn-stash': ('half', 'rnn', dict(T=9, B=2, S=9, M=130, dim_x=6, dim_u=2, dim_y=2, recog_len=2), {'adjoint_stash_gib': 3e-4}),
    'prssm-rnn': ('prssm', 'rnn', SMALL_RNN, {}),
    'prssm-conv': ('prssm', 'conv', dict(T=20, B=2, S=5, M=33, recog_len=16, dim_x=4, dim_u=1, dim_y=1), {}),
    # rows of tg.HALF_CASES at seven, ten and twenty row blocks
    'half-nb7': ('half', 'rnn', tg.CASE_KW['nb7_kt1_dk2'], {}),
    'half-nb10': ('half', 'rnn', tg.CASE_KW['nb10_fill_dk4'], {}),
    'half-nb20': ('half', 'rnn', tg.CASE_KW['nb20_mid_dk6'], {}),
}
assert {'nb7_kt1_dk2', 'nb10_fill_dk4', 'nb20_mid_dk6'} <= set(tg.HALF_CASES)


def _half_case(key, dtype='float64', seq='s1', ig=False):
    from test_oracle import _half_setup, _prssm_setup
    variant, recog, kw, extra = HALF_ROWS[key]
    w, cfg, p, u, y, noise = (_prssm_setup if variant == 'prssm' else _half_setup)(recog, **kw)
    cfg.update(extra)
    if dtype == 'float32':
        cfg['gp_form'] = 'tri'
    params = _dev(p)
    names = set(half_param_names(cfg, variant))

    def make():
        return HipHalfGrad(cfg, DEV, variant=variant, dtype=dtype)

    def target(eng):
        out = _grad_out(eng, eng.loss_and_grads(params, u, y, noise, True, input_grads=ig))
        assert set(k for k in out if k.startswith('grad.')) == {'grad.' + k for k in names | ({'u', 'y'} if ig else set())}
        return out

    def dirty(eng):
        dB, dT = (2, 3) if seq == 's2' else (0, 0)
        p2, u2, y2, n2 = _other(w, p, dB, dT, half=True)
        if seq == 's4':
            eng.forward(p2, u2, y2, n2, True)
            eng.loss_and_grads(p2, u2, y2, n2, True, input_grads=not ig)
            if ig:
                return
        eng.loss_and_grads(p2, u2, y2, n2, True, input_grads=ig)
        if seq == 's2':
            p3, u3, y3, n3 = _other(w, p, seed=21, half=True)
            eng.loss_and_grads(p3, u3, y3, n3, True, input_grads=ig)
        if seq == 's3':
            eng.loss_and_grads(p2, u2, y2, n2, False, input_grads=ig)

    def expect(eng):
        return _expect_half(eng, ig=(ig and seq != 's4') or (seq == 's4' and not ig))

    _reuse('HipHalfGrad %s %s %s ig=%d' % (key, dtype, seq, ig), make, target, dirty, expect)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('key', ['half-rnn', 'half-output', 'prssm-rnn', 'prssm-conv'])
def test_half_grads(key, dtype):
    _half_case(key, dtype)


@pytest.mark.parametrize('key', ['half-rnn-stash', 'half-nb7', 'half-nb10', 'half-nb20'])
def test_half_grads_at_the_tall_tiles(key):
    _half_case(key)


@pytest.mark.parametrize('key', ['half-rnn', 'half-output', 'prssm-conv'])
def test_half_grads_with_input_gradients(key):
    _half_case(key, ig=True)


@pytest.mark.parametrize('seq,ig', [('s2', False), ('s3', False), ('s4', False), ('s4', True)])
def test_half_grads_after_other_shapes_conditions_and_calls(seq, ig):
    _half_case('half-rnn', seq=seq, ig=ig)


# ---- train steps: five steps with batch sizes 3, 3, 2, 3, 3 on distinct data, untouched and with poison before every step ----------
BATCHES = (3, 3, 2, 3, 3)


def _five_steps(what, make, batch, expect):
    res = {}
    for mode in ('untouched', 'nan', 'huge'):
        step = make()
        losses = []
        for i, B in enumerate(BATCHES):
            if mode != 'untouched':
                rep = wp.poison(step, wp.WORDS[mode])
                if i:                                          # (before the first step no workspace exists yet)
                    _guard(rep, expect(step.engine), what)
                    assert any('TFAdam.flat' in g.kept_by for g in rep.kept())
                    assert any(p.endswith('.loss') or "['loss']" in p for p in rep.poisoned_paths()) == bool(step.use_graph)
            losses.append(step.step(*batch(B, i)).clone())
        torch.cuda.synchronize()
        assert step.opt.t == len(BATCHES) and float(step.opt.t_dev) == len(BATCHES)
        res[mode] = (torch.stack(losses), step.opt.flat.clone(), step.opt.m.clone(), step.opt.v.clone())
        assert all(torch.isfinite(t).all() for t in res[mode]), (what, mode)
    for mode in ('nan', 'huge'):
        for k, (a, b) in enumerate(zip(res['untouched'], res[mode])):
            assert torch.equal(a, b), '%s, %s: %s differs from the untouched run' % (what, mode, ('losses', 'parameters', 'm', 'v')[k])


@pytest.mark.parametrize('name,dtype', [('m20', 'float64'), (NON_STASH, 'float64'), ('m20', 'float32')])
def test_train_step_with_graph(name, dtype):
    kw = dict(M=20, T=9, B=3, S=5) if name == 'm20' else tg.CASE_KW[name]
    w = syn.tiny(**kw)
    assert w.B == 3
    cfg = w.model_config()
    cfg['gp_form'] = 'tri' if dtype == 'float32' else 'dense'
    p = syn.perturb_params(syn.make_params(w, seed=tg.PARAM_SEED), scale=tg.PERTURB_SCALE)

    def make():
        st = train.HipTrainStep(cfg, _dev(p), DEV, graph=True, dtype=dtype)
        assert st.use_graph
        return st

    def batch(B, i):
        wb = dataclasses.replace(w, B=B)
        return syn.make_inputs(wb, seed=30 + i) + (syn.make_noise(wb, seed=50 + i),)

    _five_steps('HipTrainStep %s %s' % (name, dtype), make, batch,
                lambda eng: _expect_grad(eng, tiles=True))


def test_half_train_step_with_graph():
    from test_oracle import _half_setup
    w, cfg, p, u, y, noise = _half_setup('rnn', **SMALL_RNN)
    assert w.B == 3

    def make():
        from cbfssm.hip.train import TFAdam
        eng = HipHalfGrad(cfg, DEV)
        st = HipHalfTrainStep(eng, TFAdam({k: torch.tensor(p[k], device=DEV) for k in half_param_names(cfg)}, 0.01), graph=True)
        assert st.use_graph
        return st

    def batch(B, i):
        wb = dataclasses.replace(w, B=B)
        return syn.make_inputs(wb, seed=30 + i) + ({'eps_f': syn.make_noise(wb, seed=50 + i)['eps_f']},)

    _five_steps('HipHalfTrainStep half-rnn', make, batch, _expect_half)
