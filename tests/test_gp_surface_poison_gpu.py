"""Every entry point of the GPModel surface on poisoned per-call allocations, through the shipped Python path
(tests/gp_surface_poison.py): cbfssm.model.gp_tf.GPModel where it has the method, cbfssm.hip.autograd / cbfssm.hip.ops /
the functions of gp_tf otherwise.

Per case the call runs three times -- every torch.empty / torch.empty_like of the glue filled with the word 0, with the NaN
word and with the huge word of tests/workspace_poison.py, the model's own pack poisoned with the same word before every call
and again before every backward -- and every output and every gradient must be bitwise the same in the three runs, NaN in
the same places (`_same` of tests/test_gp_eks_gpu.py).  A kernel that reads a padding row, a lane of a ragged last group, a
scratch slab or an unconditioned step's record that this call did not write cannot do that.  The word-0 run is also held to
the CPU reference of the case by the rule of the entry point's own GPU file (the helpers are imported, not copied).

Before any comparison the coverage guard checks from the log that the call poisoned what the glue allocates for that entry
point and mode: TABLES names, per entry point, the functions of the three product files whose allocation lines must have
been hit (a stash-only buffer such as `image` only at the stash heights, `vsave` only under grad, ...: _expected), and no
allocation of a product file may come from a line outside them.  tests/test_gp_surface_poison_cpu.py holds the other half:
every allocation line of the three files belongs to a function some table names, or to EXEMPT.

Shapes: the `*_first_*` row of each of the eight tile heights of gp_tile_grid.ROWS (one data row in front of whole blocks of
padding; all three input widths) and nb7_kt3_dk6, the C3 shape, through the existing case builders -- N = 21 chains or 37
points (a ragged last group), T = 5; the two-triangular form with the pack forced at TRI_ROWS; one wide case per adjoint
that reduces slabs (at least 128 workgroups: cbfssm_reduce_partials_f64 in its two-stage form on a poisoned scratch); the
flagged-failure cases of the eks, adf / ads and moment_match files."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

import gp_adf_cases as ac
import gp_autograd_cases as gc
import gp_ekf_cases as ec
import gp_ekf_grad_cases as egc
import gp_eks_cases as sc
import gp_filter_cases as fc
import gp_filter_fullq_grid as fg
import gp_fullq_cases as fq
import gp_linearize_cases as lc
import gp_moment_match_cases as mc
import gp_rollout_cases as rc
import gp_surface_poison as gsp
import gp_tile_grid as gg
import rigid_filter_cases as rgc
from gp_autograd_cases import PARAMS, within_rule
from test_gp_eks_gpu import _same

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

FIRST_ROWS = ['nb1_first_dk2', 'nb2_first_dk4', 'nb4_first_dk6', 'nb7_first_dk4', 'nb10_first_dk2', 'nb13_first_dk4',
              'nb16_first_dk6', 'nb20_first_dk2']
C3_ROW = 'nb7_kt3_dk6'
TRI_ROWS = ['nb7_kt3_dk6', 'nb13_first_dk4']
# (row, forced form or None for the automatic switch)
SHAPES = [(r, None) for r in FIRST_ROWS + [C3_ROW]] + [(r, 'tri') for r in TRI_ROWS]
SHAPE_IDS = ['%s-%s' % (r, f or 'auto') for r, f in SHAPES]
WIDE_ROW = 'nb1_first_dk2'                       # the smallest tile height
WIDE_N, WIDE_T = 16 * 128 + 5, 3
WIDE_RIGID = (64 * 128 + 5, 3)                   # (N, S): the rigid filter runs 64 chains per workgroup

A, O, G = 'autograd.py:', 'ops.py:', 'gp_tf.py:'
# entry point -> the functions whose allocation lines the call must hit (file:function as gp_surface_poison.sites_of takes it)
TABLES = {
    'predict_grad': [O + 'GPPack.predict', A + '_GpPredict.backward', A + '_gp_tail'],
    'conditional_diag_grad': [O + 'GPPack.predict', A + '_GpConditionalDiag.backward', A + '_gp_tail'],
    'fullq_eval': [A + '_fq_qpack', A + '_fq_forward', A + '_fq_kl'],
    'fullq_grad': [A + '_fq_qpack', A + '_fq_forward', A + '_fq_kl', A + '_GpPredictFullq.backward', A + '_fq_tail',
                   A + '_GpPriorKlFullq.backward'],
    'conditional_fullq_eval': [G + 'conditional'],
    'rollout_eval': [A + '_rollout_forward'],
    'rollout_grad': [A + '_rollout_forward', A + '_GpRollout.backward', A + '_gp_tail'],
    'filter_eval': [A + '_filter_forward'],
    'filter_grad': [A + '_filter_forward', A + '_GpFilter.backward', A + '_gp_tail'],
    'linearize': [A + 'gp_linearize_eval'],
    'transition_jacobians': [A + 'gp_linearize_eval'],
    'moment_match': [A + 'gp_moment_match_eval'],
    'transition_moments': [A + 'gp_moment_match_eval'],
    'ekf_eval': [A + 'gp_ekf_eval'],
    'ekf_grad': [A + '_GpEkf.forward', A + '_GpEkf.backward', A + '_gp_tail'],
    'eks': [A + 'gp_eks_eval'],
    'adf': [A + 'gp_adf_eval', A + '_adf_work'],
    'ads': [A + 'gp_ads_eval', A + '_adf_work'],
    'rigid_filter': [A + '_rigid_forward', A + '_RigidFilter.backward'],
    'rigid_filter_eval': [A + '_rigid_forward'],
    'pack_predict': [O + 'GPPack.predict'],
    'pack_predict_f32': [O + 'GPPack.predict_f32'],
    'rbf_k': [G + 'RBF.K'],
    'cast_cholesky': [G + 'cast_cholesky'],
    'kmm_chol': [O + 'kmm_chol'],
}
# allocation sites no case of this file reaches, and why
EXEMPT = {O + 'NoisePipeline.next': 'the pre-drawn noise of the engines: tests/test_engine_reuse_gpu.py (KEEP of workspace_poison)'}
# `work` of these adjoints exists at the stash heights only (the *_work_elems query returns 0 below them)
STASH_WORK = {'_GpPredict.backward', '_GpPredictFullq.backward', '_GpConditionalDiag.backward', '_GpRollout.backward',
              '_GpFilter.backward'}
# allocations through a `new = lambda ...` of the glue share one line: their number per call
LAMBDA_COUNTS = {'gp_eks_eval': lambda f: 12 + f['lag_one'], 'gp_ads_eval': lambda f: 11 + f['lag_one'],
                 'gp_adf_eval': lambda f: 7, '_GpEkf.forward': lambda f: 8}


def _dev(a):
    return None if a is None else torch.tensor(np.asarray(a), dtype=torch.float64, device=DEV)


def _row(name):
    return gg.ROW_BY_NAME[name]


def _flags(M, D, Do, **kw):
    from cbfssm.hip import lib
    f = dict(stash=bool(lib.pack_layout(M, D, Do).rev_stash), grad=False, has_a=D > Do, variance=True, cross=True,
             lag_one=False, has_P0=True)
    f.update(kw)
    return f


def _expected(site, f):
    """does this allocation line run in the mode the flags describe"""
    if site.name == 'image':
        return f['stash']
    if site.name == 'work' and site.func in STASH_WORK:
        return f['stash']
    if site.name in ('vsave', 'msave'):
        return f['grad']
    if site.name == 'ga':
        return f['has_a']
    if site.name == 'dvar':
        return f['variance']
    if site.name == 'xcov':
        return f['cross']
    if site.name == 'gP0':
        return f['has_P0']
    return True


def _guard(entry, log, flags):
    """the coverage guard: from the log, the call poisoned every allocation the glue makes for this entry point and mode,
    and made none in a product file that TABLES does not expect"""
    sites = gsp.sites_of(*TABLES[entry])
    hit = collections.Counter((a.file, a.line) for a in log.product())
    lines = {(s.file, s.line) for s in sites}
    stray = sorted(set(hit) - lines)
    assert not stray, '%s: allocations outside the table: %s' % (entry, [a for a in log.product() if (a.file, a.line) in stray])
    for s in sites:
        want, got = _expected(s, flags), hit[(s.file, s.line)] > 0
        assert want == got, '%s: %s:%d %s.%s was %s' % (entry, s.file, s.line, s.func, s.name,
                                                         'not poisoned' if want else 'allocated in a mode that should not')
        if s.name == 'new' and s.func in LAMBDA_COUNTS:
            assert hit[(s.file, s.line)] == LAMBDA_COUNTS[s.func](flags), (entry, s.func, hit[(s.file, s.line)])
    for a in log.product():
        assert a.nbytes > 0, (entry, a)


def _three(entry, call, flags, tag):
    """the call on word 0, NaN and huge; the guard on each log; then bitwise equality with the baseline.  Returns the
    baseline's results."""
    outs, logs = {}, {}
    for name in gsp.ORDER:
        with gsp.poisoned_allocations(gsp.WORDS[name]) as log:
            outs[name] = call(gsp.WORDS[name])
        torch.cuda.synchronize()
        logs[name] = log
    for name in gsp.ORDER:
        _guard(entry, logs[name], flags)
    assert [(a.file, a.line, a.shape) for a in logs['nan'].product()] == [(a.file, a.line, a.shape) for a in logs['zero'].product()]
    print('%s %s: %d allocations, %d bytes poisoned per call' % (entry, tag, len(logs['nan'].product()),
                                                                 logs['nan'].product().nbytes()))
    base = outs['zero']
    for name in gsp.ORDER[1:]:
        assert set(outs[name]) == set(base)
        for k, v in base.items():
            assert _same(v, outs[name][k]), '%s %s: %s differs from the word-0 run under the %s word' % (entry, tag, k, name)
    return base


def _gp(p, M, D, Do, grad=(), form=None, q_full=False):
    """a gp_tf.GPModel carrying the case's parameters as leaves (the `_model` of the entry points' own GPU files); `form`:
    the pack forced to 'dense' / 'tri' as those files force it (ops.GPPack(form_mode=...)), still through the model"""
    from cbfssm.hip import ops
    from cbfssm.model import gp_tf
    gp = gp_tf.GPModel(in_dim=D, out_dim=Do, num_points=M, gp_var=0.4, gp_len=1.0, zeta_mean=0.1, zeta_pos=1.0, zeta_var=0.01,
                       seed=0, device=DEV, q_full=q_full)
    gp.zeta_pos, gp.zeta_mean = _dev(p['zeta_pos']), _dev(p['zeta_mean'])
    if q_full:
        gp.zeta_sqrt = _dev(p['zeta_sqrt'])
    else:
        gp.zeta_var_unc = _dev(p['zeta_var_unc'])
    gp.kern.variance_unc, gp.kern.lengthscales_unc = _dev(p['variance_unc']), _dev(p['lengthscales_unc'])
    if form is not None:
        gp._pack = ops.GPPack(M, D, Do, torch.device(DEV), form_mode=form)
    names = fq.PARAMS if q_full else PARAMS
    leaves = dict(zip(names, gp.parameters()))
    for k in grad:
        leaves[k].requires_grad_()
    return gp, leaves


def _np(t):
    return t.detach().cpu().numpy()


def _values(out, ref, atol):
    np.testing.assert_allclose(_np(out['fmean']), ref['fmean'], rtol=1e-8, atol=atol)
    np.testing.assert_allclose(_np(out['fvar']), ref['fvar'], rtol=1e-8, atol=atol)


# ---- predict + prior_kl under grad; conditional() with a diagonal q_sqrt under grad
def _predict_grad(case, form, tag):
    M, D, Do, npts = case
    p, X, Wm, Wv = gc.make_inputs(*case)

    def call(word):
        gp, leaves = _gp(p, M, D, Do, PARAMS, form)
        Xd = _dev(X).requires_grad_()
        gsp.poison_pack(gp, word)
        fmean, fvar = gp.predict(Xd)
        gsp.poison_pack(gp, word)
        kl = gp.prior_kl()
        assert fmean.grad_fn is not None and kl.grad_fn is not None
        gsp.poison_pack(gp, word)                            # (the backward runs on the call's own copy of the pack)
        ((_dev(Wm) * fmean).sum() + (_dev(Wv) * fvar).sum() + gc.KL_WEIGHT * kl).backward()
        out = {'fmean': fmean.detach(), 'fvar': fvar.detach(), 'kl': kl.detach(), 'g_X': Xd.grad}
        out.update({'g_' + k: leaves[k].grad for k in PARAMS})
        return out
    out = _three('predict_grad', call, _flags(M, D, Do, grad=True), tag)
    ref = gc.reference(*case)
    _values(out, ref, 1e-12)
    assert float(out['kl']) == pytest.approx(ref['kl'], rel=1e-9)
    for k in ('X',) + PARAMS:
        within_rule('%s predict: %s' % (tag, k), _np(out['g_' + k]).reshape(ref['g_' + k].shape), ref['g_' + k])


@pytest.mark.parametrize('row,form', SHAPES, ids=SHAPE_IDS)
def test_predict_and_prior_kl_under_grad(row, form):
    _predict_grad(gg.predict_case(_row(row)), form, row)


def test_predict_under_grad_wide():
    from cbfssm.hip import lib
    _, M, D, Do = _row(WIDE_ROW)
    assert lib.load().cbfssm_gp_predict_bwd_workgroups(C.byref(lib.pack_layout(M, D, Do)), WIDE_N) >= 128
    _predict_grad((M, D, Do, WIDE_N), None, 'wide')


@pytest.mark.parametrize('row,form', SHAPES, ids=SHAPE_IDS)
def test_conditional_with_a_diagonal_q_sqrt_under_grad(row, form, monkeypatch):
    from cbfssm.model import gp_tf
    from test_gp_fullq_gpu import _diag_reference, _kern
    M, D, Do, npts = case = gg.predict_case(_row(row))
    if form is not None:
        monkeypatch.setenv('CBFSSM_GP_FORM', form)           # (conditional() builds its own pack: the form by the environment)
    p, X, Wm, Wv = gc.make_inputs(*case)
    q = 0.2 * np.exp(np.random.default_rng(3).uniform(-0.5, 0.5, (M, Do)))
    q[::3] *= -1.0

    def call(word):
        kern = _kern(p)
        t = {'Xnew': _dev(X), 'X': _dev(p['zeta_pos']), 'f': _dev(p['zeta_mean']), 'q_sqrt': _dev(q),
             'variance_unc': kern.variance_unc, 'lengthscales_unc': kern.lengthscales_unc}
        for v in t.values():
            v.requires_grad_()
        fmean, fvar = gp_tf.conditional(t['Xnew'], t['X'], kern, t['f'], t['q_sqrt'])
        assert fmean.grad_fn is not None
        ((_dev(Wm) * fmean).sum() + (_dev(Wv) * fvar).sum()).backward()
        out = {'fmean': fmean.detach(), 'fvar': fvar.detach()}
        out.update({'g_' + k: v.grad for k, v in t.items()})
        return out
    out = _three('conditional_diag_grad', call, _flags(M, D, Do, grad=True), row)
    fm_r, fv_r, want = _diag_reference(p, X, Wm, Wv, q)
    _values(out, {'fmean': fm_r, 'fvar': fv_r}, 1e-11)
    for k, r in (('Xnew', want['Xnew']), ('X', want['zeta_pos']), ('f', want['zeta_mean']), ('q_sqrt', want['q']),
                 ('variance_unc', want['variance_unc']), ('lengthscales_unc', want['lengthscales_unc'])):
        within_rule('%s conditional: %s' % (row, k), _np(out['g_' + k]).reshape(r.shape), r)


# ---- full-covariance q(z): predict / prior_kl, evaluation and under grad; conditional() with (Do, M, M) factors
@pytest.mark.parametrize('grad', [False, True], ids=['eval', 'grad'])
@pytest.mark.parametrize('row,form', SHAPES, ids=SHAPE_IDS)
def test_full_q_predict_and_prior_kl(row, form, grad):
    M, D, Do, npts = case = fg.fullq_case(_row(row))
    p, X, Wm, Wv = fq.make_inputs(*case)

    def call(word):
        gp, leaves = _gp(p, M, D, Do, fq.PARAMS if grad else (), form, q_full=True)
        Xd = _dev(X).requires_grad_(grad)
        gsp.poison_pack(gp, word)
        fmean, fvar = gp.predict(Xd)
        gsp.poison_pack(gp, word)
        kl = gp.prior_kl()
        out = {'fmean': fmean.detach(), 'fvar': fvar.detach(), 'kl': kl.detach()}
        assert (fmean.grad_fn is not None) == grad and (kl.grad_fn is not None) == grad
        if grad:
            gsp.poison_pack(gp, word)
            ((_dev(Wm) * fmean).sum() + (_dev(Wv) * fvar).sum() + fq.KL_WEIGHT * kl).backward()
            out['g_X'] = Xd.grad
            out.update({'g_' + k: leaves[k].grad for k in fq.PARAMS})
        return out
    out = _three('fullq_grad' if grad else 'fullq_eval', call, _flags(M, D, Do, grad=grad), row)
    ref = fq.reference(*case)
    _values(out, ref, 1e-11)
    assert float(out['kl']) == pytest.approx(ref['kl'], rel=1e-9)
    if grad:
        for k in ('X',) + fq.PARAMS:
            within_rule('%s full q: %s' % (row, k), _np(out['g_' + k]).reshape(ref['g_' + k].shape), ref['g_' + k])
        upper = np.triu(np.ones((M, M), dtype=bool), 1)
        assert np.all(_np(out['g_zeta_sqrt'])[:, upper] == 0.0)


@pytest.mark.parametrize('row', [FIRST_ROWS[0], FIRST_ROWS[4], C3_ROW])
def test_conditional_with_full_factors_evaluation(row):
    """the (Do, M, M) branch of gp_tf.conditional without a gradient request allocates in gp_tf itself"""
    from cbfssm.model import gp_tf
    from test_gp_fullq_gpu import _kern
    M, D, Do, npts = case = fg.fullq_case(_row(row))
    p, X, _, _ = fq.make_inputs(*case)

    def call(word):
        fmean, fvar = gp_tf.conditional(_dev(X), _dev(p['zeta_pos']), _kern(p), _dev(p['zeta_mean']), _dev(np.tril(p['zeta_sqrt'])))
        assert fmean.grad_fn is None
        return {'fmean': fmean, 'fvar': fvar}
    out = _three('conditional_fullq_eval', call, _flags(M, D, Do), row)
    _values(out, fq.reference(*case), 1e-11)


# ---- rollout
def _rollout(case, form, grad, tag, flip=False):
    from test_gp_rollout_gpu import _check_grads
    M, D, Do, N, T, reverse, with_var = case
    reverse = reverse != flip
    case = (M, D, Do, N, T, reverse, with_var)
    p, h0, a, eps, var_add, W = rc.make_inputs(*case)

    def call(word):
        gp, leaves = _gp(p, M, D, Do, PARAMS if grad else (), form)
        lv = {'h0': _dev(h0).requires_grad_(grad)}
        if D > Do:
            lv['a'] = _dev(a).requires_grad_(grad)
        if with_var:
            lv['var_add'] = _dev(var_add).requires_grad_(grad)
        gsp.poison_pack(gp, word)
        traj, ent = gp.rollout(lv['h0'], lv.get('a'), _dev(eps), lv.get('var_add'), reverse=reverse)
        assert (traj.grad_fn is not None) == grad and traj.shape == (T, N, Do)
        out = {'traj': traj.detach(), 'entropy': ent.detach()}
        if grad:
            gsp.poison_pack(gp, word)
            ((_dev(W) * traj).sum() + rc.ENT_WEIGHT * ent).backward()
            out.update({'g_' + k: v.grad for k, v in lv.items()})
            out.update({'g_' + k: leaves[k].grad for k in PARAMS})
        return out
    out = _three('rollout_grad' if grad else 'rollout_eval', call, _flags(M, D, Do, grad=grad), tag)
    ref = rc.reference(case)
    rc.traj_rule('traj', _np(out['traj']), ref['traj'])
    rc.entropy_rule(float(out['entropy']), ref['entropy'])
    if grad:
        got = {k[2:]: _np(v) for k, v in out.items() if k.startswith('g_')}
        got.setdefault('a', np.zeros((T, N, 0)))
        _check_grads(got, ref, ('h0', 'a') + (('var_add',) if with_var else ()) + PARAMS)


@pytest.mark.parametrize('grad', [False, True], ids=['eval', 'grad'])
@pytest.mark.parametrize('row,form', SHAPES, ids=SHAPE_IDS)
def test_rollout(row, form, grad):
    _rollout(gg.rollout_case(_row(row)), form, grad, row)


@pytest.mark.parametrize('row', [FIRST_ROWS[1], FIRST_ROWS[5], C3_ROW])
def test_rollout_under_grad_every_optional_argument_both_directions(row):
    """var_add present whatever the row derives, and the direction the row does not derive as well"""
    M, D, Do, N, T, reverse, _ = gg.rollout_case(_row(row))
    assert D > Do
    for flip in (False, True):
        _rollout((M, D, Do, N, T, reverse, True), None, True, '%s flip %d' % (row, flip), flip=flip)


def test_rollout_under_grad_wide():
    from cbfssm.hip import lib
    _, M, D, Do = _row(WIDE_ROW)
    assert lib.load().cbfssm_gp_rollout_bwd_workgroups(C.byref(lib.pack_layout(M, D, Do)), WIDE_N) >= 128
    _rollout((M, D, Do, WIDE_N, WIDE_T, False, True), None, True, 'wide')


# ---- filter
def _filter(case, form, grad, tag):
    from test_gp_filter_gpu import _check_grads
    M, D, Do, N, T, reverse, with_vx, k_factor, mask = case
    p, h0, a, ytilde, cond, eps, var_x, var_y, W = fc.make_inputs(*case)

    def call(word):
        gp, leaves = _gp(p, M, D, Do, PARAMS if grad else (), form)
        lv = {'h0': _dev(h0).requires_grad_(grad), 'ytilde': _dev(ytilde).requires_grad_(grad),
              'var_y': _dev(var_y).requires_grad_(grad)}
        if D > Do:
            lv['a'] = _dev(a).requires_grad_(grad)
        if with_vx:
            lv['var_x'] = _dev(var_x).requires_grad_(grad)
        gsp.poison_pack(gp, word)
        traj, kl = gp.filter(lv['h0'], lv.get('a'), lv['ytilde'], _dev(eps), lv.get('var_x'), lv['var_y'], cond=_dev(cond),
                             k_factor=k_factor, reverse=reverse)
        assert (traj.grad_fn is not None) == grad and traj.shape == (T, N, Do)
        out = {'traj': traj.detach(), 'kl': kl.detach()}
        if grad:
            gsp.poison_pack(gp, word)
            ((_dev(W) * traj).sum() + fc.KL_WEIGHT * kl).backward()
            out.update({'g_' + k: v.grad for k, v in lv.items()})
            out.update({'g_' + k: leaves[k].grad for k in PARAMS})
        return out
    out = _three('filter_grad' if grad else 'filter_eval', call, _flags(M, D, Do, grad=grad), tag)
    ref = fc.reference(case)
    fc.traj_rule('traj', _np(out['traj']), ref['traj'])
    fc.kl_rule(float(out['kl']), ref['kl'])
    if grad:
        got = {k[2:]: _np(v) for k, v in out.items() if k.startswith('g_')}
        got.setdefault('a', np.zeros((T, N, 0)))
        _check_grads(got, ref, case)
        if cond is not None:
            assert not np.any(got['ytilde'][cond == 0.0])


@pytest.mark.parametrize('grad', [False, True], ids=['eval', 'grad'])
@pytest.mark.parametrize('row,form', SHAPES, ids=SHAPE_IDS)
def test_filter_random_mask(row, form, grad):
    _filter(fg.filter_case(_row(row)), form, grad, row)


def test_filter_under_grad_wide():
    from cbfssm.hip import lib
    _, M, D, Do = _row(WIDE_ROW)
    assert lib.load().cbfssm_gp_filter_bwd_workgroups(C.byref(lib.pack_layout(M, D, Do)), WIDE_N) >= 128
    _filter((M, D, Do, WIDE_N, WIDE_T, False, True, 1.3, 'random'), None, True, 'wide')


# ---- linearize, transition_jacobians
LIN_ROWS = SHAPES


@pytest.mark.parametrize('variance', [True, False], ids=['variance', 'mean_only'])
@pytest.mark.parametrize('row,form', LIN_ROWS, ids=['%s-%s' % (r, f or 'auto') for r, f in LIN_ROWS])
def test_linearize(row, form, variance):
    from test_gp_linearize_gpu import _check
    M, D, Do, npts = case = gg.predict_case(_row(row))
    p, X, _, _ = gc.make_inputs(*case)

    def call(word):
        gp, _ = _gp(p, M, D, Do, (), form)
        gsp.poison_pack(gp, word)
        return dict(zip(('fmean', 'fvar', 'dmean', 'dvar'), gp.linearize(_dev(X), variance=variance)))
    out = _three('linearize', call, _flags(M, D, Do, variance=variance), row)
    assert (out['dvar'] is None) == (not variance)
    ref = lc.reference_autodiff(*case)
    dvar = out['dvar'] if variance else _dev(ref['dvar'])
    _check(case, (out['fmean'], out['fvar'], out['dmean'], dvar), 'poison')


@pytest.mark.parametrize('row,form', SHAPES, ids=SHAPE_IDS)
def test_transition_jacobians(row, form):
    M, D, Do, npts = case = gg.predict_case(_row(row))
    p, X, _, _ = gc.make_inputs(*case)

    def call(word):
        gp, _ = _gp(p, M, D, Do, (), form)
        gsp.poison_pack(gp, word)
        return dict(zip('AB', gp.transition_jacobians(_dev(X[:, :Do]), _dev(X[:, Do:]) if D > Do else None)))
    out = _three('transition_jacobians', call, _flags(M, D, Do, variance=False), row)
    Ar, Br = lc.transition_reference(*case)
    within_rule('%s A' % row, _np(out['A']), Ar)
    if D > Do:
        within_rule('%s B' % row, _np(out['B']), Br)
    assert out['B'].shape == Br.shape


# ---- moment_match, transition_moments
@pytest.mark.parametrize('cross', [True, False], ids=['cross', 'no_cross'])
@pytest.mark.parametrize('row,form', SHAPES, ids=SHAPE_IDS)
def test_moment_match(row, form, cross):
    from test_gp_moment_match_gpu import _check
    _, M, D, Do = _row(row)
    case = (M, D, Do, mc.N_POINTS)
    p, mean, cov, _ = mc.make_beliefs(*case)

    def call(word):
        gp, _ = _gp(p, M, D, Do, (), form)
        gsp.poison_pack(gp, word)
        return dict(zip(('fmean', 'fcov', 'xcov', 'info'), gp.moment_match(_dev(mean), _dev(cov), cross=cross)))
    out = _three('moment_match', call, _flags(M, D, Do, cross=cross), row)
    assert (out['xcov'] is None) == (not cross)
    _check('%s poison' % row, (out['fmean'], out['fcov'], out['xcov'], out['info']), mc.reference_closed_form(*case))


def test_moment_match_flagged_point():
    """the indefinite covariance of tests/test_gp_moment_match_gpu.py: the flagged point is NaN, info is what it was, every
    other point bitwise the baseline"""
    M, D, Do, npts = 100, 21, 14, 37
    p, mean, cov, _ = mc.make_beliefs(M, D, Do, npts)
    bad = cov.copy()
    bad[20] = -3.0 * np.eye(D) * mc.softplus(p['lengthscales_unc']) ** 2

    def run(c):
        def call(word):
            gp, _ = _gp(p, M, D, Do)
            gsp.poison_pack(gp, word)
            return dict(zip(('fmean', 'fcov', 'xcov', 'info'), gp.moment_match(_dev(mean), _dev(c))))
        return call
    good = _three('moment_match', run(cov), _flags(M, D, Do), 'good')
    out = _three('moment_match', run(bad), _flags(M, D, Do), 'flagged')
    info = _np(out['info'])
    assert info[20] == 1 and not np.delete(info, 20).any() and not _np(good['info']).any()
    keep = torch.tensor(np.delete(np.arange(npts), 20), device=DEV)
    for k in ('fmean', 'fcov', 'xcov'):
        assert torch.isnan(out[k][20]).all() and torch.equal(out[k][keep], good[k][keep]), k


@pytest.mark.parametrize('row,form', SHAPES, ids=SHAPE_IDS)
def test_transition_moments(row, form):
    _, M, D, Do = _row(row)
    case = (M, D, Do, mc.N_POINTS)
    p, mean, cov, _ = mc.make_beliefs(M, D, Do, mc.N_POINTS, 'transition')

    def call(word):
        gp, _ = _gp(p, M, D, Do, (), form)
        gsp.poison_pack(gp, word)
        h, P = _dev(mean[:, :Do]), _dev(cov[:, :Do, :Do])
        return dict(zip(('m', 'P', 'cross', 'info'), gp.transition_moments(h, P, _dev(mean[:, Do:]) if D > Do else None)))
    out = _three('transition_moments', call, _flags(M, D, Do), row)
    mr, Pr, cr = mc.transition_reference(*case)
    assert not _np(out['info']).any()
    for k, r in (('m', mr), ('P', Pr), ('cross', cr)):
        within_rule('%s %s+' % (row, k), _np(out[k]), r, 1e-8)
    assert torch.equal(out['P'], out['P'].transpose(1, 2))


# ---- ekf: evaluation, and differentiable with all eleven gradients and with loglik alone
def _ekf_args(c, grad, **over):
    i = dict(ec.make_inputs(c))
    i.update(over)
    lv = {k: _dev(i[k]).requires_grad_(grad) for k in egc.grad_names(c)}
    return lv, tuple(lv.get(k) for k in ('m0', 'P0', 'a', 'y', 'var_x', 'var_y')), _dev(i['cond'])


@pytest.mark.parametrize('row,form', SHAPES, ids=SHAPE_IDS)
def test_ekf_evaluation(row, form):
    from test_gp_ekf_gpu import _check
    c = ec.grid_case(_row(row))
    M, D, Do = c[:3]
    p = ec.make_inputs(c)['p']

    def call(word):
        gp, _ = _gp(p, M, D, Do, (), form)
        _, args, cond = _ekf_args(c, False)
        gsp.poison_pack(gp, word)
        return dict(zip(('means', 'covs', 'loglik'), gp.ekf(*args, cond=cond)))
    out = _three('ekf_eval', call, _flags(M, D, Do), row)
    _check(c, (out['means'], out['covs'], out['loglik']), 'poison')


def _ekf_grad(c, form, which, tag):
    from test_gp_ekf_grad_gpu import _check
    M, D, Do = c[:3]
    p = ec.make_inputs(c)['p']

    def call(word):
        gp, leaves = _gp(p, M, D, Do, PARAMS, form)
        lv, args, cond = _ekf_args(c, True)
        gsp.poison_pack(gp, word)
        res = gp.ekf(*args, cond=cond, differentiable=True)
        assert all(t.grad_fn is not None for t in res)
        gsp.poison_pack(gp, word)                            # the records between the forward and its backward are the call's own
        names = list(lv) + list(PARAMS)
        gs = torch.autograd.grad(egc.loss_of(c, which, *res), [lv[k] for k in lv] + [leaves[k] for k in PARAMS], allow_unused=True)
        out = dict(zip(('means', 'covs', 'loglik'), (t.detach() for t in res)))
        out.update({'g_' + k: g for k, g in zip(names, gs)})
        return out
    out = _three('ekf_grad', call, _flags(M, D, Do, grad=True, has_P0=c[8]), tag)
    gs = {k[2:]: v for k, v in out.items() if k.startswith('g_')}
    assert len(gs) == 11 - (D == Do)
    _check(c, (out['means'], out['covs'], out['loglik']), gs, 'poison', which)


@pytest.mark.parametrize('which', ['full', 'loglik'])
@pytest.mark.parametrize('row,form', SHAPES, ids=SHAPE_IDS)
def test_ekf_differentiable(row, form, which):
    """`loglik`: only the log-likelihood is used, the cotangents of means and covs reach the entry point as NULL"""
    _ekf_grad(ec.grid_case(_row(row)), form, which, '%s %s' % (row, which))


def test_ekf_differentiable_wide():
    from cbfssm.hip import lib
    _, M, D, Do = _row(WIDE_ROW)
    assert lib.load().cbfssm_gp_ekf_bwd_workgroups(C.byref(lib.pack_layout(M, D, Do)), WIDE_N) >= 128
    _ekf_grad(ec.case(M, D, Do, N=WIDE_N, T=WIDE_T), None, 'full', 'wide')


# ---- eks, adf, ads
EKS_FIELDS = ('smeans', 'scovs', 'loglik', 'means', 'covs', 'pmeans', 'pcovs', 'init_mean', 'init_cov', 'lag_one', 'info')
ADF_FIELDS = ('means', 'covs', 'loglik', 'pmeans', 'pcovs', 'cross', 'info')


def _smoother(entry, c, form, tag, lag_one=None, **over):
    """eks / adf / ads on a case of gp_ekf_cases: the baseline's result as the namedtuple the entry point returns"""
    M, D, Do = c[:3]
    p = ec.make_inputs(c)['p']
    kw = {} if lag_one is None else {'lag_one': lag_one}
    box = {}

    def call(word):
        gp, _ = _gp(p, M, D, Do, (), form)
        _, args, cond = _ekf_args(c, False, **over)
        gsp.poison_pack(gp, word)
        res = getattr(gp, entry)(*args, cond=cond, **kw)
        box.setdefault('type', type(res))
        return dict(zip(res._fields, res))
    out = _three(entry, call, _flags(M, D, Do, lag_one=bool(lag_one)), tag)
    return box['type'](**out)


@pytest.mark.parametrize('lag_one', [True, False], ids=['lag_one', 'no_lag_one'])
@pytest.mark.parametrize('row,form', SHAPES, ids=SHAPE_IDS)
def test_eks(row, form, lag_one):
    from test_gp_eks_gpu import _check
    c = ec.grid_case(_row(row))
    res = _smoother('eks', c, form, row, lag_one)
    assert res._fields == EKS_FIELDS and (res.lag_one is None) == (not lag_one)
    _check(c, res, 'poison', sc.KEYS if lag_one else sc.KEYS[:-1])


@pytest.mark.parametrize('row,form', SHAPES, ids=SHAPE_IDS)
def test_adf(row, form):
    from test_gp_adf_gpu import _check
    c = ec.grid_case(_row(row))
    res = _smoother('adf', c, form, row)
    assert res._fields == ADF_FIELDS
    _check(c, res, 'poison')


@pytest.mark.parametrize('lag_one', [True, False], ids=['lag_one', 'no_lag_one'])
@pytest.mark.parametrize('row,form', SHAPES, ids=SHAPE_IDS)
def test_ads(row, form, lag_one):
    from test_gp_adf_gpu import _check, _figure, RULE
    c = ec.grid_case(_row(row))
    res = _smoother('ads', c, form, row, lag_one)
    assert res._fields == EKS_FIELDS and (res.lag_one is None) == (not lag_one)
    fwd, ref = ac.reference_sequential(c), ac.reference_rts(c)
    for k in ('means', 'covs', 'loglik', 'pmeans', 'pcovs'):
        _figure(c, 'ads', k, _np(getattr(res, k)), fwd[k], RULE)
    for k in ('smeans', 'scovs', 'init_mean', 'init_cov') + (('lag_one',) if lag_one else ()):
        _figure(c, 'ads', k, _np(getattr(res, k)), ref[k], RULE)
    assert not res.info.any()


def test_eks_flagged_chain():
    """tests/test_gp_eks_gpu.py's failed factorisation under poison: what is NaN stays NaN in the same places (the bitwise
    comparison of the three runs), info is unchanged, every other chain is bitwise the good run's baseline"""
    c, n = sc.FAIL_CASE, sc.FAIL_CHAIN
    good = _smoother('eks', c, None, 'good', True)
    bad = _smoother('eks', c, None, 'flagged', True, P0=sc.fail_P0())
    assert int(bad.info[n]) == 1 and int(bad.info.abs().sum()) == 1 and not good.info.any()
    assert torch.isnan(bad.init_mean[n]).all() and torch.isnan(bad.init_cov[n]).all() and torch.isnan(bad.lag_one[0, n]).all()
    others = [k for k in range(c[3]) if k != n]
    for k in ('smeans', 'scovs', 'means', 'covs', 'pmeans', 'pcovs', 'lag_one'):
        assert torch.equal(getattr(good, k)[:, others], getattr(bad, k)[:, others]), k
    for k in ('loglik', 'init_mean', 'init_cov'):
        assert torch.equal(getattr(good, k)[others], getattr(bad, k)[others]), k


def test_adf_and_ads_flagged_chain():
    c, n = ac.FAIL_CASE, ac.FAIL_CHAIN
    expect = torch.zeros(c[3], dtype=torch.int64, device=DEV)
    expect[n] = 1
    keep = torch.tensor([k for k in range(c[3]) if k != n], device=DEV)
    good, bad = _smoother('adf', c, None, 'good'), _smoother('adf', c, None, 'flagged', P0=ac.fail_P0())
    assert torch.equal(bad.info, expect) and not good.info.any()
    for k in ('means', 'covs', 'pmeans', 'pcovs', 'cross'):
        assert torch.isnan(getattr(bad, k)[:, n]).all(), k
        assert torch.equal(getattr(good, k)[:, keep], getattr(bad, k)[:, keep]), k
    assert torch.isnan(bad.loglik[n]) and torch.equal(good.loglik[keep], bad.loglik[keep])
    sg, sb = _smoother('ads', c, None, 'good', True), _smoother('ads', c, None, 'flagged', True, P0=ac.fail_P0())
    assert torch.equal(sb.info, expect) and not sg.info.any()
    for k in ('smeans', 'scovs', 'init_mean', 'init_cov', 'lag_one'):
        ax = 0 if k.startswith('init') else 1
        assert torch.isnan(getattr(sb, k).select(ax, n)).all(), k
        assert torch.equal(getattr(sg, k).index_select(ax, keep), getattr(sb, k).index_select(ax, keep)), k


# ---- the rigid-body filter
def _rigid(case, grad, tag):
    from cbfssm.hip import autograd
    from test_rigid_filter_gpu import _body
    inp = rgc.make_inputs(*case)

    def call(word):
        lv = {k: _dev(inp[k]).requires_grad_(grad) for k in rgc.GRADS}
        fn = autograd.rigid_filter if grad else autograd.rigid_filter_eval
        traj, kl = fn(_body(), lv['x0'], lv['u'], lv['y'], _dev(inp['eps']), lv['var_x'], lv['var_y'])
        assert (traj.grad_fn is not None) == grad
        out = {'traj': traj.detach(), 'kl': kl.detach()}
        if grad:
            ((_dev(inp['W']) * traj).sum() + rgc.KL_WEIGHT * kl).backward()
            out.update({'g_' + k: v.grad for k, v in lv.items()})
        return out
    out = _three('rigid_filter' if grad else 'rigid_filter_eval', call, dict(_flags(1, 1, 1), grad=grad), tag)
    ref = rgc.reference(case)
    rgc.traj_rule('traj', _np(out['traj']), ref['traj'])
    rgc.scalar_rule('kl', float(out['kl']), ref['kl'])
    if grad:
        for k in rgc.GRADS:
            within_rule('rigid: ' + k, _np(out['g_' + k]), ref['g_' + k])


@pytest.mark.parametrize('grad', [False, True], ids=['eval', 'grad'])
def test_rigid_filter(grad):
    _rigid(rgc.CASES[4], grad, str(rgc.CASES[4]))             # three workgroups, a ragged last one


def test_rigid_filter_under_grad_wide():
    from cbfssm.hip import lib
    assert lib.load().cbfssm_rigid_filter_partials(WIDE_RIGID[0]) >= 128
    _rigid(WIDE_RIGID, True, 'wide')


# ---- the primitives: GPPack.predict / predict_f32, RBF.K, cast_cholesky, kmm_chol
def _prepared_pack(p, M, D, Do, form):
    from cbfssm.hip import ops
    pack = ops.GPPack(M, D, Do, torch.device(DEV), form_mode=form)
    pt = {k: _dev(p[k]) for k in PARAMS}
    con = {k: (ops.tf_forward(pt[k]) if k.endswith('_unc') else pt[k]) for k in PARAMS}
    pack.prepare(con['zeta_pos'], con['lengthscales_unc'], con['variance_unc'], con['zeta_mean'], con['zeta_var_unc'])
    return pack


@pytest.mark.parametrize('row,form', SHAPES, ids=SHAPE_IDS)
def test_pack_predict_and_predict_f32(row, form):
    M, D, Do, npts = case = gg.predict_case(_row(row))
    p, X, _, _ = gc.make_inputs(*case)
    ref = gc.reference(*case)

    def f64(word):
        return dict(zip(('fmean', 'fvar'), _prepared_pack(p, M, D, Do, form).predict(_dev(X))))

    def f32(word):
        from cbfssm.hip import ops
        pack = ops.GPPack(M, D, Do, torch.device(DEV), form_mode=form)
        pack.pack_f32()                                      # (the float32 images exist before the poison reaches them)
        gsp.wp.poison(pack, word)
        pt = {k: _dev(p[k]) for k in PARAMS}
        con = {k: (ops.tf_forward(pt[k]) if k.endswith('_unc') else pt[k]) for k in PARAMS}
        pack.prepare(con['zeta_pos'], con['lengthscales_unc'], con['variance_unc'], con['zeta_mean'], con['zeta_var_unc'])
        return dict(zip(('fmean', 'fvar'), pack.predict_f32(_dev(X))))
    out = _three('pack_predict', f64, _flags(M, D, Do), row)
    _values(out, ref, 1e-12)
    out32 = _three('pack_predict_f32', f32, _flags(M, D, Do), row)
    # tests/test_f32_gpu.py holds predict_f32 to 1e-4 of the largest entry of the float64 result on its well-conditioned
    # models (cond_2(K_mm) up to a few hundred).  The float32 cast of K^-1 carries 2^-24 per entry and the contraction
    # amplifies it by cond_2(K_mm), up to 9.8e4 on these rows: the bound is that file's, or 4 cond 2^-24 where that is larger
    tol = max(1e-4, 4.0 * gg.kmm_condition(M, D, Do) * 2.0 ** -24)
    for k in ('fmean', 'fvar'):
        err = float((out32[k] - out[k]).abs().max()) / float(out[k].abs().max())
        print('%s predict_f32 %s: %.2e of the largest entry (bound %.2e)' % (row, k, err, tol))
        assert torch.isfinite(out32[k]).all() and err <= tol, (k, err, tol)


@pytest.mark.parametrize('M,D', [(7, 3), (100, 21), (200, 6), (257, 6)])
def test_rbf_k_cast_cholesky_and_kmm_chol(M, D):
    from cbfssm.hip import ops
    from cbfssm.model import gp_tf
    from oracle import cbfssm_oracle as orc
    rng = np.random.default_rng(M)
    X, X2 = rng.uniform(-2, 2, (M, D)), rng.standard_normal((37, D))
    var, ls = 0.3, rng.uniform(0.8, 2.0, D)
    kref = orc.RBF(orc.tf_backward(np.array([var])), orc.tf_backward(ls))
    K = kref.K(X)

    def k_call(word):
        kern = gp_tf.RBF(var, ls, device=DEV)
        return {'K': kern.K(X), 'K2': kern.K(X, X2)}
    out = _three('rbf_k', k_call, _flags(1, 1, 1), str((M, D)))
    np.testing.assert_allclose(_np(out['K']), K, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(_np(out['K2']), kref.K(X, X2), rtol=1e-12, atol=1e-15)

    def c_call(word):
        return {'L': gp_tf.cast_cholesky(torch.tensor(K, device=DEV)),
                'L32': gp_tf.cast_cholesky(torch.tensor(K, dtype=torch.float32, device=DEV))}
    out = _three('cast_cholesky', c_call, _flags(1, 1, 1), str((M, D)))
    L = _np(out['L'])
    np.testing.assert_allclose(L, orc.cast_cholesky(K), rtol=1e-7, atol=1e-10)
    np.testing.assert_allclose(L @ L.T, K + 1e-8 * np.eye(M), rtol=1e-11, atol=1e-13)
    assert np.all(np.triu(L, 1) == 0.0) and out['L32'].dtype == torch.float32

    def m_call(word):
        kern = gp_tf.RBF(var, ls, device=DEV)
        Kmm, Lm, info = ops.kmm_chol(_dev(X), kern.lengthscales, kern.variance)
        return {'Kmm': Kmm, 'L': Lm, 'info': info}
    out = _three('kmm_chol', m_call, _flags(1, 1, 1), str((M, D)))
    assert float(out['info'][0]) == 0.0
    np.testing.assert_allclose(_np(out['Kmm']), K, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(np.tril(_np(out['L'])), orc.cast_cholesky(K), rtol=1e-7, atol=1e-10)
