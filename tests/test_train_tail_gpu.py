"""The five entry points of csrc/cbfssm_tail.hip through ctypes, in every mode, against the autodiff reference of
tests/train_tail_cases.py.  The GP packs come from the library's own prepare, so a wrong Kinv, Kmm, Zs or jitter scalar in
the pack shows up as well.

Tolerance, per tensor, of its largest reference entry: max(1e-12, 20 x the case's CPU floor of that tensor)
(train_tail_cases.floors; the factor covers the pack's K^-1 against the reference's -- two inversions, each good to about
cond eps -- and the GPU's summation order).  A reference tensor that is zero everywhere (prior-KL gradient of zeta_pos and
the lengthscales at M = 1, the zeta_var entries of the full-covariance tail) asks for exact zeros.

Around every call: `work` has exactly the *_work_elems size and starts as NaN (scratch is written before it is read),
sentinel words sit behind `work` and `gflat`, `gflat` starts as a sentinel that every entry must overwrite, every padding
element of the slabs and images is NaN, and a second call must give the same bits."""
import ctypes as C

import pytest
import torch

import train_tail_cases as tc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RUN = tc.runnable()
IDS = [tc.case_id(c) for c in RUN]
GUARD, SENT_WORK, SENT_G = 64, -7.25e33, 1.2345e300
NAN = float('nan')


def _dev(a):
    return a.to(torch.float64).contiguous().to(DEV)


def _guarded(n, fill, sent):
    buf = torch.full((n + GUARD,), sent, dtype=torch.float64, device=DEV)
    buf[:n] = fill
    return buf


class Gp:
    """one GP of a case on the device: raw / constrained parameters, the library's pack(s), slabs and images"""

    def __init__(self, M, D, Do, lsv, seed=0, shared=False):
        from cbfssm.hip import ops
        self.M, self.D, self.Do, self.shared = M, D, Do, shared
        self.t = tc.build(M, D, Do, lsv, seed, shared)
        self.ref = tc.reference(M, D, Do, lsv, seed, shared)
        fl = tc.floors(M, D, Do, lsv, seed, shared)
        self.tol = {k: tc.tolerance(fl[k]) for k in tc.GP_PARAMS}
        self.floor = fl
        t = self.t
        self.con = {k: (tc._sp(t[k]) if k.endswith('_unc') else t[k]) for k in tc.GP_PARAMS}
        self.pack = ops.GPPack(M, D, Do, torch.device(DEV), form_mode='dense')
        self.lay = self.pack.layout
        args = [_dev(self.con[k]) for k in ('zeta_pos', 'lengthscales_unc', 'variance_unc', 'zeta_mean', 'zeta_var_unc')]
        self.pack.prepare(*args)
        self._args, self._klpack, self._qpack = args, None, None
        nb, stash = self.lay.NBLK, bool(self.lay.rev_stash)
        self.gm = tc.g_mode_of(self.lay)
        G = tc.g_image_matrix(self.ref, t)
        img0, imgG = tc.matrix_image(t['B'], nb), tc.matrix_image(G, nb, self.gm)
        # the slab per matrix form; at the stash tile heights the slab has no matrix section and the image travels alone
        self.slab = {0: tc.pack_slab(t, self.lay, None if stash else img0), self.gm: tc.pack_slab(t, self.lay, None if stash else imgG)}
        self.image = {0: _dev(img0) if stash else None, self.gm: _dev(imgG) if stash else None}
        self.ld = M + 3
        self.dense = _dev(tc.dense_ld(t['B'], self.ld)) if stash else None

    def klpack(self):
        """PR-SSM: the pack of the same parameters prepared with jitter 0 (prssm.py:81-82)"""
        from cbfssm.hip import ops
        if self._klpack is None:
            self._klpack = ops.GPPack(self.M, self.D, self.Do, torch.device(DEV), form_mode='dense')
            self._klpack.prepare(*self._args, jitter=0.0)
        return self._klpack

    def qpack(self):
        from cbfssm.hip import lib as _l
        from cbfssm.hip.ops import _ptr, _stream
        if self._qpack is None:
            lib = _l.load()
            self._qpack = torch.full((lib.cbfssm_gp_fullq_pack_elems(C.byref(self.lay)),), NAN, dtype=torch.float64, device=DEV)
            q = _dev(self.t['q_sqrt'])
            _l.check(lib.cbfssm_gp_fullq_prepare_f64(C.byref(self.lay), _ptr(q), _ptr(self._qpack), _stream()), 'fullq prepare')
        return self._qpack

    def flats(self, shared_ls=False, zvar_nan=False):
        """(pflat, cflat) of the five GP tensors in the single-GP order, on the CPU"""
        out = []
        for src in (self.t, self.con):
            parts = []
            for k in tc.GP_PARAMS:
                v = src[k].reshape(-1)
                if k == 'lengthscales_unc' and shared_ls:
                    v = v[:1]
                if k == 'zeta_var_unc' and zvar_nan:
                    v = torch.full_like(v, NAN)
                parts.append(v)
            out.append(torch.cat(parts))
        return out

    def expected(self, klw=1.0, kl='jitter', data=True, shared_ls=False):
        return tc.expected(self.ref, self.t, klw, kl, data, shared_ls)


def _compare(case, entry, variant, got, want, tol, floor=None):
    """every tensor of one launch against the reference; prints one record per tensor, returns the failures"""
    bad = []
    for k in want:
        err = tc.rel_err(got[k].cpu(), want[k])
        line = 'TT|%s|%s|%s|%s|%.2e|%.2e|%.2e' % (case, entry, variant, k, (floor or {}).get(k, 0.0), tol[k], err)
        print(line)
        if not err <= tol[k]:
            bad.append((entry, variant, k, err, tol[k]))
    return bad


def _split(gflat, shapes):
    out, o = {}, 0
    for k, shp in shapes:
        n = 1
        for s in shp:
            n *= s
        out[k] = gflat[o:o + n].reshape(shp)
        o += n
    assert o == gflat.numel()
    return out


def _run_twice(call, nwork, ngrad):
    """call(work, gflat) -> rc, twice on fresh guarded buffers; returns the gradient vector"""
    res = []
    for _ in range(2):
        work = _guarded(nwork, NAN, SENT_WORK)
        gbuf = _guarded(ngrad, SENT_G, SENT_WORK)
        rc = call(work[:nwork], gbuf[:ngrad])
        torch.cuda.synchronize()
        assert rc == 0, rc
        assert bool((work[nwork:] == SENT_WORK).all()), 'the words behind work were written'
        assert bool((gbuf[ngrad:] == SENT_WORK).all()), 'the words behind gflat were written'
        g = gbuf[:ngrad].clone()
        assert bool((g != SENT_G).all()), 'an entry of gflat was not written'
        res.append(g)
    assert torch.equal(res[0], res[1]) or bool(torch.isnan(res[0]).any()), 'two calls differ'
    assert not bool(torch.isnan(res[0]).any()), 'NaN in gflat: padding, the upper block triangle or unwritten scratch was read'
    return res[0]


def _single_shapes(g, shared_ls=False, dim_y=0):
    M, D, Do = g.M, g.D, g.Do
    s = [('zeta_pos', (M, D)), ('zeta_mean', (M, Do)), ('zeta_var_unc', (M, Do)), ('variance_unc', (1,)),
         ('lengthscales_unc', (1 if shared_ls else D,))]
    if dim_y:
        s += [('var_x_unc', (Do,)), ('var_y_unc', (dim_y,))]
    return s


def _two_gp(case, c):
    """cbfssm_train_tail_f64 / _g_f64: gp_f (M, D, Do) and gp_b (M, D, Do - dim_y), dim_x = Do, dim_u = D - Do"""
    from cbfssm.hip import lib as _l
    from cbfssm.hip.ops import _ptr, _stream
    lib = _l.load()
    dim_x, dim_y = c.Do, (c.Do + 1) // 2
    gf, gb = Gp(c.M, c.D, c.Do, c.lsv), Gp(c.M, c.D, dim_x - dim_y, c.lsv, seed=1)
    pl = _l.param_layout(c.M, dim_x, c.D - dim_x, dim_y)
    tf, tb = gf.t, gb.t
    noise = {'var_x_unc': tf['var_x_unc'], 'var_y_unc': tf['var_y_unc']}
    pflat = torch.cat([v for g in (gf, gb) for v in g.flats()[:1]] + [noise['var_x_unc'], noise['var_y_unc']])
    cflat = torch.cat([v for g in (gf, gb) for v in g.flats()[1:]] + [tc._sp(noise['var_x_unc']), tc._sp(noise['var_y_unc'])])
    assert pflat.numel() == pl.total
    pflat, cflat = _dev(pflat), _dev(cflat)
    shapes = [('f.' + k, s) for k, s in _single_shapes(gf)] + [('b.' + k, s) for k, s in _single_shapes(gb)] + \
             [('var_x_unc', (dim_x,)), ('var_y_unc', (dim_x,))]
    # var_x collects both slabs (gp_b's on its own output dims), var_y the slab of gp_f and the log-likelihood's pull
    gvx = tf['gvx'].clone()
    gvx[:gb.Do] += tb['gvx']
    gvy = tf['gvy'].clone()
    gvy[:dim_y] += tf['tail_vy'][:dim_y]
    nvx, nvy = tc.noise_grads(gvx, gvy, noise['var_x_unc'], noise['var_y_unc'])
    want = {'f.' + k: v for k, v in gf.expected().items()}
    want.update({'b.' + k: v for k, v in gb.expected().items()})
    want.update({'var_x_unc': nvx, 'var_y_unc': nvy})
    tol = {'f.' + k: v for k, v in gf.tol.items()}
    tol.update({'b.' + k: v for k, v in gb.tol.items()})
    tol.update({'var_x_unc': tc.TOL_MIN, 'var_y_unc': tc.TOL_MIN})
    floor = {'f.' + k: v for k, v in gf.floor.items()}
    floor.update({'b.' + k: v for k, v in gb.floor.items()})
    nwork = int(lib.cbfssm_train_tail_work_elems(C.byref(gf.lay), C.byref(gb.lay)))
    stash = bool(gf.lay.rev_stash)
    bad = []
    variants = [('f64', 0, 'image' if stash else 'slab')] + ([('f64', 0, 'dense')] if stash else []) + \
               [('g_f64', gf.gm, 'image' if stash else 'slab')]
    for entry, gm, src in variants:
        red = _dev(torch.cat([gf.slab[gm], gb.slab[gm], tc.tail_block(tf, dim_y)]))
        imf, imb, ld = (gf.dense, gb.dense, gf.ld) if src == 'dense' else (gf.image[gm], gb.image[gm], 0)

        def call(work, gflat):
            common = (C.byref(pl), C.byref(gf.lay), _ptr(gf.pack.buf), C.byref(gb.lay), _ptr(gb.pack.buf), _ptr(red), _ptr(imf),
                      _ptr(imb), ld)
            rest = (_ptr(pflat), _ptr(cflat), _ptr(work), _ptr(gflat), _stream())
            if entry == 'f64':
                return lib.cbfssm_train_tail_f64(*common, *rest)
            return lib.cbfssm_train_tail_g_f64(*common, gm, *rest)
        g = _split(_run_twice(call, nwork, int(pl.total)), shapes)
        bad += _compare(case, 'train_tail_' + entry, 'g_mode %d, %s' % (gm, src), g, want, tol, floor)
    return bad


def _half(case, c):
    """cbfssm_train_tail_half_f64: with and without pack_kl and shared_ls, g_mode 0 and 1 / 2, dim_y < Do and == Do"""
    from cbfssm.hip import lib as _l
    from cbfssm.hip.ops import _ptr, _stream
    lib = _l.load()
    gps = {False: Gp(c.M, c.D, c.Do, c.lsv), True: Gp(c.M, c.D, c.Do, c.lsv, shared=True)}
    gm = gps[False].gm
    small = max(1, c.Do // 2)
    bad = []
    for g_mode, kl, shared, dim_y in ((0, False, False, c.Do), (gm, True, False, small), (gm, False, True, c.Do),
                                      (0, True, True, small)):
        g = gps[shared]
        t, lay = g.t, g.lay
        p5, c5 = g.flats(shared_ls=shared)
        pflat = _dev(torch.cat([p5, t['var_x_unc'], t['var_y_unc'][:dim_y]]))
        cflat = _dev(torch.cat([c5, tc._sp(t['var_x_unc']), tc._sp(t['var_y_unc'][:dim_y])]))
        red = _dev(torch.cat([g.slab[g_mode], tc.tail_block(t, dim_y)]))
        klbuf = g.klpack().buf if kl else None
        nwork = int(lib.cbfssm_train_tail_half_work_elems(C.byref(lay)))

        def call(work, gflat):
            return lib.cbfssm_train_tail_half_f64(C.byref(lay), _ptr(g.pack.buf), _ptr(klbuf), int(shared), _ptr(red),
                                                  _ptr(g.image[g_mode]), 0, g_mode, dim_y, _ptr(pflat), _ptr(cflat), _ptr(work),
                                                  _ptr(gflat), _stream())
        got = _split(_run_twice(call, nwork, pflat.numel()), _single_shapes(g, shared, dim_y))
        want = g.expected(1.0, 'nojit' if kl else 'jitter', shared_ls=shared)
        nvx, nvy = tc.noise_grads(t['gvx'], t['gvy'][:dim_y] + t['tail_vy'][:dim_y], t['var_x_unc'], t['var_y_unc'][:dim_y])
        want.update({'var_x_unc': nvx, 'var_y_unc': nvy})
        tol = dict(g.tol, var_x_unc=tc.TOL_MIN, var_y_unc=tc.TOL_MIN)
        bad += _compare(case, 'train_tail_half', 'g_mode %d, %s, %s, dim_y %d' % (g_mode, 'Kkl' if kl else 'Kinv',
                        'shared ls' if shared else 'ARD', dim_y), got, want, tol, g.floor)
    return bad


def _gp_tails(case, c):
    """cbfssm_gp_tail_f64 (kl_weight 0, 0.37, 1; without a slab; the dense image at the stash heights) and
    cbfssm_gp_tail_fullq_f64 with the library's own q pack"""
    from cbfssm.hip import lib as _l
    from cbfssm.hip.ops import _ptr, _stream
    lib = _l.load()
    g = Gp(c.M, c.D, c.Do, c.lsv)
    lay = g.lay
    nwork = int(lib.cbfssm_train_tail_half_work_elems(C.byref(lay)))
    slab = _dev(g.slab[0])
    bad = []
    variants = [(0.0, True, 'natural'), (0.37, True, 'natural'), (1.0, True, 'natural'), (1.0, False, 'none'), (0.37, False, 'none')]
    if lay.rev_stash:
        variants.append((0.37, True, 'dense'))
    p5, c5 = (_dev(v) for v in g.flats())
    for klw, data, src in variants:
        img, ld = (g.dense, g.ld) if src == 'dense' else ((g.image[0], 0) if data else (None, 0))

        def call(work, gflat):
            return lib.cbfssm_gp_tail_f64(C.byref(lay), _ptr(g.pack.buf), _ptr(slab) if data else None, _ptr(img), ld, klw,
                                          _ptr(p5), _ptr(c5), _ptr(work), _ptr(gflat), _stream())
        got = _split(_run_twice(call, nwork, p5.numel()), _single_shapes(g))
        bad += _compare(case, 'gp_tail', 'kl_weight %g, %s' % (klw, 'no slab' if not data else 'slab, matrix: ' + src), got,
                        g.expected(klw, 'jitter', data), g.tol, g.floor)
        if c.M == 1 and not data:       # K_mm is the scalar s^2: nothing of the prior KL reaches z or the lengthscales
            assert bool((got['zeta_pos'] == 0.0).all()) and bool((got['lengthscales_unc'] == 0.0).all())
    # full-covariance q(z): the zeta_var entries of pflat / cflat are not read (NaN here), those of gflat are exactly zero
    pq, cq = (_dev(v) for v in g.flats(zvar_nan=True))
    qpack = g.qpack()
    for klw, data in ((0.37, True), (1.0, False)):
        def call(work, gflat):
            return lib.cbfssm_gp_tail_fullq_f64(C.byref(lay), _ptr(g.pack.buf), _ptr(qpack), _ptr(slab) if data else None,
                                                _ptr(g.image[0]) if data else None, 0, klw, _ptr(pq), _ptr(cq), _ptr(work),
                                                _ptr(gflat), _stream())
        got = _split(_run_twice(call, nwork, pq.numel()), _single_shapes(g))
        assert bool((got['zeta_var_unc'] == 0.0).all()), 'the zeta_var entries of the full-covariance tail are exact zeros'
        bad += _compare(case, 'gp_tail_fullq', 'kl_weight %g, %s' % (klw, 'slab' if data else 'no slab'), got,
                        g.expected(klw, 'fullq', data), g.tol, g.floor)
    return bad


@pytest.mark.parametrize('c', RUN, ids=IDS)
def test_every_entry_point_against_the_independent_adjoint(c):
    case = tc.case_id(c)
    bad = []
    if tc.two_gp(c):
        bad += _two_gp(case, c)
    bad += _half(case, c)
    bad += _gp_tails(case, c)
    assert not bad, '\n'.join('%s [%s] %s: %.2e > %.2e' % b for b in bad)


def test_error_returns_leave_the_gradient_untouched():
    from cbfssm.hip import lib as _l
    from cbfssm.hip.ops import _ptr, _stream
    lib = _l.load()
    for c in (next(c for c in RUN if c.M == 16 and c.Do == 7), next(c for c in RUN if c.M == 113)):
        dim_x, dim_y = c.Do, (c.Do + 1) // 2
        gf, gb = Gp(c.M, c.D, c.Do, c.lsv), Gp(c.M, c.D, dim_x - dim_y, c.lsv, seed=1)
        stash = bool(gf.lay.rev_stash)
        pl = _l.param_layout(c.M, dim_x, c.D - dim_x, dim_y)
        n2 = int(pl.total)
        zeros = torch.zeros(n2, dtype=torch.float64, device=DEV)       # pflat / cflat stand-ins: no call below launches
        red = _dev(torch.cat([gf.slab[0], gb.slab[0], tc.tail_block(gf.t, dim_y)]))
        work = torch.zeros(int(lib.cbfssm_train_tail_work_elems(C.byref(gf.lay), C.byref(gb.lay))) +
                           int(lib.cbfssm_train_tail_half_work_elems(C.byref(gf.lay))), dtype=torch.float64, device=DEV)
        gflat = torch.full((n2,), SENT_G, dtype=torch.float64, device=DEV)
        # the opposite of what the tile height asks for: an image below the stash heights, none at them
        spare = torch.zeros(gf.lay.NBLK ** 2 * 256, dtype=torch.float64, device=DEV)
        wrong_f, wrong_b = (None, None) if stash else (spare, spare)
        right_f, right_b = (gf.image[0], gb.image[0])
        two = lambda imf, imb, gm: lib.cbfssm_train_tail_g_f64(
            C.byref(pl), C.byref(gf.lay), _ptr(gf.pack.buf), C.byref(gb.lay), _ptr(gb.pack.buf), _ptr(red), _ptr(imf), _ptr(imb), 0,
            gm, _ptr(zeros), _ptr(zeros), _ptr(work), _ptr(gflat), _stream())
        half = lambda im, gm, dy, slab=red: lib.cbfssm_train_tail_half_f64(
            C.byref(gf.lay), _ptr(gf.pack.buf), None, 0, _ptr(slab), _ptr(im), 0, gm, dy, _ptr(zeros), _ptr(zeros), _ptr(work),
            _ptr(gflat), _stream())
        gpt = lambda slab, im: lib.cbfssm_gp_tail_f64(C.byref(gf.lay), _ptr(gf.pack.buf), _ptr(slab), _ptr(im), 0, 1.0, _ptr(zeros),
                                                      _ptr(zeros), _ptr(work), _ptr(gflat), _stream())
        gpq = lambda slab, im: lib.cbfssm_gp_tail_fullq_f64(C.byref(gf.lay), _ptr(gf.pack.buf), _ptr(gf.qpack()), _ptr(slab), _ptr(im),
                                                            0, 1.0, _ptr(zeros), _ptr(zeros), _ptr(work), _ptr(gflat), _stream())
        calls = {
            'two GPs, g_mode 3': lambda: two(right_f, right_b, 3),
            'two GPs, g_mode -1': lambda: two(right_f, right_b, -1),
            'two GPs, image of gp_f against the tile height': lambda: two(wrong_f, right_b, 0),
            'two GPs, image of gp_b against the tile height': lambda: two(right_f, wrong_b, 0),
            'f64 entry, images against the tile height': lambda: lib.cbfssm_train_tail_f64(
                C.byref(pl), C.byref(gf.lay), _ptr(gf.pack.buf), C.byref(gb.lay), _ptr(gb.pack.buf), _ptr(red), _ptr(wrong_f),
                _ptr(wrong_b), 0, _ptr(zeros), _ptr(zeros), _ptr(work), _ptr(gflat), _stream()),
            'half, g_mode 3': lambda: half(right_f, 3, dim_y),
            'half, image against the tile height': lambda: half(wrong_f, 0, dim_y),
            'half, dim_y 0': lambda: half(right_f, 0, 0),
            'half, dim_y Do + 1': lambda: half(right_f, 0, c.Do + 1),
            'half, no slab': lambda: half(right_f, 0, dim_y, None),
            'gp tail, image against the tile height': lambda: gpt(red, wrong_f),
            'gp tail, image without a slab': lambda: gpt(None, spare),
            'full-q tail, image against the tile height': lambda: gpq(red, wrong_f),
            'full-q tail, image without a slab': lambda: gpq(None, spare),
        }
        for what, fn in calls.items():
            rc = fn()
            torch.cuda.synchronize()
            assert rc != 0, what
            assert bool((gflat == SENT_G).all()), what + ': gflat was written'
            assert lib.cbfssm_last_error(), what
