"""The tile grid of the GP filter loop and of full-covariance q(z): the rows of tests/gp_tile_grid.py once more, for the four
kernel families that are copies of gp_predict_bwd_kernel / gp_rollout_bwd_kernel / gp_rollout_kernel with one phase replaced

    filter       gp_filter_kernel      (csrc/cbfssm_gp_filter.hpp, launch_gp_filt_n -> launch_gp_filt_t -> launch_gp_filt_k)
    filter_bwd   gp_filter_bwd_kernel  (launch_gp_filt_bwd_n)
    fullq_bwd    gp_fullq_bwd_kernel   (csrc/cbfssm_gp_fullq.hpp, launch_gp_fq_n)
    fullq_fwd    gp_fullq_fwd_kernel   (launch_gp_fq_fwd_n)

(tests/test_gp_filter_fullq_grid_cpu.py holds the proof that the rows reach every compiled leaf,
tests/test_gp_filter_tile_grid_gpu.py and tests/test_gp_fullq_tile_grid_gpu.py run every row against the references of
tests/gp_filter_cases.py and tests/gp_fullq_cases.py).  The leaf of a shape is gp_tile_grid.leaf_key: (NBLK, DK, KT), KT for
the forward filter only; every leaf exists in a dense and a two-triangular form, and every row runs both.

A row (name, M, D, Do) of gp_tile_grid.ROWS gives

    filter_case(row)  (M, D, Do, N = 21, T = 5, reverse = (M odd), var_x = (Do odd), k_factor = (1.0, 1.3, 2.0)[M % 3],
                      'random') of gp_filter_cases: two chain groups, the second ragged; the random mask makes both branches
                      of the conditioned epilogue and of its adjoint run in every leaf, ytilde is NaN where the mask is 0
    fullq_case(row)   (M, D, Do, npts = 37) of gp_fullq_cases: three column blocks, the last ragged

and three more tables exercise the host-side schedules of the full-q path (cbfssm_gp_fullq.hip), restated below:

    FULLQ_BWD_LONG    more column blocks than GpBwdCfg::MAXWG workgroups: the persistent loop of the adjoint goes round twice
    FULLQ_FWD_LONG    more than 4 MAXWG: the same loop of the forward
    FULLQ_SLICE_ROWS  the W_d sum in 2 and in 3 slices of the column blocks (every other case has 1 or 8)

Measured on the CPU (reference against second coding): the filter codings agree to 6.1e-13 of max |traj|, 4.0e-14 on kl and
3.0e-11 of the largest entry of every gradient tensor; no filter gradient tensor's largest entry is below 5.1e-2 and no kl
below 35.4; the mask's zero fraction lies in 0.25 .. 0.42.  The full-q codings agree to 6.0e-13 (values) and 2.2e-11
(gradients) on the rows, to 1.5e-11 at worst on the long and slice cases (the five long cases per table added for the other
tile heights: 1.5e-11 at (320, 12, 4, 16449), 1.3e-12 or better elsewhere; their cond_2(K_mm + 1e-8 I) is at most 1.6e4,
asserted to stay below 1e5; of the older long rows (300, 6, 4) has 1.6e5); min fvar is 3.7e-2 on the rows and 2.6e-2 on the
long cases.  At M = 1, K is a scalar and
the gradient of prior_kl alone with respect to zeta_pos and lengthscales_unc is exactly zero: KL_ZERO names those two.

To extend: a new tile height, input width or trim in any of the four launcher families makes
test_gp_filter_fullq_grid_cpu fail until gp_tile_grid.ROWS has a row that reaches it.
"""
import functools
import re

import gp_tile_grid as gg
import tile_grid as tg
from gp_tile_grid import ROWS, ROW_IDS, ROW_BY_NAME, LONG_ROWS, CHAIN_GROUP_ROWS, leaf_key, trim   # noqa: F401  (re-exported)

N_CHAINS, N_STEPS, N_POINTS = gg.N_CHAINS, gg.N_STEPS, gg.N_POINTS
K_FACTORS = (1.0, 1.3, 2.0)

# (M, D, Do, npts): 260 and 257 column blocks on the 256 workgroups of the stash heights, 1026 on the 1024 of NBLK <= 2
FULLQ_BWD_LONG = LONG_ROWS
# 4099 / 1027 / 2051 column blocks on the forward's 4096 (NBLK <= 2) / 1024 (stash heights) / 2048 (NBLK <= 7) workgroups;
# then the other five tile heights, npts = 16 (cap + k) + r with cap = fullq_fwd_cap(NBLK), 1 <= k <= 4, 1 <= r <= 15
FULLQ_FWD_LONG = [(12, 4, 3, 65573), (130, 6, 4, 16421), (50, 9, 2, 32805),
                  (24, 8, 8, 16 * (4096 + 1) + 7), (99, 7, 5, 16 * (2048 + 3) + 9), (180, 6, 2, 16 * (1024 + 1) + 3),
                  (250, 12, 6, 16 * (1024 + 3) + 13), (320, 12, 4, 16 * (1024 + 4) + 1)]
# 18 column blocks: 2 slices of 9 + 9 (the last block ragged); 41: 3 slices of 14 + 14 + 13
FULLQ_SLICE_ROWS = [(50, 9, 2, 277), (24, 8, 8, 643)]

# gradient tensors of prior_kl alone that are exactly zero by construction
KL_ZERO = ('zeta_pos', 'lengthscales_unc')


def filter_case(row):
    _, M, D, Do = row
    return (M, D, Do, N_CHAINS, N_STEPS, bool(M % 2), bool(Do % 2), K_FACTORS[M % 3], 'random')


def fullq_case(row):
    _, M, D, Do = row
    return (M, D, Do, N_POINTS)


def kl_zero_names(M):
    """the tensors whose prior_kl gradient is exactly zero: K is a scalar at M = 1"""
    return KL_ZERO if M == 1 else ()


# ---- the host-side schedules of cbfssm_gp_fullq.hip, restated
def fq_slices(nblocks):
    """(ns, per) of cbfssm_gp_fullq_wd_f64: ns = clamp(ceil(nblocks / 16), 1, 8) slices of per = ceil(nblocks / ns)"""
    ns = min(max((nblocks + 15) // 16, 1), 8)
    return ns, (nblocks + ns - 1) // ns


def slice_sizes(nblocks):
    """column blocks per slice, as fq_wd_kernel bounds them: [z per, min(z per + per, nblocks))"""
    ns, per = fq_slices(nblocks)
    return [max(min(z * per + per, nblocks) - z * per, 0) for z in range(ns)]


def fullq_bwd_cap(nblk):
    """cbfssm_gp_fullq_bwd_workgroups: GpBwdCfg<NBLK>::MAXWG"""
    return gg.max_workgroups(nblk)


def fullq_fwd_cap(nblk):
    """cbfssm_gp_fullq_predict_f64: 4 GpBwdCfg<NBLK>::MAXWG"""
    return 4 * gg.max_workgroups(nblk)


def _body_of(text, func, ret='int'):
    """gp_tile_grid._body for a function of any return type"""
    m = re.search(r'\b%s %s\([^)]*\)\s*\{' % (ret, func), text)
    assert m, func
    depth, i = 1, m.end()
    while depth:
        depth += {'{': 1, '}': -1}.get(text[i], 0)
        i += 1
    return text[m.end():i]


def source_schedules():
    """what the source text states of the three restatements above: {'maxwg': ((bound, cap), ..., last cap),
    'slices': (blocks per slice step, lowest, highest), 'per': the expression, 'bwd_cap', 'fwd_cap': multiples of MAXWG}"""
    bwd, host = tg._read('cbfssm_gp_bwd.hpp'), tg._read('cbfssm_gp_fullq.hip')
    m = re.search(r'static constexpr int MAXWG = \(NBLK <= (\d+)\) \? (\d+) : \(\(NBLK <= (\d+)\) \? (\d+) : (\d+)\);', bwd)
    assert m, 'GpBwdCfg::MAXWG'
    b1, c1, b2, c2, c3 = (int(v) for v in m.groups())
    body = gg._body(host, 'fq_slices')
    s = re.search(r'const int64_t s = \(nblocks \+ (\d+)\) / (\d+);\s*return int\(s < (\d+) \? \3 : \(s > (\d+) \? \4 : s\)\);', body)
    assert s and int(s.group(1)) + 1 == int(s.group(2)), 'fq_slices'
    per = re.search(r'const int ns = fq_slices\(nblocks\);\s*const int64_t per = ([^;]+);', host)
    assert per, 'per'
    assert re.search(r'static int gp_fq_maxwg\(int NBLK\)\s*\{\s*switch \(NBLK\) \{\s*#define X\(NB\) case NB: return '
                     r'GpBwdCfg<NB>::MAXWG;', host), 'gp_fq_maxwg'
    fwd = re.search(r'cap = (?:(\d+) \* )?int64_t\(gp_fq_maxwg\(L->NBLK\)\);', _body_of(host, 'cbfssm_gp_fullq_predict_f64'))
    back = re.search(r'cap = (?:(\d+) \* )?gp_fq_maxwg\(L->NBLK\);', _body_of(host, 'cbfssm_gp_fullq_bwd_workgroups', 'int64_t'))
    assert fwd and back, 'workgroup caps'
    return {'maxwg': ((b1, c1), (b2, c2), c3), 'slices': (int(s.group(2)), int(s.group(3)), int(s.group(4))),
            'per': per.group(1).strip(), 'fwd_cap': int(fwd.group(1) or 1), 'bwd_cap': int(back.group(1) or 1)}


# ---- the compiled tree, from the source text
@functools.lru_cache(maxsize=None)
def compiled_families():
    """{family: (tile heights, DK values)} of the four launcher families.  Nothing is compiled or imported."""
    filt, fullq = tg._read('cbfssm_gp_filter.hpp'), tg._read('cbfssm_gp_fullq.hpp')
    return {
        'filter': (gg._instantiated('CBF_GPFILT_INSTANTIATE'), gg._case_values(filt, 'launch_gp_filt_n')),
        'filter_bwd': (gg._instantiated('CBF_GPFILT_INSTANTIATE'), gg._case_values(filt, 'launch_gp_filt_bwd_n')),
        'fullq_bwd': (gg._instantiated('CBF_GPFQ_INSTANTIATE'), gg._case_values(fullq, 'launch_gp_fq_n')),
        'fullq_fwd': (gg._instantiated('CBF_GPFQ_INSTANTIATE'), gg._case_values(fullq, 'launch_gp_fq_fwd_n')),
    }


def dispatch_heights():
    """the heights the four host dispatchers switch over: each expands CBF_FOR_EACH_GPBWD_NBLK"""
    for name, funcs in (('cbfssm_gp_filter.hip', ('launch_gp_filt_nb', 'launch_gp_filt_bwd_nb')),
                        ('cbfssm_gp_fullq.hip', ('launch_gp_fq_nb', 'launch_gp_fq_fwd_nb'))):
        text = tg._read(name)
        for f in funcs:
            assert re.search(r'#define X\(NB\) case NB: return %s##NB\([^\n]*\n\s*CBF_FOR_EACH_GPBWD_NBLK\(X\)' % f, text), f
    return gg.dispatch_heights()


@functools.lru_cache(maxsize=None)
def compiled_filter_trims():
    """(the tile height that trims, the KT values launch_gp_filt_t instantiates there)"""
    m = re.search(r'constexpr bool trim_tiles\(\)\s*\{\s*return NBLK == (\d+);\s*\}', tg._read('cbfssm_inst.hpp'))
    assert m, 'trim_tiles'
    text = tg._read('cbfssm_gp_filter.hpp')
    body = gg._body(text, 'launch_gp_filt_t')
    assert 'if constexpr (trim_tiles<NBLK>())' in body
    kts = sorted({int(v) for v in re.findall(r'launch_gp_filt_k<NBLK, DK, (-?\d+)>', body)})
    assert sorted(v for v in kts if v >= 0) == gg._case_values(text, 'launch_gp_filt_t')
    # every DK case of launch_gp_filt_n goes through launch_gp_filt_t
    assert len(re.findall(r'launch_gp_filt_t<NBLK, \d+>', gg._body(text, 'launch_gp_filt_n'))) == \
        len(gg._case_values(text, 'launch_gp_filt_n'))
    return int(m.group(1)), kts


def launcher_template_arguments(func):
    """the template argument lists of the kernel launchers the DK switch of `func` calls, as tuples of strings"""
    name = {'launch_gp_filt_bwd_n': ('cbfssm_gp_filter.hpp', 'launch_gp_filt_bwd_k'),
            'launch_gp_fq_n': ('cbfssm_gp_fullq.hpp', 'launch_gp_fq_k'),
            'launch_gp_fq_fwd_n': ('cbfssm_gp_fullq.hpp', 'launch_gp_fq_fwd_k')}[func]
    body = gg._body(tg._read(name[0]), func)
    return [tuple(a.strip() for a in args.split(',')) for args in re.findall(r'%s<([^>]*)>' % name[1], body)]


def compiled_leaves(family):
    """Every (NBLK, DK) of one launcher family."""
    heights, dks = compiled_families()[family]
    assert heights and dks, family
    return {(nb, dk) for nb in heights for dk in dks}


def compiled_filter_leaves():
    """Every (NBLK, DK, KT) of the forward filter (each exists in the dense and in the two-triangular form)."""
    heights, dks = compiled_families()['filter']
    trim_height, kts = compiled_filter_trims()
    return {(nb, dk, kt) for nb in heights for dk in dks for kt in (kts if nb == trim_height else [-1])}


def reached(rows=None):
    """{(NBLK, DK, KT): [row names]} of the rows, from the host-only layout query"""
    out = {}
    for name, M, D, Do in (ROWS if rows is None else rows):
        out.setdefault(leaf_key(M, D, Do), []).append(name)
    return out


def missing_leaves(rows=None):
    """{family: sorted leaves no row reaches}; empty when the table is complete"""
    got3 = set(reached(rows))
    got2 = {(nb, dk) for nb, dk, _ in got3}
    out = {}
    for family in ('filter_bwd', 'fullq_bwd', 'fullq_fwd', 'filter'):
        miss = sorted(compiled_leaves(family) - got2)
        if miss:
            out[family] = miss
    miss = sorted(compiled_filter_leaves() - got3)
    if miss:
        out['filter (NBLK, DK, KT)'] = miss
    return out
