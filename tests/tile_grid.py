"""The tile grid: one small workload per compiled leaf of the time-loop kernels, and the rule that proves the table
complete (tests/test_tile_grid_cpu.py holds the proof, tests/test_tile_grid_gpu.py runs every row against the oracle).

The host picks a template instantiation from the shape:

    NBLK  tile height in 16-row blocks of inducing points, M padded up to the next of CBF_FOR_EACH_NBLK
    DK    k-steps of the input width: 2 (D <= 8), 4 (D <= 16), 6 (D <= 24)
    KT    at seven row blocks the number of trimmed all-padding k-steps, 4*7 - ceil(M/4) in {0..3}; -1 elsewhere
          (launch_pass_t / launch_predict_t, csrc/cbfssm_inst.hpp)
    KD    the adjoint's output k-steps at seven row blocks: 2 when the GP has Do <= 8 outputs, else 4
          (launch_rev_t, csrc/cbfssm_adjoint_inst.hpp); 4 at every other height
    mode  'fwd' (forward GP, Do = dim_x) or 'bwd' (backward GP, Do = dim_x - dim_y)

A row of CASES is a set of keyword arguments of cbfssm.synthetic.tiny.  Every row keeps B*S off the multiples of 16 (a
ragged last chain group), both backward runs resample at least once (T >= 2 recog_len) and the entropy weight (tiny's
loss_factors) is not zero, so the adjoint of the backward runs carries signal.  gp_len is chosen per row so that
cond(K_mm + jitter I) < 1e6 for both GPs at the perturbed parameters (checked on the CPU): the 1e-6 gradient rule is
stated for well-conditioned sets.

The input-gradient adjoint (launch_revin_n) is a family of the same tree with its own LDS geometry: the IG_* tables below,
proved complete by tests/test_tile_grid_cpu.py too, run by tests/test_input_grads_tile_grid_gpu.py.

To extend: a new tile height, input width or trim makes test_tile_grid_cpu fail until CASES has a row that reaches it.
"""
import os
import re

from cbfssm import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'cbf-ssm_amd', 'csrc')

PARAM_SEED = 1
PERTURB_SCALE = 0.1


def _case(name, M, dim_x, dim_u, dim_y, gp_len, T=7, B=2, S=5, recog_len=2, **kw):
    d = dict(M=M, dim_x=dim_x, dim_u=dim_u, dim_y=dim_y, gp_len=gp_len, T=T, B=B, S=S, recog_len=recog_len, k_factor=5.)
    d.update(kw)
    return name, d


# name: <tile height>_<what it is there for>_<input width>.  first = first M of a height (one data row in the last data
# row block, whole blocks of padding behind it), fill = 16 * NBLK (no padding row at all).
CASES = [
    # one row block
    _case('nb1_first_dk2', 1, 2, 1, 1, 1.5, T=6, B=2, S=3),
    _case('nb1_fill_dk4', 16, 7, 2, 3, 6.0, B=3, S=3),                       # D = 9
    _case('nb1_mid_dk6', 9, 12, 5, 4, 8.0),                                  # D = 17
    # two row blocks
    _case('nb2_first_dk4', 17, 10, 6, 4, 8.0, T=8, recog_len=3),             # D = 16
    _case('nb2_fill_dk6', 32, 16, 8, 15, 8.0, B=3, S=3),                     # D = 24, dim_x = 16, one hidden dimension
    _case('nb2_mid_dk2', 24, 5, 3, 2, 5.0, B=3, S=7),                        # D = 8
    # four row blocks
    _case('nb4_first_dk6', 33, 14, 7, 7, 8.0),
    _case('nb4_fill_dk2', 64, 4, 1, 1, 1.2, T=9, B=3, S=6),
    _case('nb4_mid_dk4', 50, 9, 3, 2, 5.0, T=8, recog_len=3),
    # seven row blocks, D > 16: every trim; KD = 2 and KD = 4 in both modes
    _case('nb7_first_kt-1_dk6', 65, 14, 7, 7, 8.0),                          # fwd KD 4, bwd KD 2
    _case('nb7_kt3_dk6', 97, 8, 9, 2, 5.0, B=3, S=7),                        # D = 17; fwd KD 2 (dim_x = 8), bwd KD 2
    _case('nb7_kt2_dk6', 103, 16, 5, 7, 6.0, T=8),                           # bwd GP with Do = 9: KD 4 in both modes
    _case('nb7_kt1_dk6', 106, 14, 7, 7, 6.0, T=9, recog_len=3),
    _case('nb7_fill_kt0_dk6', 112, 12, 12, 2, 8.0),                          # D = 24; bwd Do = 10
    # seven row blocks, D <= 8: every trim once more; the K^-1 image leaves the LDS between M = 108 and 109
    _case('nb7_kt-1_dk2', 96, 5, 2, 2, 2.0),                                 # six whole row blocks, one of padding
    _case('nb7_kt3_dk2', 100, 4, 2, 2, 1.8, B=3, S=7),
    _case('nb7_kt2_dk2', 101, 6, 2, 1, 2.5),
    _case('nb7_kt1_dk2', 108, 5, 1, 2, 1.8, T=8, recog_len=3),               # last M with the K^-1 image in LDS
    _case('nb7_kt0_dk2', 109, 4, 4, 1, 2.5),                                 # D = 8; first M that streams K^-1
    # seven row blocks, 8 < D <= 16
    _case('nb7_kt1_dk4', 105, 12, 4, 3, 5.0),                                # D = 16; Do = 9 backward GP
    _case('nb7_kt-1_dk4', 80, 7, 2, 3, 3.0, B=3, S=6),                       # D = 9; KD 2 in both modes
    # ten row blocks (stash mode from here on)
    _case('nb10_first_dk2', 113, 4, 2, 2, 1.8),
    _case('nb10_fill_dk4', 160, 9, 3, 2, 3.5),
    _case('nb10_mid_dk6', 130, 14, 7, 7, 6.0),
    # thirteen row blocks
    _case('nb13_first_dk4', 161, 10, 3, 4, 3.5),
    _case('nb13_fill_dk6', 208, 14, 7, 7, 5.0, T=6),
    _case('nb13_mid_dk2', 180, 5, 2, 2, 1.8, B=3, S=6),
    # sixteen row blocks
    _case('nb16_first_dk6', 209, 14, 7, 7, 5.0, T=6),
    _case('nb16_fill_dk2', 256, 4, 2, 2, 1.2),
    _case('nb16_mid_dk4', 250, 12, 4, 6, 4.0, T=6),                          # Sarcos-like width at the C5-like height
    # twenty row blocks
    _case('nb20_first_dk2', 257, 4, 2, 2, 1.2, T=6),
    _case('nb20_fill_dk4', 320, 8, 4, 4, 3.0, T=6),                          # the largest tile, with its gradient
    _case('nb20_mid_dk6', 300, 14, 7, 7, 5.0, T=6, B=2, S=4),
]
CASE_IDS = [name for name, _ in CASES]
CASE_KW = dict(CASES)

# The K^-1 image of the seven-row-block adjoint stays in LDS at every M for DK = 4 and DK = 6 (kinv_in_lds below), so the
# streamed variant of those widths is reached by running a row once more under CBFSSM_NO_BLDS=1, as
# test_input_adjoint_with_streamed_kinv_at_seven_row_blocks does; DK = 2 reaches both sides by shape (M = 108 / 109).
NO_BLDS_CASES = ['nb7_fill_kt0_dk6', 'nb7_kt1_dk4']

# `condition` False in the gradient block: one row per tile height
GRAD_NOCOND_CASES = ['nb1_fill_dk4', 'nb2_first_dk4', 'nb4_mid_dk4', 'nb7_kt2_dk6', 'nb10_first_dk2', 'nb13_fill_dk6',
                     'nb16_mid_dk4', 'nb20_fill_dk4']

# forward-only variant: one row per tile height above seven row blocks, plus the KT = 1 and KT = 2 rows
HALF_CASES = ['nb10_fill_dk4', 'nb13_first_dk4', 'nb16_first_dk6', 'nb20_mid_dk6', 'nb7_kt1_dk6', 'nb7_kt2_dk6',
              'nb7_kt1_dk2', 'nb7_kt2_dk2', 'nb7_kt1_dk4']

# ---- the input-gradient family (launch_revin_n: rev_kernel<..., IG = true>; tests/test_input_grads_tile_grid_gpu.py) ---------
# Every row of CASES runs with input_grads=True (GRAD_NOCOND_CASES also with `condition` False).  With IG the K^-1 image is
# in LDS at every M of heights 1, 2, 4 and at no M of heights >= 10 (kinv_in_lds(..., ig=True)); at seven row blocks the
# rows reach both placements by shape for every DK.  The streamed kernels of heights 1, 2, 4 run under CBFSSM_NO_BLDS=1,
# every row of those heights once more (one per DK):
IG_NO_BLDS_CASES = ['nb1_first_dk2', 'nb1_fill_dk4', 'nb1_mid_dk6', 'nb2_first_dk4', 'nb2_fill_dk6', 'nb2_mid_dk2',
                    'nb4_first_dk6', 'nb4_fill_dk2', 'nb4_mid_dk4']
# stash-mode time chunks (adjoint_stash_gib = 1e-9: one step / one segment per launch) at the heights above ten row blocks
IG_STASH_CHUNK_CASES = ['nb13_mid_dk2', 'nb16_mid_dk4', 'nb20_mid_dk6']
# forward-only variant (HipHalfGrad, 'rnn' recogniser; the MODE_FWD leaves with RevArgs::half): one row per tile height
IG_HALF_CASES = ['nb1_mid_dk6', 'nb2_mid_dk2', 'nb4_mid_dk4', 'nb7_kt2_dk6', 'nb10_fill_dk4', 'nb13_fill_dk6',
                 'nb16_fill_dk2', 'nb20_fill_dk4']
IG_PRSSM_CASES = ['nb13_first_dk4']


def workload(kw):
    return syn.tiny(**kw)


def setup(kw):
    """(workload, config, perturbed parameters, u, y, noise) of a row -- what tests/test_hip_edges.py::_run builds."""
    w = workload(kw)
    p = syn.perturb_params(syn.make_params(w, seed=PARAM_SEED), scale=PERTURB_SCALE)
    u, y = syn.make_inputs(w)
    return w, w.model_config(), p, u, y, syn.make_noise(w)


def input_steps(D):
    """DK of cbfssm_gp_pack_layout"""
    return 2 if D <= 8 else (4 if D <= 16 else 6)


def trim(nblk, M):
    """KT of launch_pass_t / launch_predict_t (csrc/cbfssm_inst.hpp): trimmed tiles exist at seven row blocks only."""
    if nblk != 7:
        return -1
    kt = 4 * nblk - (M + 3) // 4
    return kt if 0 <= kt <= 3 else -1


def rev_kd(nblk, Do):
    """KD of launch_rev_t (csrc/cbfssm_adjoint_inst.hpp)."""
    return 2 if (nblk == 7 and Do <= 8) else 4


def leaf_keys(kw):
    """The dispatch leaves (NBLK, DK, KT, KD, mode) one row reaches, from the host-only layout query."""
    from cbfssm.hip import lib
    w = workload(kw)
    keys = set()
    for mode, Do in (('fwd', w.dim_x), ('bwd', w.dim_out_b)):
        lay = lib.pack_layout(w.M, w.D, Do)
        keys.add((int(lay.NBLK), int(lay.DK), trim(int(lay.NBLK), w.M), rev_kd(int(lay.NBLK), Do), mode))
    return keys


def revin_leaf_keys(kw, no_blds=False):
    """The kernels (NBLK, DK, mode, K^-1 image in LDS) of launch_revin_k one row launches with input_grads=True."""
    w = workload(kw)
    return {(nb, dk, mode, (not no_blds) and kinv_in_lds(nb, dk, w.M, ig=True)) for nb, dk, _, _, mode in leaf_keys(kw)}


def last_data_block(M):
    """row range [lo, M) of the last 16-row block that holds data: where padding and trimming act"""
    return 16 * ((M - 1) // 16), M


def kinv_in_lds(nblk, dk, M, ig=False):
    """launch_rev_k's `LDS_BASE + NBLK * KSr * 64 <= LDS_LIMIT` (csrc/cbfssm_adjoint_inst.hpp: RevGeom, RevCfg;
    csrc/cbfssm_adjoint.hpp: RevInGeom) restated: True when the K^-1 image of the adjoint lives in LDS.  ig: the same
    switch of launch_revin_k, RevInGeom<DK, IG = true>: SPLITJ off, so PSL = max(JB, 2) * 256 and ECS = 0 at every width."""
    rb = 2 if nblk > 7 else 1
    waves = (nblk + rb - 1) // rb
    jb = (4 * dk + 1 + 15) // 16
    splitj = jb == 2 and not ig
    psl = 272 if splitj else max(jb, 2) * 256
    ecs = 16 if splitj else 0
    base = 2 * 4 * dk * 17 + 2 * (16 * nblk) * 17 + 2 * 16 * 17 + waves * psl + 64 + waves * ecs
    return base + nblk * ((M + 3) // 4) * 64 <= 163840 // 8


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _heights(text, macro):
    m = re.search(r'#define\s+%s\(X\)((?:[ \t]*X\(\d+\))+)' % macro, text)
    assert m, macro
    return [int(v) for v in re.findall(r'X\((\d+)\)', m.group(1))]


def _switch_cases(text, func):
    """{(DK, mode)} of the `case N:` lines inside the body of the function template `func`; a line that names no
    MODE_FWD / MODE_BWD (the float32 launchers take the mode at run time) counts for both."""
    m = re.search(r'\bint %s\(int DK, int mode[^)]*\)\s*\{' % func, text)
    assert m, func
    depth, i = 1, m.end()
    while depth:
        depth += {'{': 1, '}': -1}.get(text[i], 0)
        i += 1
    out = set()
    for line in text[m.end():i].splitlines():
        c = re.search(r'\bcase (\d+):', line)
        if c:
            modes = [md.lower() for md in re.findall(r'\bMODE_(FWD|BWD)\b', line)] or ['fwd', 'bwd']
            out.update((int(c.group(1)), md) for md in modes)
    return out


def _dispatch_heights(text, func):
    """tile heights of the `case N: return func<N>(` lines (the float32 files list them one per line)."""
    return sorted(int(v) for v in re.findall(r'case (\d+): return %s<\1>\(' % func, text))


def compiled_families():
    """{family: (tile heights, {(DK, mode)})} read from the source text of the five launcher families: float64 passes,
    float64 adjoint, float64 input-gradient adjoint (one revin_nb<N>.hip unit per height), float32 passes, float32
    adjoint.  Nothing is compiled or imported."""
    inst, adj = _read('cbfssm_inst.hpp'), _read('cbfssm_adjoint_inst.hpp')
    families = {
        'pass': (_heights(inst, 'CBF_FOR_EACH_NBLK'), _switch_cases(inst, 'launch_pass_n')),
        'rev': (_heights(adj, 'CBF_FOR_EACH_REV_NBLK'), _switch_cases(adj, 'launch_rev_n')),
        'revin': (_heights(adj, 'CBF_FOR_EACH_REV_NBLK'), _switch_cases(adj, 'launch_revin_n')),
    }
    for nb in families['revin'][0]:
        unit = 'revin_nb%d.hip' % nb
        assert os.path.exists(os.path.join(CSRC, unit)) and 'CBF_REVIN_INSTANTIATE(%d)' % nb in _read(unit), unit
    for key, fname, func in (('pass32', 'cbfssm_f32.hip', 'launch32_n'), ('rev32', 'cbfssm_rev32.hip', 'launch_rev32_n')):
        text = _read(fname)
        families[key] = (_dispatch_heights(text, func), _switch_cases(text, func))
    return families


def compiled_leaves():
    """Every (NBLK, DK, mode) some launcher family instantiates."""
    leaves = set()
    for key, (heights, dks) in compiled_families().items():
        assert heights and dks, key
        leaves.update((nb, dk, mode) for nb in heights for dk, mode in dks)
    return leaves
