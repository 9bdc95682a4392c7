"""The tile grid of the GP-surface kernels: one small workload per compiled leaf of gp_predict_bwd_kernel,
gp_rollout_bwd_kernel and gp_rollout_kernel, and the rule that proves the table complete
(tests/test_gp_tile_grid_cpu.py holds the proof, tests/test_gp_tile_grid_gpu.py runs every row against the oracle).

The host picks a template instantiation from the shape (tests/tile_grid.py states the same for the time loops):

    NBLK  tile height in 16-row blocks of inducing points, M padded up to the next of CBF_FOR_EACH_GPBWD_NBLK
    DK    k-steps of the input width: 2 (D <= 8), 4 (D <= 16), 6 (D <= 24)
    KT    forward rollout only, at the height trim_tiles names (seven row blocks): the number of trimmed all-padding
          k-steps, 4*7 - ceil(M/4) in {0..3}; -1 elsewhere (launch_gp_roll_t, csrc/cbfssm_gp_rollout.hpp)
    TRI   forward rollout only: dense or two-triangular form, chosen at run time from the layout -- every row runs both

What changes with the leaf inside the adjoint kernels: W = ceil(NBLK / RB) waves (RB = 2 in stash mode, NBLK > 7) share
the NG = 4 JB groups of the input-adjoint tile, GPW = ceil(NG / W) each (JB = 1 for DK = 2, else 2): at seven row blocks
with DK 2 or 4 some waves own none or a second one, at one row block a single wave owns all eight and its 64 threads load
the 256 upstream-adjoint entries four each.  The first M of a height leaves whole row blocks of padding behind one data
row; the exact fill has no padding row at all.

A row is (name, M, D, Do); its inputs are derived, not tabulated:

    rollout_case(row)  (M, D, Do, N = 21, T = 5, reverse = (M odd), var_add = (Do odd)) of tests/gp_rollout_cases.py:
                       two chain groups, the second ragged; rows with D == Do have no auxiliary input (Da = 0)
    predict_case(row)  (M, D, Do, npts = 37) of tests/gp_autograd_cases.py: three column blocks, the last ragged

LONG_ROWS (M, D, Do, npts) make the persistent column-block loop of gp_predict_bwd_kernel go round a second time: more
column blocks than the workgroup cap of the height (GpBwdCfg::MAXWG), at most twice as many -- one row per tile height,
because the wave layout, and with it what a second trip can find left over in LDS, differs per height.

Measured on the CPU over the 36 rows (oracle against second coding, see evaluate_predict): cond_2(K_mm + 1e-8 I) is at
most 9.8e4; the two codings agree on every gradient tensor to 2.7e-11 of its largest entry (rollout) and 1.3e-11
(predict; 5.5e-11 on the first three long rows; on the five added for the other tile heights cond_2 is at most 1.6e4 and
the codings agree to 5.4e-13), on the trajectories to 3.1e-12 of max |traj| and on the entropy to 5e-14 relative;
no gradient tensor's largest entry is below 7.9e-3.  D = 4 is not used at M >= 113: on this input family (256, 4, 2) has
cond 4e6 and the codings then agree on the trajectory to 2.9e-9 only.

To extend: a new tile height, input width or trim makes test_gp_tile_grid_cpu fail until ROWS has a row that reaches it.

The same rows run the GP filter loop and full-covariance q(z), whose kernels are copies of these with one phase replaced:
tests/gp_filter_fullq_grid.py derives their cases from ROWS and reads their launchers.
"""
import functools
import os
import re

import numpy as np
import torch

import gp_autograd_cases as gc
import gp_rollout_cases as rc
import tile_grid as tg
from tile_grid import input_steps, trim, last_data_block   # noqa: F401  (re-exported)

N_CHAINS, N_STEPS, N_POINTS = 21, 5, 37

# name: <tile height>_<what it is there for>_<input width>.  first = first M of a height, fill = 16 * NBLK, ktK = trim K
ROWS = [
    ('nb1_first_dk2', 1, 2, 1), ('nb1_fill_dk4', 16, 16, 16), ('nb1_mid_dk6', 9, 17, 16),   # Do = 16: Da = 0 and Da = 1
    ('nb2_first_dk4', 17, 16, 9), ('nb2_fill_dk6', 32, 24, 8), ('nb2_mid_dk2', 24, 8, 8),
    ('nb4_first_dk6', 33, 21, 14), ('nb4_fill_dk2', 64, 4, 1), ('nb4_mid_dk4', 50, 9, 2),
    # seven row blocks: W = 7 waves on NG = 4 (DK 2) or 8 (DK 4, 6) groups, and every trim of the rollout at every width
    ('nb7_first_dk4', 65, 9, 9), ('nb7_first_dk6', 65, 17, 3), ('nb7_kt-1_dk2', 96, 5, 3),
    ('nb7_kt3_dk2', 99, 7, 5), ('nb7_kt3_dk4', 100, 12, 9), ('nb7_kt3_dk6', 100, 21, 14),
    ('nb7_kt2_dk2', 101, 6, 1), ('nb7_kt2_dk4', 104, 10, 4), ('nb7_kt2_dk6', 103, 21, 9),
    ('nb7_kt1_dk2', 108, 5, 2), ('nb7_kt1_dk4', 105, 16, 8), ('nb7_kt1_dk6', 106, 21, 14),
    ('nb7_kt0_dk2', 109, 8, 4), ('nb7_fill_dk4', 112, 13, 7), ('nb7_fill_dk6', 112, 24, 16),
    # stash mode from here on
    ('nb10_first_dk2', 113, 6, 2), ('nb10_fill_dk4', 160, 9, 3), ('nb10_mid_dk6', 130, 21, 14),
    ('nb13_first_dk4', 161, 10, 4), ('nb13_fill_dk6', 208, 21, 7), ('nb13_mid_dk2', 180, 6, 2),
    ('nb16_first_dk6', 209, 21, 14), ('nb16_fill_dk2', 256, 7, 2), ('nb16_mid_dk4', 250, 12, 6),
    ('nb20_first_dk2', 257, 6, 3), ('nb20_fill_dk4', 320, 12, 4), ('nb20_mid_dk6', 300, 21, 7),
]
ROW_IDS = [r[0] for r in ROWS]
ROW_BY_NAME = {r[0]: r for r in ROWS}

# (M, D, Do, npts): 260 and 257 column blocks on the 256 workgroups of the stash heights, 1026 on the 1024 of NBLK <= 2;
# then one row for each of the other five tile heights, npts = 16 (cap + k) + r with cap = max_workgroups(NBLK), 1 <= k <= 4,
# 1 <= r <= 15 (LONG_K_R): a few workgroups go round a second time and the last column block is ragged.  Their (M, D, Do)
# are those of rows of ROWS (nb2_mid_dk2, nb4_mid_dk4, nb7_kt3_dk6 -- the C3 shape --, nb13_mid_dk2, nb16_mid_dk4)
LONG_ROWS = [(130, 6, 4, 4149), (300, 6, 4, 4101), (12, 4, 3, 16405),
             (24, 8, 8, 16 * (1024 + 1) + 7), (50, 9, 2, 16 * (512 + 2) + 3), (100, 21, 14, 16 * (512 + 3) + 9),
             (180, 6, 2, 16 * (256 + 2) + 11), (250, 12, 6, 16 * (256 + 4) + 13)]


def long_k_r(npts, cap):
    """(k, r) of npts = 16 (cap + k) + r with 1 <= r <= 16"""
    blocks = (npts + 15) // 16
    return blocks - 1 - cap, npts - 16 * (blocks - 1)


def long_heights(rows):
    """the tile heights of a long table"""
    return sorted(leaf_key(M, D, Do)[0] for M, D, Do, _ in rows)

# chains 0..15 of a row's N = 21 run against an N = 16 run: one stash height, one below
CHAIN_GROUP_ROWS = ['nb13_mid_dk2', 'nb7_kt1_dk4']


def rollout_case(row):
    _, M, D, Do = row
    return (M, D, Do, N_CHAINS, N_STEPS, bool(M % 2), bool(Do % 2))


def predict_case(row):
    _, M, D, Do = row
    return (M, D, Do, N_POINTS)


def leaf_key(M, D, Do):
    """(NBLK, DK, KT) of a shape, from the host-only layout query"""
    from cbfssm.hip import lib
    lay = lib.pack_layout(M, D, Do)
    return int(lay.NBLK), int(lay.DK), trim(int(lay.NBLK), M)


def max_workgroups(nblk):
    """GpBwdCfg<NBLK>::MAXWG (csrc/cbfssm_gp_bwd.hpp) restated"""
    return 1024 if nblk <= 2 else (512 if nblk <= 7 else 256)


# ---- the compiled tree, from the source text
def _body(text, func):
    """text of the body of the function template `int func(...)`"""
    m = re.search(r'\bint %s\([^)]*\)\s*\{' % func, text)
    assert m, func
    depth, i = 1, m.end()
    while depth:
        depth += {'{': 1, '}': -1}.get(text[i], 0)
        i += 1
    return text[m.end():i]


def _case_values(text, func):
    return sorted(int(v) for v in re.findall(r'\bcase (-?\d+):', _body(text, func)))


def _instantiated(macro):
    """tile heights N of the translation units that consist of `macro(N)`"""
    out = []
    for name in sorted(os.listdir(tg.CSRC)):
        if name.endswith('.hip'):
            out += [int(v) for v in re.findall(r'^%s\((\d+)\)' % macro, tg._read(name), re.M)]
    return sorted(out)


def compiled_families():
    """{family: (tile heights, DK values)} of the three launcher families.  Nothing is compiled or imported."""
    bwd, roll = tg._read('cbfssm_gp_bwd.hpp'), tg._read('cbfssm_gp_rollout.hpp')
    return {
        'predict_bwd': (_instantiated('CBF_GPBWD_INSTANTIATE'), _case_values(bwd, 'launch_gp_bwd_n')),
        'rollout': (_instantiated('CBF_GPROLL_INSTANTIATE'), _case_values(roll, 'launch_gp_roll_n')),
        'rollout_bwd': (_instantiated('CBF_GPROLL_INSTANTIATE'), _case_values(roll, 'launch_gp_roll_bwd_n')),
    }


def dispatch_heights():
    """the heights the three host dispatchers switch over"""
    return tg._heights(tg._read('cbfssm_gp_bwd.hpp'), 'CBF_FOR_EACH_GPBWD_NBLK')


def compiled_trims():
    """(the tile height that trims, the KT values launch_gp_roll_t instantiates there)"""
    m = re.search(r'constexpr bool trim_tiles\(\)\s*\{\s*return NBLK == (\d+);\s*\}', tg._read('cbfssm_inst.hpp'))
    assert m, 'trim_tiles'
    body = _body(tg._read('cbfssm_gp_rollout.hpp'), 'launch_gp_roll_t')
    kts = sorted({int(v) for v in re.findall(r'launch_gp_roll_k<NBLK, DK, (-?\d+)>', body)})
    assert sorted(v for v in kts if v >= 0) == _case_values(tg._read('cbfssm_gp_rollout.hpp'), 'launch_gp_roll_t')
    return int(m.group(1)), kts


def compiled_leaves():
    """Every (NBLK, DK) some launcher family instantiates."""
    leaves = set()
    for key, (heights, dks) in compiled_families().items():
        assert heights and dks, key
        leaves.update((nb, dk) for nb in heights for dk in dks)
    return leaves


def compiled_rollout_leaves():
    """Every (NBLK, DK, KT) of the forward rollout (each exists in the dense and in the two-triangular form)."""
    heights, dks = compiled_families()['rollout']
    trim_height, kts = compiled_trims()
    return {(nb, dk, kt) for nb in heights for dk in dks for kt in (kts if nb == trim_height else [-1])}


# ---- references
def kmm_condition(M, D, Do):
    from oracle import cbfssm_torch_ref as tref
    p, _, _, _ = gc.make_inputs(M, D, Do, 1)
    t, _ = gc.oracle_model(p)
    with torch.no_grad():
        K = tref.RBF(t['variance_unc'], t['lengthscales_unc']).K(t['zeta_pos']) + tref.JITTER * torch.eye(M, dtype=torch.float64)
    return float(np.linalg.cond(K.numpy()))


def evaluate_predict(case, coding='oracle'):
    """the loss of gp_autograd_cases on (M, D, Do, npts) and its gradients 'g_X', 'g_' + name; coding 'second': predict
    through an explicit inverse of K_mm (gp_rollout_cases.second_coding); prior_kl is the oracle's in both"""
    p, X, Wm, Wv = gc.make_inputs(*case)
    t, gp = gc.oracle_model(p)
    Xt = torch.tensor(X, requires_grad=True)
    fmean, fvar = (gp.predict if coding == 'oracle' else rc.second_coding(t))(Xt)
    loss = (torch.tensor(Wm) * fmean).sum() + (torch.tensor(Wv) * fvar).sum() + gc.KL_WEIGHT * gp.prior_kl()
    loss.backward()
    out = {'g_X': Xt.grad.numpy().copy()}
    for k in gc.PARAMS:
        out['g_' + k] = t[k].grad.numpy().copy()
    return out


@functools.lru_cache(maxsize=None)
def predict_reference(case):
    """computed once per case and shared (treat as read-only)"""
    return evaluate_predict(case)
