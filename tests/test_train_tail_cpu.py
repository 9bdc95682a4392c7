"""The train-tail cases on the CPU (tests/train_tail_cases.py): the packers round-trip, every case sits in its
conditioning window, the autodiff reference agrees with central finite differences of F, and the float64 floor of the
tail's formulation (train._gp_adjoint on CPU tensors against the reference) is what profiles/train_tail/README.md records."""
import pytest
import torch

import train_tail_cases as tc

RUN = tc.runnable()
IDS = [tc.case_id(c) for c in RUN]


def test_no_more_than_a_quarter_of_the_listed_combinations_has_no_slab():
    skipped = [tc.case_id(c) for c in tc.CASES if c not in RUN]
    assert 4 * len(skipped) <= len(tc.CASES), skipped
    # what is skipped is exactly the input width no pack layout exists for
    assert all(c.D > 24 for c in tc.CASES if c not in RUN) and all(c.D <= 24 for c in RUN)


def test_the_listed_sizes_reach_every_tile_height_and_index_rule():
    lays = [tc.layout_of(c.M, c.D, c.Do) for c in RUN]
    assert {l.NBLK for l in lays} == set(tc.TILE_HEIGHTS)
    assert {c.M for c in tc.CASES} >= {1, 16, 17, 33, 48, 49, 112, 113, 161, 208, 209, 320}
    assert {c.D for c in tc.CASES} == {1, 9, 16, 17, 24, 32} and {c.Do for c in tc.CASES} == {1, 7, 16}
    by_m = {c.M: l for c, l in zip(RUN, lays)}
    assert by_m[33].NBLK == 4 and by_m[112].NBLK == 7 and not by_m[112].rev_stash      # an empty block; last slab size
    assert by_m[113].rev_stash and tc.g_mode_of(by_m[113]) == 1                        # first stash size, still g_mode 1
    assert tc.g_mode_of(by_m[161]) == 2 and by_m[161].NBLK == 13
    assert {l.JB for l in lays} == {1, 2} and {l.DK for l in lays} == {2, 4, 6}


def test_the_two_gp_entry_points_are_reached_at_every_tile_height():
    assert {tc.layout_of(c.M, c.D, c.Do).NBLK for c in RUN if tc.two_gp(c)} == set(tc.TILE_HEIGHTS)


def test_c_layout_packer_is_the_inverse_of_the_engine_s_unpacker():
    from cbfssm.hip.train import _unpack_c
    for nrb, ncb in ((1, 1), (2, 1), (4, 2), (7, 7), (13, 2)):
        a = torch.arange(256.0 * nrb * ncb, dtype=torch.float64).reshape(16 * nrb, 16 * ncb)
        img = tc.pack_c(a, nrb, ncb)
        assert torch.equal(_unpack_c(img, nrb, ncb), a)
        # the kernel's own index rule (c_image in csrc/cbfssm_tail.hip) on a few elements
        for row, col in ((0, 0), (5, 3), (16 * nrb - 1, 16 * ncb - 1), (16 * nrb - 7, 16 * ncb - 16)):
            rb, rr, cb, nl = row >> 4, row & 15, col >> 4, col & 15
            assert img[((rb * ncb + cb) * 4 + (rr >> 2)) * 64 + 16 * (rr & 3) + nl] == a[row, col]


@pytest.mark.parametrize('c', RUN, ids=IDS)
def test_slab_and_images_round_trip_and_padding_is_nan(c):
    from cbfssm.hip.train import _unpack_c
    t, lay = tc.build_case(c), tc.layout_of(c.M, c.D, c.Do)
    nb, M = lay.NBLK, c.M
    img = tc.matrix_image(t['B'], nb)
    slab = tc.pack_slab(t, lay, None if lay.rev_stash else img)
    assert slab.numel() == lay.rev_slab
    u = tc.unpack_slab(slab, lay)
    for k in ('gMu', 'gS2', 'gZ', 'gvx', 'gvy', 'glx', 'gsig', 'glogsig'):
        assert torch.equal(u[k], t[k]), k
    if not lay.rev_stash:
        assert torch.equal(u['matrix'], t['B'])
    real = 2 * M * c.Do + M * (c.D + 1) + 2 * c.Do + c.D + 2 + (0 if lay.rev_stash else M * M)
    assert int((~torch.isnan(slab)).sum()) == real                  # everything else is NaN
    dense = _unpack_c(img, nb, nb)
    assert torch.equal(dense[:M, :M], t['B']) and int((~torch.isnan(dense)).sum()) == M * M
    # g_mode 2: lower blocks of G + G^T, diagonal blocks of G, the upper block triangle NaN
    G = tc.g_image_matrix(tc.reference_case(c), t)
    d2 = _unpack_c(tc.matrix_image(G, nb, 2), nb, nb)[:M, :M]
    blk = torch.arange(M) // 16
    low, dia, upp = blk[:, None] > blk[None, :], blk[:, None] == blk[None, :], blk[:, None] < blk[None, :]
    assert torch.equal(d2[low], (G + G.T)[low]) and torch.equal(d2[dia], G[dia]) and bool(torch.isnan(d2[upp]).all())
    ld = M + 3
    dl = tc.dense_ld(t['B'], ld).reshape(M, ld)
    assert torch.equal(dl[:, :M], t['B']) and bool(torch.isnan(dl[:, M:]).all())
    assert not torch.allclose(t['B'], t['B'].T) or M == 1           # a symmetric B would hide a wrong symmetrisation


@pytest.mark.parametrize('c', RUN, ids=IDS)
def test_condition_number_lies_in_the_case_s_window(c):
    cond, cond_s = tc.reference_case(c).cond, tc.reference_case(c, shared=True).cond
    print('%s cond_2(K + jitter I) = %.3g, with one shared lengthscale %.3g' % (tc.case_id(c), cond, cond_s))
    assert c.cond_lo <= cond <= c.cond_hi * (1 + 1e-12) and c.cond_lo <= cond_s <= c.cond_hi * (1 + 1e-12)
    if c.M == 1:
        assert cond == 1.0


@pytest.mark.parametrize('c', sorted(RUN, key=lambda c: c.M * (c.D + 2 * c.Do))[:3], ids=tc.case_id)
@pytest.mark.parametrize('kl,klw', [('jitter', 1.0), ('nojit', 1.0), ('fullq', 0.37)])
def test_reference_agrees_with_central_finite_differences(c, kl, klw):
    """a check of the reference's plumbing (signs, which term sees which parameter, factors of two), whose errors are of
    order one; not the source of any tolerance.  Bound 1e-4: with h = 1e-6 the difference quotient carries the rounding of F,
    about eps |z~|^2 cond |F| / h (3e-5 at M16-D1-Do1, where |z~| reaches 37), besides its own h^2 truncation"""
    t, ref = tc.build_case(c), tc.reference_case(c)
    want = tc.expected(ref, t, klw, kl)
    h = 1e-6
    Zs0 = tc.kernel_parts(tc.leaves(t, False))[3]
    Cz = t['gZ'][:, :c.D] - Zs0 * t['gZ'][:, c.D:]                  # C is a constant of F, not a function of Z / ls
    for k in tc.GP_PARAMS:
        fd = torch.zeros_like(t[k]).reshape(-1)
        for i in range(fd.numel()):
            vals = []
            for s in (+1.0, -1.0):
                th = tc.leaves(t, False)
                th[k].reshape(-1)[i] += s * h
                vals.append(float(tc.objective(t, th, klw, kl, Cz=Cz)))
            fd[i] = (vals[0] - vals[1]) / (2 * h)
        if kl == 'fullq' and k == 'zeta_var_unc':
            # F's <gS2, zvar> term belongs to the diagonal q(z) only: expected() drops it as the kernel writes zeros
            assert float(want[k].abs().max()) == 0.0 and float(fd.abs().max()) == 0.0
            continue
        err = tc.rel_err(fd, want[k])
        assert err < 1e-4 or (c.M == 1 and float(want[k].abs().max()) == 0.0 and float(fd.abs().max()) < 1e-9), (k, err)


def test_m1_prior_kl_does_not_depend_on_z_or_the_lengthscales():
    c = next(c for c in RUN if c.M == 1)
    ref = tc.reference_case(c)
    for kl in ('jitter', 'nojit', 'fullq'):
        assert float(ref.parts[kl]['zeta_pos'].abs().max()) == 0.0
        assert float(ref.parts[kl]['lengthscales_unc'].abs().max()) == 0.0


@pytest.mark.parametrize('c', RUN, ids=IDS)
def test_float64_floor_of_the_tail_s_formulation(c):
    """|train._gp_adjoint (CPU tensors, stand-in pack from the reference) - autodiff reference| / max|reference| per tensor:
    two correct float64 evaluations differ by about 2e-17 cond (two orderings of the reference itself: 2e-14 at cond 1e3),
    and the chain to zeta_pos / lengthscales forms rowsum(Ws) o z~ - Ws z~ from terms of size |Ws| |z~| and multiplies by z~
    once more, so the restatement must sit within 1e-14 (1 + cond) (1 + max|z~|^2) (only M16-D1-Do1, lengthscale 0.08 and
    |z~| up to 37, has a z~ factor above 3); a larger number is an error in one of the two, not rounding"""
    for shared in (False, True):
        fl, ref = tc.floors_case(c, shared=shared), tc.reference_case(c, shared=shared)
        cond, zs2 = ref.cond, float(ref.Zs.abs().max()) ** 2
        print('FLOOR|%s|%s|%.3g|' % (tc.case_id(c), 'shared' if shared else 'ard', cond) + '|'.join('%.2e' % fl[k] for k in tc.GP_PARAMS))
        for k in tc.GP_PARAMS:
            assert fl[k] <= 1e-14 * (1.0 + cond) * (1.0 + zs2), (k, fl[k])
            assert tc.tolerance(fl[k]) >= 1e-12
