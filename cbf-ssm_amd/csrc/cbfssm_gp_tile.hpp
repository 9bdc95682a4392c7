// The phases that the GPModel surface kernels share, one definition each.  The kernels are the five adjoints
// (gp_predict_bwd_kernel, gp_rollout_bwd_kernel, gp_filter_bwd_kernel, gp_fullq_bwd_kernel, gp_ekf_bwd_kernel) and the
// three forwards with the adjoints' wave layout (gp_linearize_kernel, gp_ekf_kernel, gp_fullq_fwd_kernel).  All of them
// give a wave RB row blocks of the 16 NBLK x 16 tile of one column block (16 points or chains) and keep the tiles in LDS as
// [row][17].  What fills xq / Fm / Fv, phase G, the carry and the terms a kernel adds to a phase stay in that kernel; a phase
// with insertions keeps its own text and calls the smaller pieces here (the products, the transposes, the Kinvbar step).
//
//   GpWave::setup, setup_forms, hold_kinv   per-wave row-block setup (ok, rbs, Z and cz rows, operand bases, BREG registers)
//   GpWave::kernel_tile                     B   kernel tile of the wave's rows -> registers and LDS, rows m >= M exactly zero
//   GpWave::image_times_tile(_fin)          A-operand image x LDS tile (phases C and F, S_d A2, the forwards' products)
//   GpWave::regs_times_tile, kinv_times     the same product from K^-1 rows held in VGPRs (BREG)
//   GpWave::a2_forms                        A2 in the dense or the two-triangular form, with the sigma^2 - fvar0 partial
//   GpWave::load_upstream, a2bar_diag,      E   A2bar, the two transposes through the wave's own rows, the gMu / gS2
//     phase_E, store_c, load_a, kinv_adjoint    MFMAs, the stash store or the gB accumulation (slot index from the caller)
//   GpWave::kbar, ebar_of, phase_F_tail     F   Kbar, Ebar, the (Z~)^T Ebar partial tiles, the gZ accumulation
//   GpWave::write_slab, write_state_sums,   the slab: gMu / gS2 / gB / gZ, the per-state-dimension sums, the lengthscale sums
//     write_sums                                and the two block sums
//
// Everything is __forceinline__ and takes the register arrays by reference: the kernels compile to the statements they
// held before, in the same order, and every floating-point operation keeps its operands and its association.
#pragma once
#include "cbfssm_adjoint.hpp"

namespace cbfssm {

// v summed over the four lane groups g = l >> 4 (the k index of a 16 x 16 x 4 operand): every lane holds the sum
__device__ __forceinline__ double gp_sum_groups(double v)
{
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

// the upstream adjoints of one column block as MFMA operands
struct GpUpstream {
    double fvsum;                                       // colsum(Fv) of this lane's point
    double fmB[4], fvB[4];                              // B operands [k = d][col = n]
    double fmT[4], fvT[4];                              // the same tiles with the point index as k: [n = 4s+g][col = nl]
};

// accumulators of the parameter adjoints (all column blocks or steps of a workgroup)
template <int NBLK, int RB, int JB, bool STASH>
struct GpAdjAcc {
    static constexpr int NCB = STASH ? 1 : NBLK;
    d4 gMu[RB], gS2[RB], gZ[RB][JB], gB[RB][NCB];

    __device__ __forceinline__ void zero()
    {
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            gMu[i] = d4{0, 0, 0, 0};
            gS2[i] = d4{0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < JB; ++j) gZ[i][j] = d4{0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < NCB; ++j) gB[i][j] = d4{0, 0, 0, 0};
        }
    }
};

// BREG: the wave's rows of the K^-1 image and of the ZT image stay in VGPRs (one row block per wave; the forwards that use
// the K^-1 image 1 + Do times per column block)
template <int NBLK, int RB, int DK, bool BREG = false>
struct GpWave {
    static constexpr int W = (NBLK + RB - 1) / RB, NT = 64 * W, MP = 16 * NBLK, KS = MP / 4;
    static constexpr int JB = (4 * DK + 1 + 15) / 16;
    static constexpr int PD = 17;
    static constexpr int PSL = JB * 256;
    static_assert(!BREG || RB == 1, "K^-1 rows in registers: one row block per wave");

    int tid, l, w, g, nl, KSr;
    bool ok[RB];
    int rbs[RB];
    double Zreg[RB][DK], czr[RB][4];
    const double *bop[RB], *wop[RB], *wtop[RB];
    double breg[BREG ? KS : 1];
    double ztr[BREG ? JB * 4 : 1];

    // ---- per-wave row-block setup
    __device__ __forceinline__ void setup(const PackPtrs& pk, int tid_)
    {
        tid = tid_; l = tid & 63; w = tid >> 6; g = l >> 4; nl = l & 15;
        KSr = pk.KSr;
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            ok[i] = (w * RB + i) < NBLK;
            rbs[i] = ok[i] ? (w * RB + i) : (NBLK - 1);
#pragma unroll
            for (int s = 0; s < DK; ++s) Zreg[i][s] = pk.Zp[(rbs[i] * DK + s) * 64 + l];
#pragma unroll
            for (int r = 0; r < 4; ++r) czr[i][r] = pk.cz[16 * rbs[i] + 4 * r + g];
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) bop[i] = pk.Bp + rbs[i] * KS * 64 + l;
    }
    // the operand images of the two-triangular form (W = L^-1 and W^T)
    __device__ __forceinline__ void setup_forms(const PackPtrs& pk)
    {
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            wop[i] = pk.Wp + rbs[i] * KS * 64 + l;
            wtop[i] = pk.WTp + rbs[i] * KS * 64 + l;
        }
    }
    // BREG: the wave's K^-1 rows and (Z / l)^T operands, loop invariant, into VGPRs (else streamed from L2 at every use)
    __device__ __forceinline__ void hold_kinv(const RevPackPtrs& rk)
    {
        if constexpr (BREG) {
#pragma unroll
            for (int s = 0; s < KS; ++s) breg[s] = bop[0][s * 64];
#pragma unroll
            for (int q = 0; q < JB * 4; ++q) ztr[q] = rk.ZT[rbs[0] * JB * 256 + q * 64 + l];
        }
    }

    // ---- B: kernel tile (rows of this wave); rows m >= M are exactly zero
    __device__ __forceinline__ void kernel_tile(const double* xq, double* Kt, int M, d4 (&kreg)[RB]) const
    {
        double bx[DK], xx = 0.0;
#pragma unroll
        for (int s = 0; s < DK; ++s) {
            bx[s] = xq[(4 * s + g) * PD + nl];
            xx = fma(bx[s], bx[s], xx);
        }
        xx = gp_sum_groups(xx);
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            kreg[i] = d4{0, 0, 0, 0};
            if (ok[i]) {
                d4 e;
#pragma unroll
                for (int r = 0; r < 4; ++r) e[r] = czr[i][r] - 0.5 * xx;
#pragma unroll
                for (int s = 0; s < DK; ++s) e = CBF_MFMA(Zreg[i][s], bx[s], e);
                e = tile_exp4(e);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    kreg[i][r] = (16 * rbs[i] + 4 * r + g < M) ? e[r] : 0.0;
                    Kt[(16 * rbs[i] + 4 * r + g) * PD + nl] = kreg[i][r];
                }
            }
        }
    }

    // ---- (rows of the A-operand image behind aop[i]) x (the [16 NBLK][17] tile in LDS), on two accumulators per row block
    // that fin(i, acc0, acc1) receives.  The image streams from L2 (zero padded to KS k-steps): the operand loads of four
    // k-steps are issued together, ahead of their MFMAs
    template <class Fin>
    __device__ __forceinline__ void image_times_tile_fin(const double* const (&aop)[RB], const double* tile, Fin&& fin) const
    {
        d4 acc[RB][2];
#pragma unroll
        for (int i = 0; i < RB; ++i) { acc[i][0] = d4{0, 0, 0, 0}; acc[i][1] = d4{0, 0, 0, 0}; }
#pragma unroll 1
        for (int s0 = 0; s0 < KSr; s0 += 4) {
            double b[4], av[RB][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int i = 0; i < RB; ++i) av[i][j] = aop[i][(s0 + j) * 64];
                b[j] = tile[(4 * (s0 + j) + g) * PD + nl];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < RB; ++i)
                    if (ok[i]) acc[i][j & 1] = CBF_MFMA(av[i][j], b[j], acc[i][j & 1]);
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) fin(i, acc[i][0], acc[i][1]);
    }
    // out[i] = acc0 + acc1 of that product
    __device__ __forceinline__ void image_times_tile(const double* const (&aop)[RB], const double* tile, d4 (&out)[RB]) const
    {
        image_times_tile_fin(aop, tile, [&](int i, d4 acc0, d4 acc1) { out[i] = acc0 + acc1; });
    }
    // the same product with the wave's K^-1 rows held in VGPRs: the same k-steps in the same order on the same two accumulators
    __device__ __forceinline__ d4 regs_times_tile(const double* tile) const
    {
        d4 acc[2] = {d4{0, 0, 0, 0}, d4{0, 0, 0, 0}};
#pragma unroll
        for (int s0 = 0; s0 < KS; s0 += 4) {
            if (s0 < KSr) {
                double b[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) b[j] = tile[(4 * (s0 + j) + g) * PD + nl];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j & 1] = CBF_MFMA(breg[s0 + j], b[j], acc[j & 1]);
            }
        }
        return acc[0] + acc[1];
    }
    // the rows of K^-1 times a tile: from the registers where they are held, else streamed from L2
    __device__ __forceinline__ void kinv_times(const double* tile, d4 (&out)[RB]) const
    {
        if constexpr (BREG) out[0] = regs_times_tile(tile);
        else image_times_tile(bop, tile, out);
    }

    // ---- A2 of this wave's rows in the form the layout asks for, and this wave's part of sigma^2 - fvar0 (returned before
    // its sum over the lane groups).  dense: A2 = K^-1 k, part = sum_m k a2; two-triangular (gp_tf.py:137-145): A = L^-1 k
    // through A2t and one workgroup barrier, part = sum_m A^2, A2 = L^-T A (A2t still holds A when this returns)
    __device__ __forceinline__ double a2_forms(int tri, const double* Kt, double* A2t, const d4 (&kreg)[RB], d4 (&a2)[RB]) const
    {
        double v0 = 0.0;
        if (tri) {
            d4 A[RB];
            image_times_tile(wop, Kt, A);
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                if (ok[i]) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        v0 = fma(A[i][r], A[i][r], v0);
                        A2t[(16 * rbs[i] + g + 4 * r) * PD + nl] = A[i][r];
                    }
                }
            }
            __syncthreads();
            image_times_tile(wtop, A2t, a2);
        } else {
            kinv_times(Kt, a2);
#pragma unroll
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) v0 = fma(kreg[i][r], a2[i][r], v0);
        }
        return v0;
    }

    // ---- 16 x 16 transposes through a wave's own rows of an LDS tile (nobody else reads them before the next workgroup
    // barrier; the caller puts wave barriers between a store and a load): C-layout (row g+4r, col nl) in, A-operand layout
    // (row nl, k = 4s+g) out
    __device__ __forceinline__ void store_c(double* own, const d4& v) const
    {
#pragma unroll
        for (int r = 0; r < 4; ++r) own[(g + 4 * r) * PD + nl] = v[r];
    }
    __device__ __forceinline__ void load_a(const double* own, double (&vT)[4]) const
    {
#pragma unroll
        for (int s = 0; s < 4; ++s) vT[s] = own[nl * PD + 4 * s + g];
    }

    // ---- E: the upstream adjoints as operands; d fvar / d sigma^2 = 1 (padded columns hold zeros).  FV = false (full-covariance
    // q(z)): Fv enters through its column sum only
    template <bool FV = true>
    __device__ __forceinline__ void load_upstream(const double* Fm, const double* Fv, GpUpstream& u, double& gsig) const
    {
        u.fvsum = 0.0;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            u.fmB[s] = Fm[(4 * s + g) * PD + nl];
            const double fv = Fv[(4 * s + g) * PD + nl];
            if constexpr (FV) u.fvB[s] = fv;
            u.fvsum += fv;
        }
        u.fvsum = gp_sum_groups(u.fvsum);
        if (w == 0 && g == 0) gsig += u.fvsum;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            u.fmT[s] = Fm[nl * PD + 4 * s + g];
            if constexpr (FV) u.fvT[s] = Fv[nl * PD + 4 * s + g];
        }
    }
    // A2bar = mu Fm + 2 A2 o (s2 Fv) - K o colsum(Fv) of row block i (diagonal q(z))
    __device__ __forceinline__ d4 a2bar_diag(int i, const RevPackPtrs& rk, const GpUpstream& u, const d4& a2, const d4& kreg) const
    {
        const double* mBp = rk.muB + rbs[i] * 256 + l;
        const double* sBp = rk.s2B + rbs[i] * 256 + l;
        double mv[4], sv[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) { mv[s] = mBp[s * 64]; sv[s] = sBp[s * 64]; }
        d4 T1 = {0, 0, 0, 0}, T2 = {0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            T1 = CBF_MFMA(mv[s], u.fmB[s], T1);
            T2 = CBF_MFMA(sv[s], u.fvB[s], T2);
        }
        d4 a2bar;
#pragma unroll
        for (int r = 0; r < 4; ++r) a2bar[r] = T1[r] + 2.0 * a2[r] * T2[r] - kreg[r] * u.fvsum;
        return a2bar;
    }
    // Kinvbar += A2bar K^T of row block i.  STASH: A2bar^T and K^T of the row block leave as the MFMA operand images of that
    // product, at the caller's slot (the column block in the batch kernels, workgroup * T + step in the time loops)
    template <bool STASH, int NCB>
    __device__ __forceinline__ void kinv_adjoint(int i, const double (&abT)[4], const double* Kt, int64_t slot, double* stash_a,
                                                 double* stash_k, d4 (&gB)[NCB]) const
    {
        if constexpr (STASH) {
            double* pa = stash_a + (slot * NBLK + rbs[i]) * 256 + l;
            double* pk = stash_k + (slot * NBLK + rbs[i]) * 256 + l;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                pa[s * 64] = abT[s];                                                 // A[row m][k = point]
                pk[s * 64] = Kt[(16 * rbs[i] + nl) * PD + 4 * s + g];                // B[k = point][col m]
            }
        } else {
#pragma unroll
            for (int c2 = 0; c2 < NCB; ++c2) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const double kT = Kt[(16 * c2 + nl) * PD + 4 * s + g];
                    gB[c2] = CBF_MFMA(abT[s], kT, gB[c2]);                           // Kinvbar[m'][m] += A2bar[m'][n] K[m][n]
                }
            }
        }
    }
    // phase E of the diagonal adjoints: A2bar, and the parameter adjoints that contract over the 16 points.  A2bar stays in
    // A2t as the B operand of phase F
    template <bool STASH>
    __device__ __forceinline__ void phase_E(const RevPackPtrs& rk, const GpUpstream& u, const double* Kt, double* A2t,
                                            const d4 (&a2)[RB], const d4 (&kreg)[RB], int64_t slot, double* stash_a,
                                            double* stash_k, GpAdjAcc<NBLK, RB, JB, STASH>& acc) const
    {
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            if (ok[i]) {
                const d4 a2bar = a2bar_diag(i, rk, u, a2[i], kreg[i]);
                double a2T[4], abT[4];
                double* own = A2t + 16 * rbs[i] * PD;
                store_c(own, a2[i]);
                __builtin_amdgcn_wave_barrier();
                load_a(own, a2T);
                __builtin_amdgcn_wave_barrier();
                store_c(own, a2bar);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    acc.gMu[i] = CBF_MFMA(a2T[s], u.fmT[s], acc.gMu[i]);            // mubar[m][d] += A2[m][n] Fm[d][n]
                    acc.gS2[i] = CBF_MFMA(a2T[s] * a2T[s], u.fvT[s], acc.gS2[i]);   // s2bar[m][d] += A2[m][n]^2 Fv[d][n]
                }
                __builtin_amdgcn_wave_barrier();
                load_a(own, abT);
                kinv_adjoint<STASH>(i, abT, Kt, slot, stash_a, stash_k, acc.gB[i]);
            }
        }
    }

    // ---- F: Kbar = K^-1 A2bar - A2 o colsum(Fv) of this wave's rows (A2bar is the tile phase E left in A2t)
    __device__ __forceinline__ void kbar(const double* A2t, const d4 (&a2)[RB], double fvsum, d4 (&kc)[RB]) const
    {
        image_times_tile(bop, A2t, kc);
#pragma unroll
        for (int i = 0; i < RB; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) kc[i][r] = kc[i][r] - a2[i][r] * fvsum;
    }
    // Ebar = Kbar o K, rows m >= M exactly zero
    __device__ __forceinline__ void ebar_of(const d4 (&kc)[RB], const d4 (&kreg)[RB], int M, d4 (&ebar)[RB]) const
    {
#pragma unroll
        for (int i = 0; i < RB; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double v = kc[i][r] * kreg[i][r];
                ebar[i][r] = (ok[i] && 16 * rbs[i] + 4 * r + g < M) ? v : 0.0;
            }
    }
    // the wave's partial tile of xbar~ = (Z~)^T Ebar for ALL input rows -> part, and Zbar~ += Ebar x~^T through a transpose
    // in the wave's own rows of Kt (the K tile is dead behind the barrier that ends phase E)
    __device__ __forceinline__ void phase_F_tail(const double* ZT, double* Kt, const double* xq, double* part,
                                                 const d4 (&ebar)[RB], int D, d4 (&gZ)[RB][JB]) const
    {
        {
            d4 xp[JB];
#pragma unroll
            for (int jb = 0; jb < JB; ++jb) xp[jb] = d4{0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                if (ok[i]) {
                    const double* ZTp = ZT + rbs[i] * JB * 256 + l;
#pragma unroll
                    for (int jb = 0; jb < JB; ++jb)
#pragma unroll
                        for (int r = 0; r < 4; ++r) xp[jb] = CBF_MFMA(ZTp[(jb * 4 + r) * 64], ebar[i][r], xp[jb]);   // rows j, k = m
                }
            }
#pragma unroll
            for (int jb = 0; jb < JB; ++jb)
#pragma unroll
                for (int r = 0; r < 4; ++r) part[w * PSL + (jb * 4 + r) * 64 + l] = xp[jb][r];
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            if (ok[i]) {
                double ebT[4];
                double* ownk = Kt + 16 * rbs[i] * PD;
                store_c(ownk, ebar[i]);
                __builtin_amdgcn_wave_barrier();
                load_a(ownk, ebT);
#pragma unroll
                for (int jb = 0; jb < JB; ++jb) {
                    const int j = 16 * jb + nl;
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        double xT = (j < 4 * DK) ? xq[j * PD + 4 * s + g] : 0.0;
                        if (j == D) xT = 1.0;                                         // ones column: row sums of Ebar
                        gZ[i][jb] = CBF_MFMA(ebT[s], xT, gZ[i][jb]);                  // Zbar~[m][j] += Ebar[m][n] x~[j][n]
                    }
                }
            }
        }
    }

    // ---- this workgroup's slab: the accumulators in the Slab<> layout, the small section zeroed
    template <bool STASH>
    __device__ __forceinline__ void write_slab(double* slab, const GpAdjAcc<NBLK, RB, JB, STASH>& acc) const
    {
        typedef Slab<NBLK, JB, STASH> SL;
        constexpr int NCB = GpAdjAcc<NBLK, RB, JB, STASH>::NCB;
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            if (ok[i]) {
                const int rb = rbs[i];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    slab[SL::gMu + rb * 256 + r * 64 + l] = acc.gMu[i][r];
                    slab[SL::gS2 + rb * 256 + r * 64 + l] = acc.gS2[i][r];
                    if constexpr (!STASH) {
#pragma unroll
                        for (int c2 = 0; c2 < NCB; ++c2) slab[SL::gB + (rb * NBLK + c2) * 256 + r * 64 + l] = acc.gB[i][c2][r];
                    }
#pragma unroll
                    for (int jb = 0; jb < JB; ++jb) slab[SL::gZ + (rb * JB + jb) * 256 + r * 64 + l] = acc.gZ[i][jb][r];
                }
            }
        }
        for (int i = tid; i < 192; i += NT) slab[SL::small + i] = 0.0;
    }
    // NV per-thread sums over the (chain, dim = tid & 15) entries a thread loaded -> slab small [16 q, 16 q + 16) by state
    // dimension (q = 0: d / d var_x, q = 1: d / d var_y): the threads tid' = tid mod 16 that load Fm / Fv entries, in order.
    // Goes through part (W PSL >= NV NT doubles; the steps' readers of part are done) and ends behind a workgroup barrier
    template <bool STASH, int NV>
    __device__ __forceinline__ void write_state_sums(double* slab, double* part, const double (&v)[NV]) const
    {
        typedef Slab<NBLK, JB, STASH> SL;
        static_assert(W * PSL >= NV * NT, "the sums go through the partial tiles");
#pragma unroll
        for (int q = 0; q < NV; ++q) part[q * NT + tid] = v[q];
        __syncthreads();
        if (tid < 16 * NV) {
            constexpr int NL = (NT < 256) ? NT : 256;   // threads that load Fm / Fv entries
            const int d = tid & 15;
            const double* src = part + (tid >> 4) * NT;
            double s = 0.0;
            for (int k = d; k < NL; k += 16) s += src[k];
            slab[SL::small + tid] = s;
        }
    }
    // the lengthscale sums of the phase G lanes (input row j = 4 gi + g, gi = w + k2 W < NG) and the two block sums; behind
    // a workgroup barrier after write_slab
    template <bool STASH, int GPW>
    __device__ __forceinline__ void write_sums(double* slab, const double (&glx)[GPW], double gsig, double glogsig, double* red) const
    {
        typedef Slab<NBLK, JB, STASH> SL;
#pragma unroll
        for (int k2 = 0; k2 < GPW; ++k2) {
            const int gi = w + k2 * W;
            double v = glx[k2];
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (gi < 4 * JB && nl == 0) slab[SL::small + 32 + 4 * gi + g] = v;
        }
        const double s1 = block_sum(gsig, red, tid, NT);
        const double s2 = block_sum(glogsig, red, tid, NT);
        if (tid == 0) {
            slab[SL::small + 96] = s1;
            slab[SL::small + 97] = s2;
        }
    }
};

}  // namespace cbfssm
