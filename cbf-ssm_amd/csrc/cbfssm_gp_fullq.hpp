// Batch adjoint of the full-covariance conditional (gp_tf.py:68-100 with q_sqrt of shape (Do, M, M), and the
// zeta_std.ndims == 3 branch of GPModel.predict, gp_tf.py:150-159): q(z_d) = N(f_d, S_d), S_d = L_d L_d^T, L_d = tril(q_sqrt[d]).
//
//   fvar[n][d] = sigma^2 - k_n^T a_n + a_n^T S_d a_n,   a_n = K^-1 k_n
//
// This is gp_predict_bwd_kernel (cbfssm_gp_bwd.hpp) as a copy -- that kernel keeps its code -- with one term of phase E
// replaced and one result added:
//
//   D'  A2 of the whole block -> LDS (every wave needs all rows) and -> one C-layout image per column block, from
//       which cbfssm_gp_fullq_wd_f64 forms W_d = sum_n Fv[n][d] a_n a_n^T afterwards
//   E   A2bar = mu Fm + 2 sum_d (S_d A2) diag(Fv[:, d]) - K o colsum(Fv)
//       S_d streams from L2 as an A-operand image in the layout of the pack's K^-1 image (built once per call by
//       cbfssm_gp_fullq_prepare_f64), four k-steps of loads issued together; the per-dimension scaling by Fv happens on the
//       finished 16 x 16 product, outside the MFMA loop.  The sigma_z^2 section of the slab stays zero.
//
// Everything downstream of A2bar (phases E-G, the slab, the stash images above M = 112) is the diagonal kernel's.
#pragma once
#include "../../include/cbfssm_hip.h"
#include "cbfssm_gp_bwd.hpp"

namespace cbfssm {

struct GpFqArgs {
    PackPtrs pk;
    RevPackPtrs rk;
    const double* X;       // (npts, D)
    const double* gmean;   // (npts, Do)
    const double* gvar;    // (npts, Do)
    double* gX;            // (npts, D)
    double* gpart;         // [workgroup][slab]
    int64_t slab;
    int64_t npts;
    int64_t nblocks;       // ceil(npts / 16)
    double* stash_a;       // stash tile heights: [column block][NBLK][4][64] operand images (A2bar^T, K^T)
    double* stash_k;
    const double* Sp;      // [Do][NBLK][KS][64]  S_d as A-operand images (rows / columns >= M zero)
    double* a2img;         // [column block][NBLK][4][64]  A2 in the MFMA C layout
    int M, D, Do;
};

template <int NBLK, int DK>
struct GpFqGeom {
    typedef GpBwdCfg<NBLK> C;
    static constexpr int JB = (4 * DK + 1 + 15) / 16;
    static constexpr int PD = 17;
    static constexpr int LDS_DOUBLES = 4 * DK * PD + 2 * (16 * NBLK) * PD + 2 * 16 * PD + C::W * JB * 256 + 64;
    static constexpr int SLAB = Slab<NBLK, JB, C::STASH>::total;
    static_assert(LDS_DOUBLES <= 163840 / 8, "LDS budget");
};

template <int NBLK, int RB, int DK, bool STASH>
__global__ __launch_bounds__(64 * ((NBLK + RB - 1) / RB)) void gp_fullq_bwd_kernel(GpFqArgs a)
{
    constexpr int W = (NBLK + RB - 1) / RB, NT = 64 * W, MP = 16 * NBLK, KS = MP / 4;
    constexpr int JB = (4 * DK + 1 + 15) / 16;
    constexpr int NG = 4 * JB;                          // 4-row groups of the input-adjoint tile
    constexpr int GPW = (NG + W - 1) / W;               // groups per wave in phase G
    constexpr int PD = 17;
    constexpr int PSL = JB * 256;
    typedef Slab<NBLK, JB, STASH> SL;

    extern __shared__ double lds[];
    double* xq = lds;                                   // [4 DK][17] scaled inputs x~[j][n]
    double* Kt = xq + 4 * DK * PD;                      // [MP][17]  kernel tile, then Ebar transposes
    double* A2t = Kt + MP * PD;                         // [MP][17]  A2 of the block (B operand of S_d A2), then the A2bar tile
    double* Fm = A2t + MP * PD;                         // [16][17]  d loss / d fmean [d][n]
    double* Fv = Fm + 16 * PD;                          // [16][17]
    double* part = Fv + 16 * PD;                        // [W][PSL]  per-wave partial tiles of (Z~)^T Ebar
    double* red = part + W * PSL;                       // 64

    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, g = l >> 4, nl = l & 15;
    const int M = a.M, D = a.D, Do = a.Do;
    const int KSr = a.pk.KSr;

    bool ok[RB];
    int rbs[RB];
    double Zreg[RB][DK], czr[RB][4];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        ok[i] = (w * RB + i) < NBLK;
        rbs[i] = ok[i] ? (w * RB + i) : (NBLK - 1);
#pragma unroll
        for (int s = 0; s < DK; ++s) Zreg[i][s] = a.pk.Zp[(rbs[i] * DK + s) * 64 + l];
#pragma unroll
        for (int r = 0; r < 4; ++r) czr[i][r] = a.pk.cz[16 * rbs[i] + 4 * r + g];
    }
    const double* bop[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) bop[i] = a.pk.Bp + rbs[i] * KS * 64 + l;

    // ---- accumulators of the parameter adjoints (all column blocks of this workgroup)
    constexpr int NCB = STASH ? 1 : NBLK;
    d4 gMu[RB], gZ[RB][JB], gB[RB][NCB];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        gMu[i] = d4{0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < JB; ++j) gZ[i][j] = d4{0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < NCB; ++j) gB[i][j] = d4{0, 0, 0, 0};
    }
    double glx[GPW];
#pragma unroll
    for (int k2 = 0; k2 < GPW; ++k2) glx[k2] = 0.0;
    double gsig = 0.0, glogsig = 0.0;
    // phase G lanes: input row j = 4 gi + g, gi = w + k2 W < NG; 1 / lengthscale of that row
    double ilg[GPW];
#pragma unroll
    for (int k2 = 0; k2 < GPW; ++k2) {
        const int j = 4 * (w + k2 * W) + g;
        ilg[k2] = (j < D) ? a.pk.invl[j] : 0.0;
    }

    for (int64_t cb = blockIdx.x; cb < a.nblocks; cb += gridDim.x) {
        const int64_t p0 = cb * 16;
        __syncthreads();                                // the previous block's readers of xq / part / Fm / Fv are done
        for (int i = tid; i < 4 * DK * 16; i += NT) {
            const int j = i >> 4, n = i & 15;
            const int64_t p = p0 + n;
            double v = 0.0;
            if (j < D && p < a.npts) v = a.X[p * D + j] * a.pk.invl[j];
            xq[j * PD + n] = v;
        }
        for (int i = tid; i < 256; i += NT) {
            const int n = i >> 4, d = i & 15;           // (d fastest: the upstream adjoints are (npts, Do))
            const int64_t p = p0 + n;
            double vm = 0.0, vv = 0.0;
            if (d < Do && p < a.npts) { vm = a.gmean[p * Do + d]; vv = a.gvar[p * Do + d]; }
            Fm[d * PD + n] = vm;
            Fv[d * PD + n] = vv;
        }
        __syncthreads();

        // ---- B: kernel tile (rows of this wave); rows m >= M are exactly zero
        d4 kreg[RB];
        {
            double bx[DK], xx = 0.0;
#pragma unroll
            for (int s = 0; s < DK; ++s) {
                bx[s] = xq[(4 * s + g) * PD + nl];
                xx = fma(bx[s], bx[s], xx);
            }
            xx += __shfl_xor(xx, 16);
            xx += __shfl_xor(xx, 32);
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
        __syncthreads();

        // ---- C: A2 rows of this wave.  K^-1 streams from L2 as the A-operand image of the pack (zero padded to KS
        // k-steps): the operand loads of four k-steps are issued together, ahead of their MFMAs
        d4 a2[RB];
        {
            d4 acc[RB][2];
#pragma unroll
            for (int i = 0; i < RB; ++i) { acc[i][0] = d4{0, 0, 0, 0}; acc[i][1] = d4{0, 0, 0, 0}; }
#pragma unroll 1
            for (int s0 = 0; s0 < KSr; s0 += 4) {
                double b[4], aop[RB][4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
#pragma unroll
                    for (int i = 0; i < RB; ++i) aop[i][j] = bop[i][(s0 + j) * 64];
                    b[j] = Kt[(4 * (s0 + j) + g) * PD + nl];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int i = 0; i < RB; ++i)
                        if (ok[i]) acc[i][j & 1] = CBF_MFMA(aop[i][j], b[j], acc[i][j & 1]);
            }
#pragma unroll
            for (int i = 0; i < RB; ++i) a2[i] = acc[i][0] + acc[i][1];
        }

        // ---- D': A2 of the whole block where every wave reads it, and as this column block's C-layout image (W_d)
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            if (ok[i]) {
                double* own = A2t + 16 * rbs[i] * PD;
                double* pi = a.a2img + (cb * NBLK + rbs[i]) * 256 + l;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    own[(g + 4 * r) * PD + nl] = a2[i][r];
                    pi[r * 64] = a2[i][r];
                }
            }
        }
        __syncthreads();
        // sq[m][n] = sum_d (S_d A2)[m][n] Fv[d][n]: one product like phase C per output dimension, S_d streamed from L2;
        // the scaling by Fv is one multiply-add per finished accumulator entry
        d4 sq[RB];
#pragma unroll
        for (int i = 0; i < RB; ++i) sq[i] = d4{0, 0, 0, 0};
#pragma unroll 1
        for (int d = 0; d < Do; ++d) {
            const double* sop[RB];
#pragma unroll
            for (int i = 0; i < RB; ++i) sop[i] = a.Sp + (int64_t(d) * NBLK + rbs[i]) * KS * 64 + l;
            d4 acc[RB][2];
#pragma unroll
            for (int i = 0; i < RB; ++i) { acc[i][0] = d4{0, 0, 0, 0}; acc[i][1] = d4{0, 0, 0, 0}; }
#pragma unroll 1
            for (int s0 = 0; s0 < KSr; s0 += 4) {
                double b[4], aop[RB][4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
#pragma unroll
                    for (int i = 0; i < RB; ++i) aop[i][j] = sop[i][(s0 + j) * 64];
                    b[j] = A2t[(4 * (s0 + j) + g) * PD + nl];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int i = 0; i < RB; ++i)
                        if (ok[i]) acc[i][j & 1] = CBF_MFMA(aop[i][j], b[j], acc[i][j & 1]);
            }
            const double fvd = Fv[d * PD + nl];
#pragma unroll
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) sq[i][r] = fma(acc[i][0][r] + acc[i][1][r], fvd, sq[i][r]);
        }
        __syncthreads();                                // every wave is done reading the A2 tile: phase E overwrites it

        // ---- E: A2bar, and the parameter adjoints that contract over the 16 points
        double fvsum = 0.0;
        double fmB[4], fvB[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            fmB[s] = Fm[(4 * s + g) * PD + nl];
            fvB[s] = Fv[(4 * s + g) * PD + nl];
            fvsum += fvB[s];
        }
        fvsum += __shfl_xor(fvsum, 16);
        fvsum += __shfl_xor(fvsum, 32);
        if (w == 0 && g == 0) gsig += fvsum;            // d fvar / d sigma^2 = 1 (columns beyond npts hold zeros)
        double fmT[4];                                  // the same tile with the point index as k: [n = 4s+g][col = nl]
#pragma unroll
        for (int s = 0; s < 4; ++s) fmT[s] = Fm[nl * PD + 4 * s + g];
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            if (ok[i]) {
                const double* mBp = a.rk.muB + rbs[i] * 256 + l;
                double mv[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) mv[s] = mBp[s * 64];
                d4 T1 = {0, 0, 0, 0};
#pragma unroll
                for (int s = 0; s < 4; ++s) T1 = CBF_MFMA(mv[s], fmB[s], T1);
                d4 a2bar;
#pragma unroll
                for (int r = 0; r < 4; ++r) a2bar[r] = T1[r] + 2.0 * sq[i][r] - kreg[i][r] * fvsum;
                // 16x16 transposes through this wave's own rows of the A2bar tile (nobody else reads them before the
                // next barrier): C-layout (row g+4r, col nl) -> A-operand layout (row nl, k = 4s+g)
                double a2T[4], abT[4];
                double* own = A2t + 16 * rbs[i] * PD;
#pragma unroll
                for (int s = 0; s < 4; ++s) a2T[s] = own[nl * PD + 4 * s + g];     // (phase D' left A2 in these rows)
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int r = 0; r < 4; ++r) own[(g + 4 * r) * PD + nl] = a2bar[r];      // stays: A2bar tile of phase F
#pragma unroll
                for (int s = 0; s < 4; ++s) gMu[i] = CBF_MFMA(a2T[s], fmT[s], gMu[i]);   // mubar[m][d] += A2[m][n] Fm[d][n]
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int s = 0; s < 4; ++s) abT[s] = own[nl * PD + 4 * s + g];
                if constexpr (STASH) {
                    // A2bar^T and K^T of this row block as the MFMA operand images of Kinvbar += A2bar K^T
                    double* pa = a.stash_a + (cb * NBLK + rbs[i]) * 256 + l;
                    double* pk = a.stash_k + (cb * NBLK + rbs[i]) * 256 + l;
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
                            gB[i][c2] = CBF_MFMA(abT[s], kT, gB[i][c2]);        // Kinvbar[m'][m] += A2bar[m'][n] K[m][n]
                        }
                    }
                }
            }
        }
        __syncthreads();

        // ---- F: Kbar, Ebar, input adjoint partials, Zbar~
        d4 ebar[RB];
        {
            d4 acc[RB][2];
#pragma unroll
            for (int i = 0; i < RB; ++i) { acc[i][0] = d4{0, 0, 0, 0}; acc[i][1] = d4{0, 0, 0, 0}; }
#pragma unroll 1
            for (int s0 = 0; s0 < KSr; s0 += 4) {
                double b[4], aop[RB][4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
#pragma unroll
                    for (int i = 0; i < RB; ++i) aop[i][j] = bop[i][(s0 + j) * 64];
                    b[j] = A2t[(4 * (s0 + j) + g) * PD + nl];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int i = 0; i < RB; ++i)
                        if (ok[i]) acc[i][j & 1] = CBF_MFMA(aop[i][j], b[j], acc[i][j & 1]);
            }
#pragma unroll
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double v = (acc[i][0][r] + acc[i][1][r] - a2[i][r] * fvsum) * kreg[i][r];
                    ebar[i][r] = (ok[i] && 16 * rbs[i] + 4 * r + g < M) ? v : 0.0;
                }
        }
        {
            d4 xp[JB];
#pragma unroll
            for (int jb = 0; jb < JB; ++jb) xp[jb] = d4{0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                if (ok[i]) {
                    const double* ZTp = a.rk.ZT + rbs[i] * JB * 256 + l;
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
                double* ownk = Kt + 16 * rbs[i] * PD;    // the K tile is dead behind the barrier that ends phase E
#pragma unroll
                for (int r = 0; r < 4; ++r) ownk[(g + 4 * r) * PD + nl] = ebar[i][r];
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int s = 0; s < 4; ++s) ebT[s] = ownk[nl * PD + 4 * s + g];
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
        __syncthreads();

        // ---- G: input adjoint of this block's points
        {
            const bool pvalid = (p0 + nl) < a.npts;
            double esum = 0.0;                          // colsum of Ebar for this lane's point = row D of the xbar tile
            const int jbD = D >> 4, qD = (D >> 2) & 3, gD = D & 3;
#pragma unroll
            for (int ww = 0; ww < W; ++ww) esum += part[ww * PSL + (jbD * 4 + qD) * 64 + gD * 16 + nl];
#pragma unroll
            for (int k2 = 0; k2 < GPW; ++k2) {
                const int gi = w + k2 * W;
                if (gi < NG) {
                    const int j = 4 * gi + g;
                    double xb = 0.0;
#pragma unroll
                    for (int ww = 0; ww < W; ++ww) xb += part[ww * PSL + gi * 64 + l];
                    if (j < D && pvalid) {
                        const double xt = xq[j * PD + nl];
                        xb -= xt * esum;
                        glx[k2] += xb * xt;                                        // lengthscale adjoint (inputs)
                        a.gX[(p0 + nl) * D + j] = xb * ilg[k2];
                    }
                    if (j == D && pvalid) glogsig += xb;
                }
            }
        }
    }

    // ---- write this workgroup's slab
    __syncthreads();
    double* slab = a.gpart + int64_t(blockIdx.x) * a.slab;
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        if (ok[i]) {
            const int rb = rbs[i];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                slab[SL::gMu + rb * 256 + r * 64 + l] = gMu[i][r];
                slab[SL::gS2 + rb * 256 + r * 64 + l] = 0.0;        // (no diagonal sigma_z^2 in the full form)
                if constexpr (!STASH) {
#pragma unroll
                    for (int c2 = 0; c2 < NCB; ++c2) slab[SL::gB + (rb * NBLK + c2) * 256 + r * 64 + l] = gB[i][c2][r];
                }
#pragma unroll
                for (int jb = 0; jb < JB; ++jb) slab[SL::gZ + (rb * JB + jb) * 256 + r * 64 + l] = gZ[i][jb][r];
            }
        }
    }
    for (int i = tid; i < 192; i += NT) slab[SL::small + i] = 0.0;
    __syncthreads();
#pragma unroll
    for (int k2 = 0; k2 < GPW; ++k2) {
        const int gi = w + k2 * W;
        double v = glx[k2];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (gi < NG && nl == 0) slab[SL::small + 32 + 4 * gi + g] = v;
    }
    const double s1 = block_sum(gsig, red, tid, NT);
    const double s2 = block_sum(glogsig, red, tid, NT);
    if (tid == 0) {
        slab[SL::small + 96] = s1;
        slab[SL::small + 97] = s2;
    }
}

template <int NBLK, int DK>
int launch_gp_fq_k(const GpFqArgs& a, unsigned nwg, hipStream_t st)
{
    typedef GpBwdCfg<NBLK> C;
    typedef GpFqGeom<NBLK, DK> G;
    const size_t lds = size_t(G::LDS_DOUBLES) * sizeof(double);
    auto k = gp_fullq_bwd_kernel<NBLK, C::RB, DK, C::STASH>;
    int rc = set_lds(k, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k, dim3(nwg), dim3(64 * C::W), lds, st, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -int(e) - 1000;
}

template <int NBLK>
int launch_gp_fq_n(int DK, const GpFqArgs& a, unsigned nwg, hipStream_t st)
{
    switch (DK) {
        case 2: return launch_gp_fq_k<NBLK, 2>(a, nwg, st);
        case 4: return launch_gp_fq_k<NBLK, 4>(a, nwg, st);
        case 6: return launch_gp_fq_k<NBLK, 6>(a, nwg, st);
    }
    return -2;
}

// ---- the forward on the MFMA units (gp_tf.py:76-98 with q_sqrt.ndims == 3) ----------------------------------------------
//
// Per 16-point block: the kernel tile (phase B of the adjoint), A2 in the form layout->gp_form asks for -- dense: K^-1 k,
// fvar0 = sigma^2 - sum_m k a2; two-triangular (gp_tf.py:137-145): A = L^-1 k, fvar0 = sigma^2 - sum_m A^2, A2 = L^-T A --
// then per output dimension the rows of S_d A2 (S_d streamed from L2 like K^-1) and the column reduction
// sum_m a2[m][n] (S_d A2)[m][n] into fvar: per-wave partials over the wave's rows, summed over the waves in a fixed order.
// fmean = mu^T A2 comes from the same A2 tile on the last wave.  Rows m >= M are zero in every operand image and points
// >= npts are computed on zero inputs and never written.  Only the lower triangle of q_sqrt enters (through S_d).
struct GpFqFwdArgs {
    PackPtrs pk;
    const double* X;       // (npts, D)
    const double* Sp;      // [Do][NBLK][KS][64]
    double* fmean;         // (npts, Do)
    double* fvar;          // (npts, Do)
    int64_t npts;
    int64_t nblocks;
    int M, D, Do, tri;
};

template <int NBLK, int DK>
struct GpFqFwdGeom {
    typedef GpBwdCfg<NBLK> C;
    static constexpr int PD = 17;
    static constexpr int LDS_DOUBLES = 4 * DK * PD + 2 * (16 * NBLK) * PD + C::W * 17 * 16;
    static_assert(LDS_DOUBLES <= 163840 / 8, "LDS budget");
};

// out[i] = (rows of the A-operand image behind aop[i]) x (the [16 NBLK][17] tile in LDS); four k-steps of loads together
template <int RB>
__device__ __forceinline__ void fq_image_times_tile(const double* const (&aop)[RB], const bool (&ok)[RB], const double* tile,
                                                    int KSr, int g, int nl, d4 (&out)[RB])
{
    constexpr int PD = 17;
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
    for (int i = 0; i < RB; ++i) out[i] = acc[i][0] + acc[i][1];
}

template <int NBLK, int RB, int DK>
__global__ __launch_bounds__(64 * ((NBLK + RB - 1) / RB)) void gp_fullq_fwd_kernel(GpFqFwdArgs a)
{
    constexpr int W = (NBLK + RB - 1) / RB, NT = 64 * W, MP = 16 * NBLK, KS = MP / 4;
    constexpr int PD = 17;

    extern __shared__ double lds[];
    double* xq = lds;                                   // [4 DK][17] scaled inputs x~[j][n]
    double* Kt = xq + 4 * DK * PD;                      // [MP][17]  kernel tile
    double* A2t = Kt + MP * PD;                         // [MP][17]  A (two-triangular form), then A2
    double* red = A2t + MP * PD;                        // [W][17][16] per-wave column partials: slot d < Do, slot 16 = fvar0

    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, g = l >> 4, nl = l & 15;
    const int M = a.M, D = a.D, Do = a.Do;
    const int KSr = a.pk.KSr;
    const double sig2 = a.pk.scal[CBFSSM_SCAL_SIGMA2];

    bool ok[RB];
    int rbs[RB];
    double Zreg[RB][DK], czr[RB][4];
    const double *bop[RB], *wop[RB], *wtop[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        ok[i] = (w * RB + i) < NBLK;
        rbs[i] = ok[i] ? (w * RB + i) : (NBLK - 1);
#pragma unroll
        for (int s = 0; s < DK; ++s) Zreg[i][s] = a.pk.Zp[(rbs[i] * DK + s) * 64 + l];
#pragma unroll
        for (int r = 0; r < 4; ++r) czr[i][r] = a.pk.cz[16 * rbs[i] + 4 * r + g];
        bop[i] = a.pk.Bp + rbs[i] * KS * 64 + l;
        wop[i] = a.pk.Wp + rbs[i] * KS * 64 + l;
        wtop[i] = a.pk.WTp + rbs[i] * KS * 64 + l;
    }

    for (int64_t cb = blockIdx.x; cb < a.nblocks; cb += gridDim.x) {
        const int64_t p0 = cb * 16;
        __syncthreads();                                // the previous block's readers of xq / A2t / red are done
        for (int i = tid; i < 4 * DK * 16; i += NT) {
            const int j = i >> 4, n = i & 15;
            const int64_t p = p0 + n;
            double v = 0.0;
            if (j < D && p < a.npts) v = a.X[p * D + j] * a.pk.invl[j];
            xq[j * PD + n] = v;
        }
        __syncthreads();

        // ---- kernel tile (rows of this wave); rows m >= M are exactly zero
        d4 kreg[RB];
        {
            double bx[DK], xx = 0.0;
#pragma unroll
            for (int s = 0; s < DK; ++s) {
                bx[s] = xq[(4 * s + g) * PD + nl];
                xx = fma(bx[s], bx[s], xx);
            }
            xx += __shfl_xor(xx, 16);
            xx += __shfl_xor(xx, 32);
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
        __syncthreads();

        // ---- A2 of this wave's rows and this wave's part of sigma^2 - fvar0
        d4 a2[RB];
        double v0 = 0.0;
        if (a.tri) {
            d4 A[RB];
            fq_image_times_tile<RB>(wop, ok, Kt, KSr, g, nl, A);
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
            fq_image_times_tile<RB>(wtop, ok, A2t, KSr, g, nl, a2);
            __syncthreads();                            // every wave has read A before A2 takes its place
        } else {
            fq_image_times_tile<RB>(bop, ok, Kt, KSr, g, nl, a2);
#pragma unroll
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) v0 = fma(kreg[i][r], a2[i][r], v0);
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            if (ok[i]) {
#pragma unroll
                for (int r = 0; r < 4; ++r) A2t[(16 * rbs[i] + g + 4 * r) * PD + nl] = a2[i][r];
            }
        }
        v0 += __shfl_xor(v0, 16);
        v0 += __shfl_xor(v0, 32);
        if (g == 0) red[(w * 17 + 16) * 16 + nl] = v0;
        __syncthreads();

        // ---- per output dimension: rows of S_d A2, then sum_m a2 (S_d A2) over this wave's rows
#pragma unroll 1
        for (int d = 0; d < Do; ++d) {
            const double* sop[RB];
#pragma unroll
            for (int i = 0; i < RB; ++i) sop[i] = a.Sp + (int64_t(d) * NBLK + rbs[i]) * KS * 64 + l;
            d4 sa[RB];
            fq_image_times_tile<RB>(sop, ok, A2t, KSr, g, nl, sa);
            double v = 0.0;
#pragma unroll
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) v = fma(a2[i][r], sa[i][r], v);
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if (g == 0) red[(w * 17 + d) * 16 + nl] = v;
        }

        // ---- fmean^T = mu^T A2 on the last wave: the pack's mean image read as an A operand (row d, k = m)
        if (w == W - 1) {
            d4 fm[2] = {d4{0, 0, 0, 0}, d4{0, 0, 0, 0}};
#pragma unroll 1
            for (int s = 0; s < KSr; ++s) fm[s & 1] = CBF_MFMA(a.pk.muA[s * 64 + l], A2t[(4 * s + g) * PD + nl], fm[s & 1]);
            const int64_t p = p0 + nl;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int d = g + 4 * r;
                if (d < Do && p < a.npts) a.fmean[p * Do + d] = fm[0][r] + fm[1][r];
            }
        }
        __syncthreads();
        for (int i = tid; i < 16 * Do; i += NT) {
            const int n = i / Do, d = i - n * Do;
            const int64_t p = p0 + n;
            double s0 = 0.0, s1 = 0.0;
            for (int ww = 0; ww < W; ++ww) {            // fixed order: deterministic
                s0 += red[(ww * 17 + 16) * 16 + n];
                s1 += red[(ww * 17 + d) * 16 + n];
            }
            if (p < a.npts) a.fvar[p * Do + d] = (sig2 - s0) + s1;
        }
    }
}

template <int NBLK, int DK>
int launch_gp_fq_fwd_k(const GpFqFwdArgs& a, unsigned nwg, hipStream_t st)
{
    typedef GpBwdCfg<NBLK> C;
    const size_t lds = size_t(GpFqFwdGeom<NBLK, DK>::LDS_DOUBLES) * sizeof(double);
    auto k = gp_fullq_fwd_kernel<NBLK, C::RB, DK>;
    int rc = set_lds(k, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k, dim3(nwg), dim3(64 * C::W), lds, st, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -int(e) - 1000;
}

template <int NBLK>
int launch_gp_fq_fwd_n(int DK, const GpFqFwdArgs& a, unsigned nwg, hipStream_t st)
{
    switch (DK) {
        case 2: return launch_gp_fq_fwd_k<NBLK, 2>(a, nwg, st);
        case 4: return launch_gp_fq_fwd_k<NBLK, 4>(a, nwg, st);
        case 6: return launch_gp_fq_fwd_k<NBLK, 6>(a, nwg, st);
    }
    return -2;
}

}  // namespace cbfssm

#define CBF_GPFQ_DECLARE(NB)                                                                    \
    namespace cbfssm {                                                                           \
    int launch_gp_fq_nb##NB(int DK, const GpFqArgs& a, unsigned nwg, hipStream_t st);          \
    int launch_gp_fq_fwd_nb##NB(int DK, const GpFqFwdArgs& a, unsigned nwg, hipStream_t st);   \
    }

#define CBF_GPFQ_INSTANTIATE(NB)                                                                \
    namespace cbfssm {                                                                           \
    int launch_gp_fq_nb##NB(int DK, const GpFqArgs& a, unsigned nwg, hipStream_t st)           \
    {                                                                                            \
        return launch_gp_fq_n<NB>(DK, a, nwg, st);                                              \
    }                                                                                            \
    int launch_gp_fq_fwd_nb##NB(int DK, const GpFqFwdArgs& a, unsigned nwg, hipStream_t st)    \
    {                                                                                            \
        return launch_gp_fq_fwd_n<NB>(DK, a, nwg, st);                                          \
    }                                                                                            \
    }

