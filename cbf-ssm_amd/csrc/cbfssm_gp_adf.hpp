// Assumed-density (moment-matching) Kalman filter over the transition of one sparse GP: the recursion of gp_ekf_kernel
// (cbfssm_gp_ekf.hpp) with the linearisation at the mean replaced by the exact first and second moments of the GP under the
// Gaussian belief (cbfssm_gp_mm.hpp) -- GP-ADF, PILCO's propagation -- as ONE launch for all T steps.  Per chain n:
//
//   x = concat(m, a[t]);  S = blockdiag(P, 0)                     (the auxiliary input is known)
//   fmean, fcov, xcov = moment_match(x, S);  Cx = xcov[:, :Do]    (Cx[d][i] = Cov(f_d, h_i))
//   m- = m + fmean;  cross[t] = P + Cx;  P- = P + (Cx + Cx^T) + fcov + diag(var_x)
//   pmeans[t], pcovs[t] = m-, P-
//   where cond[t, n] != 0, for j = 0 .. Dy - 1: the scalar updates of gp_ekf_kernel's C3, expression for expression
//   means[t], covs[t] = m, P = m-, P-
//
// One workgroup owns 16 chains for all T steps (grid = ceil(N / 16), GpBwdCfg<NBLK>'s waves).  A step is
//
//   G  the GP part: steps 0 to 4 of gp_moment_match_kernel as a copy, the 16 chains two at a time.  The input mean and
//      covariance are the belief, read from where the workgroup itself wrote it one step earlier (means[t-1], covs[t-1];
//      m0, P0 at t = 0) behind a workgroup barrier, padded with a[t] and the zero block exactly as
//      GPModel.transition_moments pads them: the general-D factorisations, no Do x Do shortcut.  fmean, fcov and the state
//      columns of xcov of a pair go to pmeans[t], pcovs[t], cross[t], which are outputs anyway.
//   U  after the eighth pair one update phase over all 16 chains, one lane per (chain n, row i) as gp_ekf_kernel's C2 / C3:
//      the lane reads fmean[i], row i of fcov, row i and column i of Cx and row i of P back, forms row i of cross and of
//      P- in registers -- P[i][q] + (Cx[i][q] + Cx[q][i]) + fcov[i][q]: the same expression at [q][i], P and fcov being
//      bitwise symmetric, so P- is bitwise symmetric without a mirror store -- and overwrites the three slots with m-,
//      P- and cross.  C3 runs on a [16][16][17] tile that lies over the U images / slots of the GP part (dead behind a
//      barrier), so the belief needs no LDS of its own: the kernel fits at 20 row blocks / DK 6 where GpMmGeom leaves 1 664 B.
//
// info[n] = 0, or t + 1 of the first step at which a factorisation of chain n met a pivot <= 0, not finite, or below what a
// positive semi-definite belief can give (1 for I + S~, 1 / 2 for I / 2 + S~, less rounding: this is what catches a negative
// definite P0 with entries below the squared lengthscales, whose two factors exist) -- possible only when P0 is not
// positive semi-definite: from that step on every result of the chain, and its loglik, is NaN.  The chain's arithmetic
// touches no other chain's.  No atomics, no spin wait, workgroup barriers only; every output entry has one last writer, two
// calls are bitwise identical, and a chain's results do not depend on the other chains of the call.  Rows m >= M of Q are
// zero; chains >= N are computed on zero inputs in G, repeat chain N - 1 in U, and store nothing.  A y entry at cond = 0 is
// chosen away by a select and may be NaN.
#pragma once
#include "../../include/cbfssm_hip.h"
#include "cbfssm_gp_bwd.hpp"

namespace cbfssm {

struct GpAdfArgs {
    const double* Zp;      // [NBLK][DK][64]     Z~ as A-operand image
    const double* cz;      // [16 NBLK]          -|z~|^2 / 2 + log v (padding rows: -1e30)
    const double* invl;    // [4 DK]             1 / lengthscale, zero padded
    const double* scal;
    const double* Zs;      // [M][D]             Z~
    const double* ZT;      // [NBLK][JB][4][64]  (Z~)^T as A-operand image, row D = ones
    const double* alpha;   // [16][16 NBLK]      (K^-1 mu)[m][d] at [d][m], zero padded (gp_lin_alpha_kernel)
    const double* Wimg;    // [Do][NBLK][NBLK][4][64]  W_d tiles in the accumulator layout, zero padded (gp_mm_w_kernel)
    const double* m0;      // (N, Do)
    const double* P0;      // (N, Do, Do), lower triangle read, or null: zero
    const double* a;       // (T, N, D - Do) (unused when D == Do)
    const double* y;       // (T, N, Dy): entries at cond = 0 are never used (they may be NaN)
    const double* cond;    // (T, N) 0 / 1, or null: condition everywhere
    const double* var_x;   // (Do) or null
    const double* var_y;   // (Dy)
    double* means;         // (T, N, Do)
    double* covs;          // (T, N, Do, Do)
    double* loglik;        // (N)
    double* pmeans;        // (T, N, Do)      m- of every step, before conditioning (within a step first: fmean)
    double* pcovs;         // (T, N, Do, Do)  P- of every step                      (within a step first: fcov)
    double* cross;         // (T, N, Do, Do)  P + Cx = Cov(h_t, h_{t-1})            (within a step first: Cx)
    double* info;          // (N)  0, or t + 1 of the first failed factorisation
    int N, T, M, D, Do, Dy;
};

// LDS: region A | region B, as GpMmGeom.  Region A holds the U images and L2 in steps 0 to 2, the waves' slots in steps 3
// and 4, and the covariance tile [16][16][17] of the update phase.  Region B: GpMmGeom's, and the 16 chains' info.
template <int NBLK, int DK>
struct GpAdfGeom {
    typedef GpBwdCfg<NBLK> C;
    static constexpr int PG = 2;
    static constexpr int DP = 4 * DK;
    static constexpr int MP = 16 * NBLK;
    static constexpr int JB = (4 * DK + 1 + 15) / 16;
    static constexpr int UOP = NBLK * DK * 64;
    static constexpr int LT = DP * DP;
    static constexpr int SLOT = 272 + JB * 256 + 16;
    static constexpr int PD = 17;
    static constexpr int CT = 16 * 16 * PD;
    static constexpr int RA0 = PG * UOP + PG * LT;
    static constexpr int RA1 = C::W * PG * SLOT;
    static constexpr int RA01 = RA0 > RA1 ? RA0 : RA1;
    static constexpr int RA = RA01 > CT ? RA01 : CT;
    static constexpr int RBD = 2 * PG * LT + 3 * PG * DP + 2 * PG * MP + 4 * PG + DP + 16;
    static constexpr int LDS_DOUBLES = RA + RBD;
    static_assert(LDS_DOUBLES <= 163840 / 8, "LDS budget");
};

__device__ __forceinline__ int adf_cidx(int row, int col) { return (row >> 2) * 64 + (row & 3) * 16 + col; }

// per (chain, row) lane of the update phase: what it carries from step to step
struct AdfLane {
    double m, lin;
    LogProd lp;
};

template <int NBLK, int RB, int DK>
__global__ __launch_bounds__(64 * ((NBLK + RB - 1) / RB)) void gp_adf_kernel(GpAdfArgs a)
{
    typedef GpAdfGeom<NBLK, DK> G;
    constexpr int W = (NBLK + RB - 1) / RB, NT = 64 * W, MP = G::MP, DP = G::DP, JB = G::JB, PG = G::PG, PD = G::PD;
    constexpr int UOP = G::UOP, LT = G::LT, SLOT = G::SLOT, H = NBLK / 2;
    constexpr int MOFF = 272, TOFF = 272 + JB * 256;
    constexpr int TPT = (256 + NT - 1) / NT;            // (chain, row) lanes per thread: 4, 2 or 1

    extern __shared__ double lds[];
    double* Uop = lds;                                  // [PG][NBLK][DK][64]
    double* L2t = Uop + PG * UOP;                       // [PG][DP][DP]
    double* slot = lds;                                 // [W][PG][SLOT], over the two above
    double* Pt = lds;                                   // [16][16][17]  P-[n][i][k] of the update phase, over all of those
    double* L1t = lds + G::RA;                          // [PG][DP][DP]
    double* Sg = L1t + PG * LT;                         // [PG][DP][DP]  S~, both triangles
    double* inv1 = Sg + PG * LT;                        // [PG][DP]
    double* inv2 = inv1 + PG * DP;                      // [PG][DP]
    double* mt = inv2 + PG * DP;                        // [PG][DP]      m~
    double* qv = mt + PG * DP;                          // [PG][MP]
    double* gv = qv + PG * MP;                          // [PG][MP]
    double* cst = gv + PG * MP;                         // [PG][4]       c1, log c2, info of factor 1, of factor 2
    double* il = cst + 4 * PG;                          // [DP]
    double* binfo = il + DP;                            // [16]          info of the 16 chains

    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, g = l >> 4, nl = l & 15;
    const int M = a.M, D = a.D, Do = a.Do, Dy = a.Dy, N = a.N, T = a.T;
    const int naux = D - Do;
    const int c0 = blockIdx.x * 16;
    const double sig2 = a.scal[CBFSSM_SCAL_SIGMA2];
    const double logv = log(sig2);
    const double nan = __builtin_nan("");
    const int64_t DD = int64_t(Do) * Do;

    bool ok[RB];
    int rbs[RB];
    double alj[RB][4], czj[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        ok[i] = (w * RB + i) < NBLK;
        rbs[i] = ok[i] ? (w * RB + i) : (NBLK - 1);
#pragma unroll
        for (int r = 0; r < 4; ++r) alj[i][r] = a.alpha[nl * MP + 16 * rbs[i] + 4 * r + g];
        czj[i] = 0.5 * (a.cz[16 * rbs[i] + nl] - logv);
    }
    for (int i = tid; i < DP; i += NT) il[i] = a.invl[i];           // (made visible by the barrier of the first pair)
    if (tid < 16) binfo[tid] = 0.0;

    // ---- the (chain, row) lanes of the update phase: lane id = 16 n + i, the 16 rows of a chain side by side in a wave
    AdfLane ln[TPT];
    int lc[TPT];                                        // chain of the call (clamped), for loads and stores
    double lvx[TPT];
#pragma unroll
    for (int k2 = 0; k2 < TPT; ++k2) {
        const int id = tid + k2 * NT, n = (id >> 4) & 15, i = id & 15;
        const bool act = (id < 256) && (i < Do);
        const int ic = act ? i : 0;
        lc[k2] = min(c0 + n, N - 1);
        lvx[k2] = (act && a.var_x) ? a.var_x[ic] : 0.0;
        ln[k2].m = act ? a.m0[int64_t(lc[k2]) * Do + ic] : 0.0;
        ln[k2].lin = 0.0;
        ln[k2].lp.init();
    }

    for (int t = 0; t < T; ++t) {
        // the belief of this step: what this workgroup stored one step earlier (visible behind the barrier below)
        const double* mprev = t > 0 ? a.means + int64_t(t - 1) * N * Do : a.m0;
        const double* Pprev = t > 0 ? a.covs + int64_t(t - 1) * N * DD : a.P0;
        const int64_t tN = int64_t(t) * N;

        // this step's observation and mask, issued ahead of the GP work
        double yv[TPT], cnd[TPT];
#pragma unroll
        for (int k2 = 0; k2 < TPT; ++k2) {
            const int i = (tid + k2 * NT) & 15;
            const int64_t tc = tN + lc[k2];
            yv[k2] = a.y[tc * Dy + (i < Dy ? i : 0)];
            cnd[k2] = a.cond ? a.cond[tc] : 1.0;
        }

        // ==== G: the moments of the GP under the belief, two chains at a time
        for (int pgi = 0; pgi < 16 / PG; ++pgi) {
            const int pbase = c0 + pgi * PG;
            if (pbase >= N) break;
            __syncthreads();                            // the previous pair's readers of the slots and of region B, and the
                                                        // previous step's update phase (tile, means, covs), are done

            // ---- 0: m~, and the two factorisations of a chain on one wave
            for (int i = tid; i < PG * DP; i += NT) {
                const int pp = i / DP, k = i - pp * DP;
                const int p = pbase + pp;
                double v = 0.0;
                if (p < N) {
                    if (k < Do) v = mprev[int64_t(p) * Do + k] * il[k];
                    else if (k < D) v = a.a[(tN + p) * naux + (k - Do)] * il[k];
                }
                mt[i] = v;
            }
            for (int pp = w; pp < PG; pp += W) {
                const int hh = l >> 5, i = l & 31;
                const int p = pbase + pp;
                const bool have = Pprev != nullptr && p < N && i < Do;       // S = blockdiag(P, 0)
                const double ili = (i < D) ? a.invl[i] : 0.0;
                double arow[DP];
#pragma unroll
                for (int j = 0; j < DP; ++j) {
                    double s = 0.0;
                    if (have && j <= i) s = Pprev[(int64_t(p) * Do + i) * Do + j] * ili * a.invl[j];
                    if (hh == 0 && i < DP && j <= i) {
                        Sg[pp * LT + i * DP + j] = s;
                        Sg[pp * LT + j * DP + i] = s;
                    }
                    arow[j] = s + ((j == i) ? (hh ? 0.5 : 1.0) : 0.0);
                }
                double prod = 1.0;
                bool bad = false;
                double* invd = (hh ? inv2 : inv1) + pp * DP;
                // column k of the trailing matrix goes round through LDS (the U image's place, free until step 1)
                double* colb = Uop + (pp * 2 + hh) * 32;
#pragma unroll
                for (int k = 0; k < DP; ++k) {
                    if (k < D) {
                        colb[i] = arow[k];
                        __builtin_amdgcn_wave_barrier();
                        double col[DP];
#pragma unroll
                        for (int j = k; j < DP; ++j) col[j] = colb[j];
                        __builtin_amdgcn_wave_barrier();
                        double akk = col[k];
                        // the pivots of I + S~ are >= 1 and those of I / 2 + S~ >= 1 / 2 whenever S is positive
                        // semi-definite (their Schur complements dominate those of the identity part): one below that floor
                        // by more than rounding proves that S is not, as a pivot <= 0 does
                        const double flo = hh ? 0.5 : 1.0, skk = Sg[pp * LT + k * DP + k];
                        if (!(akk > 0.0) || !(akk < __builtin_inf()) || akk < flo - 1e-10 * (flo + fabs(skk))) {
                            bad = true;
                            akk = 1.0;
                        }
                        const double inv = fast_rsqrt(akk), dd = akk * inv;
                        prod *= dd;
                        const double lik = (i == k) ? dd : ((i > k) ? arow[k] * inv : 0.0);
                        arow[k] = lik;
                        if (i == k) invd[k] = inv;
#pragma unroll
                        for (int j = k + 1; j < DP; ++j)
                            if (i >= j) arow[j] = fma(-lik, col[j] * inv, arow[j]);
                    }
                }
                if (i < DP) {
                    double* Lo = (hh ? L2t : L1t) + pp * LT + i;          // column by column: L[i][j] at [j][i]
#pragma unroll
                    for (int j = 0; j < DP; ++j) Lo[j * DP] = (j < i) ? arow[j] : 0.0;
                }
                if (i == 0) {
                    if (hh == 0) {
                        cst[pp * 4 + 0] = sig2 / prod;
                        cst[pp * 4 + 2] = bad ? 1.0 : 0.0;
                    } else {
                        cst[pp * 4 + 1] = 2.0 * logv - 0.34657359027997264 * double(D) - log(prod);
                        cst[pp * 4 + 3] = bad ? 2.0 : 0.0;
                    }
                }
            }
            __syncthreads();

            // ---- 1: w_i, u_i by forward substitution, q_i, g_i, the U image
            for (int it = tid; it < PG * MP; it += NT) {
                const int pp = it / MP, m = it - pp * MP;
                const double* L1 = L1t + pp * LT;
                const double* L2 = L2t + pp * LT;
                double r[DP], u[DP];
#pragma unroll
                for (int k = 0; k < DP; ++k) r[k] = (m < M && k < D) ? a.Zs[m * D + k] - mt[pp * DP + k] : 0.0;
                double ss = 0.0;
#pragma unroll
                for (int i = 0; i < DP; ++i) u[i] = r[i];
#pragma unroll
                for (int j = 0; j < DP; ++j) {
                    if (j < D) {
                        u[j] *= inv1[pp * DP + j];
#pragma unroll
                        for (int i = j + 1; i < DP; ++i) u[i] = fma(-L1[j * DP + i], u[j], u[i]);
                        ss = fma(u[j], u[j], ss);
                    }
                }
                qv[it] = (m < M) ? cst[pp * 4 + 0] * tile_exp(-0.5 * ss) : 0.0;
                ss = 0.0;
#pragma unroll
                for (int i = 0; i < DP; ++i) u[i] = r[i];
#pragma unroll
                for (int j = 0; j < DP; ++j) {
                    if (j < D) {
                        u[j] *= inv2[pp * DP + j];
#pragma unroll
                        for (int i = j + 1; i < DP; ++i) u[i] = fma(-L2[j * DP + i], u[j], u[i]);
                        ss = fma(u[j], u[j], ss);
                    }
                }
                gv[it] = ss;
                double* Uo = Uop + pp * UOP + (m >> 4) * DK * 64 + (m & 15);
#pragma unroll
                for (int k = 0; k < DP; ++k) Uo[(k >> 2) * 64 + (k & 3) * 16] = u[k];
            }
            __syncthreads();

            // ---- 2: the tiles of Q of this wave's column blocks, and the mean part of its rows
            d4 Racc[RB][PG], macc[PG][JB];
            double tr[PG][16];
#pragma unroll
            for (int pp = 0; pp < PG; ++pp) {
#pragma unroll
                for (int i = 0; i < RB; ++i) Racc[i][pp] = d4{0, 0, 0, 0};
#pragma unroll
                for (int jb = 0; jb < JB; ++jb) macc[pp][jb] = d4{0, 0, 0, 0};
#pragma unroll
                for (int d = 0; d < 16; ++d) tr[pp][d] = 0.0;
            }
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                if (ok[i]) {
                    const int jb = rbs[i];
                    const bool colok = (16 * jb + nl) < M;
                    double Uj[PG][DK], Zj[DK], gj[PG], lc2[PG];
#pragma unroll
                    for (int s = 0; s < DK; ++s) Zj[s] = 0.5 * a.Zp[(jb * DK + s) * 64 + l];
#pragma unroll
                    for (int pp = 0; pp < PG; ++pp) {
#pragma unroll
                        for (int s = 0; s < DK; ++s) Uj[pp][s] = Uop[pp * UOP + (jb * DK + s) * 64 + l];
                        gj[pp] = gv[pp * MP + 16 * jb + nl];
                        lc2[pp] = cst[pp * 4 + 1];
                    }
#pragma unroll 1
                    for (int o = 0; o <= H; ++o) {
                        int ib = jb + o;
                        if (ib >= NBLK) ib -= NBLK;
                        const double wgt = (o == 0 || 2 * o == NBLK) ? 0.5 : 1.0;
                        d4 zz;
                        double ali[4];
                        bool rowok[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = 16 * ib + 4 * r + g;
                            zz[r] = 0.5 * (a.cz[row] - logv) + czj[i];
                            ali[r] = a.alpha[nl * MP + row];
                            rowok[r] = colok && row < M;
                        }
#pragma unroll
                        for (int s = 0; s < DK; ++s) zz = CBF_MFMA(a.Zp[(ib * DK + s) * 64 + l], Zj[s], zz);
                        d4 Q[PG];
#pragma unroll
                        for (int pp = 0; pp < PG; ++pp) {
                            d4 acc = {0, 0, 0, 0};
                            const double* Ui = Uop + pp * UOP + ib * DK * 64 + l;
#pragma unroll
                            for (int s = 0; s < DK; ++s) acc = CBF_MFMA(Ui[s * 64], Uj[pp][s], acc);
                            d4 e;
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                e[r] = zz[r] - 0.125 * (gv[pp * MP + 16 * ib + 4 * r + g] + gj[pp]) - 0.25 * acc[r] + lc2[pp];
                            e = tile_exp4(e);
#pragma unroll
                            for (int r = 0; r < 4; ++r) Q[pp][r] = rowok[r] ? e[r] * wgt : 0.0;
#pragma unroll
                            for (int r = 0; r < 4; ++r) Racc[i][pp] = CBF_MFMA(ali[r], Q[pp][r], Racc[i][pp]);
                        }
                        const double* Wt = a.Wimg + (int64_t(ib) * NBLK + jb) * 256 + l;
#pragma unroll
                        for (int d = 0; d < 16; ++d) {
                            if (d < Do) {
                                const double* Wd = Wt + int64_t(d) * NBLK * NBLK * 256;
                                double wv[4];
#pragma unroll
                                for (int r = 0; r < 4; ++r) wv[r] = Wd[r * 64];
#pragma unroll
                                for (int pp = 0; pp < PG; ++pp)
#pragma unroll
                                    for (int r = 0; r < 4; ++r) tr[pp][d] = fma(wv[r], Q[pp][r], tr[pp][d]);
                            }
                        }
                    }
                    // the mean part of row block jb: B[k = m][col = input index] = q_m (z~_m - m~), ones row: q_m
                    const double* ZTp = a.ZT + jb * JB * 256 + l;
#pragma unroll
                    for (int pp = 0; pp < PG; ++pp) {
                        double q4[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) q4[r] = qv[pp * MP + 16 * jb + 4 * r + g];
#pragma unroll
                        for (int j2 = 0; j2 < JB; ++j2) {
                            const int col = 16 * j2 + nl;
                            const double mtv = (col < D) ? mt[pp * DP + col] : 0.0;
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                macc[pp][j2] = CBF_MFMA(alj[i][r], q4[r] * (ZTp[(j2 * 4 + r) * 64] - mtv), macc[pp][j2]);
                        }
                    }
                }
            }
#pragma unroll
            for (int pp = 0; pp < PG; ++pp) {
#pragma unroll
                for (int d = 0; d < 16; ++d) {
                    if (d < Do) {
                        double s = tr[pp][d];
#pragma unroll
                        for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o);
                        tr[pp][d] = s;
                    }
                }
            }
            __syncthreads();                            // every wave is done with the U images and L2: the slots are free

            // ---- 3: X = R_jb alpha_jb of this wave's column blocks; this wave's slots
#pragma unroll
            for (int pp = 0; pp < PG; ++pp) {
                double* sl = slot + (w * PG + pp) * SLOT;
                d4 X = {0, 0, 0, 0};
#pragma unroll
                for (int i = 0; i < RB; ++i) {
                    if (ok[i]) {
                        double rT[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) sl[(4 * r + g) * 17 + nl] = Racc[i][pp][r];
                        __builtin_amdgcn_wave_barrier();
#pragma unroll
                        for (int s = 0; s < 4; ++s) rT[s] = sl[nl * 17 + 4 * s + g];
                        __builtin_amdgcn_wave_barrier();
#pragma unroll
                        for (int s = 0; s < 4; ++s) X = CBF_MFMA(rT[s], alj[i][s], X);
                    }
                }
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int r = 0; r < 4; ++r) sl[r * 64 + l] = X[r];
#pragma unroll
                for (int j2 = 0; j2 < JB; ++j2)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sl[MOFF + j2 * 256 + r * 64 + l] = macc[pp][j2][r];
#pragma unroll
                for (int d = 0; d < 16; ++d)
                    if (l == d) sl[TOFF + d] = tr[pp][d];
            }
            __syncthreads();

            // ---- 4: the slots in a fixed order; fmean, fcov, Cx into this step's pmeans, pcovs, cross
            const int fmo = MOFF + (D >> 4) * 256;      // the ones row: input index D
            for (int it = tid; it < PG * 136; it += NT) {
                const int pp = it / 136, q = it - pp * 136;
                int d = 0;
                while ((d + 1) * (d + 2) / 2 <= q) ++d;
                const int e = q - d * (d + 1) / 2;
                const int p = pbase + pp;
                if (d >= Do || p >= N) continue;
                const double* s0 = slot + pp * SLOT;
                double sde = 0.0, sed = 0.0, fd = 0.0, fe = 0.0, s1 = 0.0;
                for (int ww = 0; ww < W; ++ww) {
                    const double* s = s0 + ww * PG * SLOT;
                    sde += s[adf_cidx(d, e)];
                    sed += s[adf_cidx(e, d)];
                    fd += s[fmo + adf_cidx(d, D & 15)];
                    fe += s[fmo + adf_cidx(e, D & 15)];
                    s1 += s[TOFF + d];
                }
                const bool bad = (cst[pp * 4 + 2] + cst[pp * 4 + 3]) != 0.0;
                double val = (sde + sed) - fd * fe;
                if (d == e) val += sig2 - 2.0 * s1;
                if (bad) val = nan;
                double* fc = a.pcovs + (tN + p) * DD;
                fc[d * Do + e] = val;
                fc[e * Do + d] = val;
                if (d == e) a.pmeans[(tN + p) * Do + d] = bad ? nan : fd;
                if (q == 0 && bad && binfo[pgi * PG + pp] == 0.0) binfo[pgi * PG + pp] = double(t + 1);
            }
            for (int it = tid; it < PG * Do; it += NT) {
                const int pp = it / Do, d = it - pp * Do;
                const int p = pbase + pp;
                if (p >= N) continue;
                const double* L1 = L1t + pp * LT;
                const double* s0 = slot + pp * SLOT + MOFF;
                double y[DP], o[DP];
#pragma unroll
                for (int i = 0; i < DP; ++i) {
                    double acc = 0.0;
                    if (i < D) {
                        const int off = (i >> 4) * 256 + adf_cidx(d, i & 15);
                        for (int ww = 0; ww < W; ++ww) acc += s0[ww * PG * SLOT + off];
                    }
                    y[i] = acc;
                    o[i] = 0.0;
                }
                // L1 y' = y column by column, then L1^T t = y' from the last row up
#pragma unroll
                for (int j = 0; j < DP; ++j) {
                    if (j < D) {
                        y[j] *= inv1[pp * DP + j];
#pragma unroll
                        for (int i = j + 1; i < DP; ++i) y[i] = fma(-L1[j * DP + i], y[j], y[i]);
                    }
                }
#pragma unroll
                for (int j = DP - 1; j >= 0; --j) {
                    if (j < D) {
                        y[j] *= inv1[pp * DP + j];
#pragma unroll
                        for (int i = 0; i < j; ++i) y[i] = fma(-L1[i * DP + j], y[j], y[i]);
                    }
                }
                const bool bad = (cst[pp * 4 + 2] + cst[pp * 4 + 3]) != 0.0;
                const double* Sp = Sg + pp * LT;
#pragma unroll
                for (int j = 0; j < DP; ++j) {
                    if (j < D) {
#pragma unroll
                        for (int k = 0; k < DP; ++k) o[k] = fma(Sp[j * DP + k], y[j], o[k]);
                    }
                }
                double* cx = a.cross + ((tN + p) * Do + d) * Do;             // the state columns of xcov
#pragma unroll
                for (int k = 0; k < DP; ++k) {
                    if (k < Do) cx[k] = bad ? nan : o[k] / il[k];
                }
            }
        }
        __syncthreads();                                // fmean, fcov, Cx of the 16 chains are stored; the slots are free

        // ==== U: the transition step and the scalar updates, whole waves (lane ids < 256)
#pragma unroll
        for (int k2 = 0; k2 < TPT; ++k2) {
            const int id = tid + k2 * NT;
            if (id < 256) {                             // (wave uniform: 256 is a multiple of 64)
                const int n = id >> 4, i = id & 15;
                const bool act = i < Do;
                const int ic = act ? i : 0;
                double* Pn = Pt + n * 16 * PD;
                const bool dc = (cnd[k2] != 0.0);
                const bool dead = binfo[n] != 0.0;
                const bool st = act && (c0 + n < N);
                const int64_t oc = tN + lc[k2];         // (step, chain)
                const int64_t o = oc * Do + ic;

                // row i of P, of fcov and of Cx, column i of Cx
                double pr[16], cr[16];
                {
                    const double fm = act ? a.pmeans[o] : 0.0;
                    const double* fr = a.pcovs + o * Do;
                    const double* cxr = a.cross + o * Do;
                    const double* cxc = a.cross + oc * DD + ic;
                    const double* pb = Pprev ? Pprev + int64_t(lc[k2]) * DD : nullptr;
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const bool on = act && q < Do;
                        double pv = 0.0;
                        if (on && pb) pv = (t > 0 || q <= i) ? pb[i * Do + q] : pb[q * Do + i];   // P0: its lower triangle
                        const double ciq = on ? cxr[q] : 0.0, cqi = on ? cxc[q * Do] : 0.0;
                        const double fv = on ? fr[q] : 0.0;
                        cr[q] = pv + ciq;
                        pr[q] = (pv + (ciq + cqi)) + fv;
                        if (q == i) pr[q] += lvx[k2];
                        if (dead) { cr[q] = on ? nan : 0.0; pr[q] = on ? nan : 0.0; }
                    }
                    ln[k2].m = dead ? nan : ln[k2].m + fm;
                }
                double mi = ln[k2].m;
#pragma unroll
                for (int q = 0; q < 16; ++q) Pn[i * PD + q] = pr[q];
                __builtin_amdgcn_wave_barrier();        // the chain's 16 lanes have read fcov and Cx before one of them
                                                        // overwrites them, and the tile is whole
                if (st) {                               // the predicted moments, before conditioning
                    a.pmeans[o] = mi;
                    double* pc = a.pcovs + o * Do;
                    double* cc = a.cross + o * Do;
#pragma unroll
                    for (int q = 0; q < 16; ++q)
                        if (q < Do) { pc[q] = pr[q]; cc[q] = cr[q]; }
                }

                // C3 of gp_ekf_kernel: the scalar updates; the own row in registers, row j from LDS
#pragma unroll 1
                for (int j = 0; j < Dy; ++j) {
                    const double* rj = Pn + j * PD;
                    const double s = rj[j] + a.var_y[j];
                    const double pij = rj[i];
                    const double rs = 1.0 / s;
                    const double dl = __shfl(yv[k2], j, 16) - __shfl(mi, j, 16);
                    mi = dc ? mi + (pij * rs) * dl : mi;
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const double dn = (pij * rj[q]) * rs;
                        pr[q] = dc ? pr[q] - dn : pr[q];
                    }
                    ln[k2].lin += dc ? dl * dl * rs : 0.0;
                    ln[k2].lp.mul(dc ? 6.283185307179586477 * s : 1.0);
                    __builtin_amdgcn_wave_barrier();
                    if (i == j + 1) {                   // the next iteration reads this row
#pragma unroll
                        for (int q = 0; q < 16; ++q) Pn[i * PD + q] = pr[q];
                    }
                    __builtin_amdgcn_wave_barrier();
                }
                ln[k2].m = mi;
                if (st) {
                    a.means[o] = mi;
                    double* cv = a.covs + o * Do;
#pragma unroll
                    for (int q = 0; q < 16; ++q)
                        if (q < Do) cv[q] = pr[q];
                }
            }
        }
    }
    __syncthreads();

    // ---- loglik[n] = -1/2 sum over the conditioned (step, j) of log(2 pi s) + delta^2 / s: every lane of a chain holds it
#pragma unroll
    for (int k2 = 0; k2 < TPT; ++k2) {
        const int id = tid + k2 * NT;
        if (id < 256 && (id & 15) == 0 && c0 + (id >> 4) < N) {
            const double fl = binfo[id >> 4];
            a.loglik[lc[k2]] = (fl != 0.0) ? nan : 0.0 - 0.5 * (ln[k2].lp.log() + ln[k2].lin);
            a.info[lc[k2]] = fl;
        }
    }
}

template <int NBLK, int DK>
int launch_gp_adf_k(const GpAdfArgs& a, hipStream_t st)
{
    typedef GpBwdCfg<NBLK> C;
    const size_t lds = size_t(GpAdfGeom<NBLK, DK>::LDS_DOUBLES) * sizeof(double);
    auto k = gp_adf_kernel<NBLK, C::RB, DK>;
    int rc = set_lds(k, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k, dim3(unsigned((a.N + 15) / 16)), dim3(64 * C::W), lds, st, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -int(e) - 1000;
}

template <int NBLK>
int launch_gp_adf_n(int DK, const GpAdfArgs& a, hipStream_t st)
{
    switch (DK) {
        case 2: return launch_gp_adf_k<NBLK, 2>(a, st);
        case 4: return launch_gp_adf_k<NBLK, 4>(a, st);
        case 6: return launch_gp_adf_k<NBLK, 6>(a, st);
    }
    return -2;
}

}  // namespace cbfssm

#define CBF_GPADF_DECLARE(NB)                                                                    \
    namespace cbfssm {                                                                           \
    int launch_gp_adf_nb##NB(int DK, const GpAdfArgs& a, hipStream_t st);                        \
    }

#define CBF_GPADF_INSTANTIATE(NB)                                                                \
    namespace cbfssm {                                                                           \
    int launch_gp_adf_nb##NB(int DK, const GpAdfArgs& a, hipStream_t st)                         \
    {                                                                                            \
        return launch_gp_adf_n<NB>(DK, a, st);                                                   \
    }                                                                                            \
    }
