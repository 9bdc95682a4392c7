// Exact Gaussian moments of one sparse GP with an RBF kernel under a Gaussian input x ~ N(m, S): the mean of the output, its
// full covariance (with the correlation between output dimensions that sharing the uncertain input brings) and its covariance
// with the input -- the moment matching of PILCO and of the GP assumed-density filter -- for GPModel.predict's posterior
// (gp_tf.py:132-161, diagonal q(z)).  Nothing is linearised and nothing is sampled.
//
//   K = K_mm + jitter I,  alpha = K^-1 mu (M x Do),  s2 = zeta_var,  W_d = K^-1 - K^-1 diag(s2[:, d]) K^-1,  v = kernel variance
//   z~_i = z_i / l,  m~ = m / l,  S~ = S / (l l^T),  r_i = z~_i - m~
//
//   A1 = I + S~   = L1 L1^T     c1 = v   / prod diag L1                 w_i = L1^-1 r_i     q_i = c1 exp(-|w_i|^2 / 2)
//   A2 = I/2 + S~ = L2 L2^T     c2 = v^2 / (2^(D/2) prod diag L2)       u_i = L2^-1 r_i     g_i = |u_i|^2
//   Q_ij = c2 exp(-|z~_i - z~_j|^2 / 4 - (g_i + g_j + 2 u_i.u_j) / 8)
//
//   fmean[n][d]   = sum_i alpha_id q_i
//   xcov[n][d][:] = l o ( S~ L1^-T L1^-1 sum_i alpha_id q_i r_i )                                   (npts, Do, D)
//   fcov[n][d][e] = sum_ij alpha_id Q_ij alpha_je - fmean_d fmean_e + delta_de (v - sum_ij W_d,ij Q_ij)   (npts, Do, Do)
//
// Only A1 and A2 are factorised: both are positive definite for any positive semi-definite S, so singular S (zero blocks,
// rank one, S = 0) is the ordinary case; S = 0 gives predict back and xcov exactly zero (the last step is a product with S~).
//
// One workgroup per 16 points (persistent, grid stride), GpBwdCfg<NBLK>'s waves.  Q (M x M per point) never leaves the
// registers: it is produced and consumed as 16 x 16 tiles.  The 16 points go through the workgroup two at a time (PG):
//
//   0  per point one wave: rows of A1 in lanes 0..31, rows of A2 in lanes 32..63, a right-looking Cholesky factorisation in
//      registers with the pivot column handed round through LDS (one write, broadcast reads); L1, L2 (column by column),
//      1 / diag, S~ -> LDS
//   1  per (point, inducing row) one thread: w_i and u_i by forward substitution, column by column so that the updates of a
//      step are independent of each other (the factors are broadcast reads), q_i, g_i, u_i into the LDS image that is both MFMA operands of the Gram product U U^T
//   2  per wave its column blocks jb of Q, row blocks ib = jb, jb + 1, .. jb + NBLK / 2 (mod NBLK): every unordered pair of
//      blocks once (Q is symmetric; the diagonal tiles and, at even NBLK, the tiles half way round count half), the same
//      number of tiles for every column block.  Per tile, shared by the PG points: -|z~_i - z~_j|^2 / 4 from the pack's Z~
//      image (DK MFMAs), alpha's rows and the Do tiles of W_d; per point DK MFMAs of the Gram product, four exponentials per
//      lane, R_jb += alpha_ib^T Q (the tile in its accumulator layout is the B operand as it stands: 4 MFMAs) and the trace
//      sums tr_d += W_d o Q on the VALU.  Then the mean part of the wave's own rows against the pack's (Z~)^T image, whose
//      ones row gives fmean:  sum_i alpha_id q_i (z~_i - m~) and sum_i alpha_id q_i                              MFMA
//   3  per wave X = R_jb alpha_jb (one 16 x 16 transpose through LDS), X, the mean tiles and tr_d into the wave's slot (the
//      slots lie over the U image, which is dead behind a barrier)
//   4  the slots summed over the waves in a fixed order; fcov = (X + X^T) - fmean fmean^T + diag(v - 2 tr): one triangle is
//      computed and written to both places, so fcov[n] is bitwise symmetric; xcov per (point, d) by two triangular solves
//      with L1 and the product with S~.
//
// A non-positive pivot (S not positive semi-definite) sets info[n] = 1 (first factor) or 2 (second) and makes the three
// results of that point NaN; the point's arithmetic touches no other point's.  No atomics, every output entry has one
// writer, two calls are bitwise identical, and the results of a point do not depend on the other points of the call.  Rows
// m >= M of Q are set to zero; points >= npts are computed on zero inputs and never stored.
#pragma once
#include "../../include/cbfssm_hip.h"
#include "cbfssm_gp_bwd.hpp"

namespace cbfssm {

struct GpMmArgs {
    const double* Zp;      // [NBLK][DK][64]     Z~ as A-operand image
    const double* cz;      // [16 NBLK]          -|z~|^2 / 2 + log v (padding rows: -1e30)
    const double* invl;    // [4 DK]             1 / lengthscale, zero padded
    const double* scal;
    const double* Zs;      // [M][D]             Z~
    const double* ZT;      // [NBLK][JB][4][64]  (Z~)^T as A-operand image, row D = ones
    const double* alpha;   // [16][16 NBLK]      (K^-1 mu)[m][d] at [d][m], zero padded (gp_lin_alpha_kernel)
    const double* Wimg;    // [Do][NBLK][NBLK][4][64]  W_d tiles in the accumulator layout, zero padded (gp_mm_w_kernel)
    const double* mean;    // (npts, D)
    const double* cov;     // (npts, D, D), lower triangle read; null: zero
    double* fmean;         // (npts, Do)
    double* fcov;          // (npts, Do, Do)
    double* xcov;          // (npts, Do, D) or null
    double* info;          // (npts)
    int64_t npts;
    int64_t nblocks;       // ceil(npts / 16)
    int M, D, Do;
};

// LDS: region A | region B.  Region A holds the U images [PG][NBLK][DK][64] and L2 [PG][DP][DP] in steps 0 to 2 and the
// waves' slots [W][PG][SLOT] in steps 3 and 4 (slot: [16][17] transpose tile / X | JB mean tiles | 16 trace sums).  Region B
// lives through all steps: L1, 1 / diag L1, 1 / diag L2, S~, m~, q, g, four scalars per point, 1 / l.
template <int NBLK, int DK>
struct GpMmGeom {
    typedef GpBwdCfg<NBLK> C;
    static constexpr int PG = 2;
    static constexpr int DP = 4 * DK;
    static constexpr int MP = 16 * NBLK;
    static constexpr int JB = (4 * DK + 1 + 15) / 16;
    static constexpr int UOP = NBLK * DK * 64;
    static constexpr int LT = DP * DP;
    static constexpr int SLOT = 272 + JB * 256 + 16;
    static constexpr int RA0 = PG * UOP + PG * LT;
    static constexpr int RA1 = C::W * PG * SLOT;
    static constexpr int RA = RA0 > RA1 ? RA0 : RA1;
    static constexpr int RBD = 2 * PG * LT + 3 * PG * DP + 2 * PG * MP + 4 * PG + DP;
    static constexpr int LDS_DOUBLES = RA + RBD;
    static_assert(LDS_DOUBLES <= 163840 / 8, "LDS budget");
};

__device__ __forceinline__ int mm_cidx(int row, int col) { return (row >> 2) * 64 + (row & 3) * 16 + col; }

template <int NBLK, int RB, int DK>
__global__ __launch_bounds__(64 * ((NBLK + RB - 1) / RB)) void gp_moment_match_kernel(GpMmArgs a)
{
    typedef GpMmGeom<NBLK, DK> G;
    constexpr int W = (NBLK + RB - 1) / RB, NT = 64 * W, MP = G::MP, DP = G::DP, JB = G::JB, PG = G::PG;
    constexpr int UOP = G::UOP, LT = G::LT, SLOT = G::SLOT, H = NBLK / 2;
    constexpr int MOFF = 272, TOFF = 272 + JB * 256;

    extern __shared__ double lds[];
    double* Uop = lds;                                  // [PG][NBLK][DK][64]
    double* L2t = Uop + PG * UOP;                       // [PG][DP][DP]
    double* slot = lds;                                 // [W][PG][SLOT], over the two above
    double* L1t = lds + G::RA;                          // [PG][DP][DP]
    double* Sg = L1t + PG * LT;                         // [PG][DP][DP]  S~, both triangles
    double* inv1 = Sg + PG * LT;                        // [PG][DP]
    double* inv2 = inv1 + PG * DP;                      // [PG][DP]
    double* mt = inv2 + PG * DP;                        // [PG][DP]      m~
    double* qv = mt + PG * DP;                          // [PG][MP]
    double* gv = qv + PG * MP;                          // [PG][MP]
    double* cst = gv + PG * MP;                         // [PG][4]       c1, log c2, info of factor 1, of factor 2
    double* il = cst + 4 * PG;                          // [DP]

    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, g = l >> 4, nl = l & 15;
    const int M = a.M, D = a.D, Do = a.Do;
    const double sig2 = a.scal[CBFSSM_SCAL_SIGMA2];
    const double logv = log(sig2);

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
    for (int i = tid; i < DP; i += NT) il[i] = a.invl[i];           // (made visible by the barrier of the first group)

    for (int64_t cb = blockIdx.x; cb < a.nblocks; cb += gridDim.x) {
        for (int pgi = 0; pgi < 16 / PG; ++pgi) {
            const int64_t pbase = cb * 16 + pgi * PG;
            if (pbase >= a.npts) break;
            __syncthreads();                            // the previous group's readers of the slots and of region B are done

            // ---- 0: m~, and the two factorisations of a point on one wave
            for (int i = tid; i < PG * DP; i += NT) {
                const int pp = i / DP, k = i - pp * DP;
                const int64_t p = pbase + pp;
                mt[i] = (k < D && p < a.npts) ? a.mean[p * D + k] * il[k] : 0.0;
            }
            for (int pp = w; pp < PG; pp += W) {
                const int hh = l >> 5, i = l & 31;
                const int64_t p = pbase + pp;
                const bool have = a.cov != nullptr && p < a.npts && i < D;
                const double ili = (i < D) ? a.invl[i] : 0.0;
                double arow[DP];
#pragma unroll
                for (int j = 0; j < DP; ++j) {
                    double s = 0.0;
                    if (have && j <= i) s = a.cov[(p * D + i) * D + j] * ili * a.invl[j];
                    if (hh == 0 && i < DP && j <= i) {
                        Sg[pp * LT + i * DP + j] = s;
                        Sg[pp * LT + j * DP + i] = s;
                    }
                    arow[j] = s + ((j == i) ? (hh ? 0.5 : 1.0) : 0.0);
                }
                double prod = 1.0;
                bool bad = false;
                double* invd = (hh ? inv2 : inv1) + pp * DP;
                // column k of the trailing matrix goes round through LDS (the U image's place, free until step 1): one
                // write and DP / 2 broadcast reads per column, where lane shuffles would be one round trip per entry
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
                        if (!(akk > 0.0)) { bad = true; akk = 1.0; }
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
                // column by column: once u[j] is final the updates of the rows below it are independent of each other
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
                        double t = tr[pp][d];
#pragma unroll
                        for (int o = 1; o < 64; o <<= 1) t += __shfl_xor(t, o);
                        tr[pp][d] = t;
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

            // ---- 4: the slots in a fixed order, the results
            const int fmo = MOFF + (D >> 4) * 256;      // the ones row: input index D
            for (int it = tid; it < PG * 136; it += NT) {
                const int pp = it / 136, q = it - pp * 136;
                int d = 0;
                while ((d + 1) * (d + 2) / 2 <= q) ++d;
                const int e = q - d * (d + 1) / 2;
                const int64_t p = pbase + pp;
                if (d >= Do || p >= a.npts) continue;
                const double* s0 = slot + pp * SLOT;
                double sde = 0.0, sed = 0.0, fd = 0.0, fe = 0.0, t = 0.0;
                for (int ww = 0; ww < W; ++ww) {
                    const double* s = s0 + ww * PG * SLOT;
                    sde += s[mm_cidx(d, e)];
                    sed += s[mm_cidx(e, d)];
                    fd += s[fmo + mm_cidx(d, D & 15)];
                    fe += s[fmo + mm_cidx(e, D & 15)];
                    t += s[TOFF + d];
                }
                const double bad = cst[pp * 4 + 2] + cst[pp * 4 + 3];
                double val = (sde + sed) - fd * fe;
                if (d == e) val += sig2 - 2.0 * t;
                if (bad != 0.0) val = __builtin_nan("");
                a.fcov[(p * Do + d) * Do + e] = val;
                a.fcov[(p * Do + e) * Do + d] = val;
                if (d == e) a.fmean[p * Do + d] = (bad != 0.0) ? __builtin_nan("") : fd;
                if (q == 0) a.info[p] = (cst[pp * 4 + 2] != 0.0) ? 1.0 : cst[pp * 4 + 3];
            }
            if (a.xcov) {
                for (int it = tid; it < PG * Do; it += NT) {
                    const int pp = it / Do, d = it - pp * Do;
                    const int64_t p = pbase + pp;
                    if (p >= a.npts) continue;
                    const double* L1 = L1t + pp * LT;
                    const double* s0 = slot + pp * SLOT + MOFF;
                    double y[DP], o[DP];
#pragma unroll
                    for (int i = 0; i < DP; ++i) {
                        double acc = 0.0;
                        if (i < D) {
                            const int off = (i >> 4) * 256 + mm_cidx(d, i & 15);
                            for (int ww = 0; ww < W; ++ww) acc += s0[ww * PG * SLOT + off];
                        }
                        y[i] = acc;
                        o[i] = 0.0;
                    }
                    // L1 y' = y column by column, then L1^T t = y' from the last row up: the updates of one step are
                    // independent of each other
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
#pragma unroll
                    for (int k = 0; k < DP; ++k) {
                        if (k < D)
                            a.xcov[(p * Do + d) * D + k] = bad ? __builtin_nan("") : o[k] / il[k];
                    }
                }
            }
        }
    }
}

template <int NBLK, int DK>
int launch_gp_mm_k(const GpMmArgs& a, unsigned nwg, hipStream_t st)
{
    typedef GpBwdCfg<NBLK> C;
    const size_t lds = size_t(GpMmGeom<NBLK, DK>::LDS_DOUBLES) * sizeof(double);
    auto k = gp_moment_match_kernel<NBLK, C::RB, DK>;
    int rc = set_lds(k, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k, dim3(nwg), dim3(64 * C::W), lds, st, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -int(e) - 1000;
}

template <int NBLK>
int launch_gp_mm_n(int DK, const GpMmArgs& a, unsigned nwg, hipStream_t st)
{
    switch (DK) {
        case 2: return launch_gp_mm_k<NBLK, 2>(a, nwg, st);
        case 4: return launch_gp_mm_k<NBLK, 4>(a, nwg, st);
        case 6: return launch_gp_mm_k<NBLK, 6>(a, nwg, st);
    }
    return -2;
}

}  // namespace cbfssm

#define CBF_GPMM_DECLARE(NB)                                                                     \
    namespace cbfssm {                                                                           \
    int launch_gp_mm_nb##NB(int DK, const GpMmArgs& a, unsigned nwg, hipStream_t st);            \
    }

#define CBF_GPMM_INSTANTIATE(NB)                                                                 \
    namespace cbfssm {                                                                           \
    int launch_gp_mm_nb##NB(int DK, const GpMmArgs& a, unsigned nwg, hipStream_t st)             \
    {                                                                                            \
        return launch_gp_mm_n<NB>(DK, a, nwg, st);                                               \
    }                                                                                            \
    }
