// The adjoint of GPModel.moment_match (cbfssm_gp_mm.hpp) with respect to the inputs of the call, mean and cov; the model is a
// constant.  Given the cotangents gf (Do), gC (Do x Do, need not be symmetric) and gX (Do x D) of fmean, fcov and xcov of a
// point, with the notation of the forward (A = I + S~ = L1 L1^T, B = I / 2 + S~ = L2 L2^T, r_i = z~_i - m~, w_i = L1^-1 r_i,
// u_i = L2^-1 r_i, q_i, Q_ij) and H = R^T diag(q) alpha (D x Do):
//
//   fm_bar = gf - (gC + gC^T) fmean
//   Qbar   = alpha Gs alpha^T - sum_d gC_dd W_d,  Gs = (gC + gC^T) / 2        E = Qbar o Q (symmetric),  e_i = sum_j E_ij
//   Yh     = diag(l) gX^T;  AH = A^-1 H;  Hb = A^-1 S~ Yh
//   qbar_i = (alpha fm_bar)_i + r_i^T Hb alpha_i;   eb_i = qbar_i q_i
//   sum_i rbar_i = Hb fmean - L1^-T sum eb_i w_i - L2^-T sum e_i u_i
//   Sbar~  = (Yh - Hb) AH^T + 1/2 L1^-T (W^T diag(eb) W - (sum eb) I) L1^-1
//                           + L2^-T (1/4 (U^T diag(e) U + U^T E U) - 1/2 (sum e) I) L2^-1
//   gmean  = -(sum_i rbar_i) / l;   Sbar = Sbar~ / (l l^T);   gcov = tril(Sbar + Sbar^T) - diag(Sbar)
//
// gcov is the gradient of the function of tril(cov) + tril(cov, -1)^T: exactly zero above the diagonal (written here), both
// symmetric contributions on a strictly lower entry.  No Cholesky adjoint: the only linear algebra is substitution with L1
// and L2.  The only M x M object is E; it is needed through its row sums and through U^T E U.
//
// One workgroup per 16 points (persistent, grid stride), GpBwdCfg<NBLK>'s waves, two points per round, the forward's steps:
//
//   0, 1  as the forward: the two register Cholesky factorisations, w_i, u_i, q_i, g_i, the U image
//   2     the forward's tile walk (every unordered pair of row blocks once, the diagonal and half-way tiles count half).  Per
//         tile and point: Q as in the forward; Qbar = (alpha_ib)(Gs alpha_jb^T) on the f64 MFMA units (the second factor once
//         per column block, in registers) minus sum_d gC_dd W_d on the VALU; E = Qbar o Q; the column sums of the tile into the
//         wave's registers, its row sums into the workgroup's scratch at [o][row] (one writer each);  T_jb += U_ib^T E with
//         the tile in its accumulator layout as the B operand.  Then the mean part of the wave's rows as in the forward: its
//         tiles are H and, in the ones row, fmean.  Without a cotangent for fcov the tile walk is skipped: E = 0.
//   3     per wave G_half = sum T_jb U_jb (one 16 x 16 transpose through LDS per tile of T) into its slot in the scratch, the
//         mean tiles into its LDS slot (over the dead U image), the column sums into e
//   4     the slots summed over the waves in a fixed order: e (column sums + the row sums in the order of o), fmean, H,
//         U^T E U = G_half + G_half^T
//   5     per (point, d): fm_bar, AH, Yh, Hb (substitutions with L1)
//   6     per (point, row): w_i again, qbar_i, eb_i, the W image; then per (k1, k2) the Gram sum over the rows in a fixed order
//   7     the same for u_i and e
//   8, 9  two rounds of back substitution per column: L^-T G, then L^-T (L^-T G)^T, and the two vectors
//   10    Sbar, the stores of gmean, the lower triangle of gcov and explicit zeros above it
//
// The small per-point matrices between the steps and the waves' G_half slots live in a scratch of the workgroup in global
// memory (L2 resident; `work` behind the forward's sections): at the largest leaf the forward's LDS image leaves 208 doubles.
// Workgroup barriers only, no atomics, every sum over waves or rows in a fixed order: two calls are bitwise identical and a
// point's gradient does not depend on the other points of the call.  info[n] != 0 (a non-positive pivot): the rows of point n
// of both gradients are NaN, by select; points >= npts are computed on zero inputs and never stored.
//
// Registers and scratch of the 24 instantiations, from -Rpass-analysis=kernel-resource-usage (the full table with SGPRs and
// occupancy: profiles/gp_moment_match_grad/resource_usage.txt).  Every leaf sits at the register limit of its workgroup size:
// 256 VGPRs up to sixteen row blocks (one wave per SIMD up to four, two from seven), 168 at twenty (three waves per SIMD).
//
//   NBLK             1     2     4     7    10    13    16    20
//   AGPRs    DK 2  190   152   182     0     0     0     0     0
//            DK 4  256   256   256     0     0     0     0     0
//            DK 6  256   256   256     0     0     0     0     0
//   scratch  DK 2    0     0     0   684  1028  1044  1088  1504      (bytes per lane)
//            DK 4  140   136   196   948  1312  1348  1584  2068
//            DK 6  500   736   744  1644  2272  2284  2296  2680
#pragma once
#include "../../include/cbfssm_hip.h"
#include "cbfssm_gp_bwd.hpp"

namespace cbfssm {

struct GpMmBwdArgs {
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
    const double* gfmean;  // (npts, Do) or null: zero
    const double* gfcov;   // (npts, Do, Do) or null: zero
    const double* gxcov;   // (npts, Do, D) or null: zero
    double* gmean;         // (npts, D)
    double* gcov;          // (npts, D, D) or null
    double* info;          // (npts) or null
    double* scratch;       // [workgroup][GpMmBwdGeom::SCRATCH]
    int64_t npts;
    int64_t nblocks;       // ceil(npts / 16)
    int M, D, Do;
};

// doubles of one workgroup's scratch: per point of the pair the waves' G_half slots, the row sums [o][row], H / AH / Yh / Hb as
// [16][DP], U^T E U, the two Gram matrices, the two rounds of substitution results and four vectors
constexpr int gp_mmb_waves(int NBLK) { return NBLK > 7 ? (NBLK + 1) / 2 : NBLK; }
constexpr int64_t gp_mmb_point_scratch(int NBLK, int DK)
{
    return int64_t(gp_mmb_waves(NBLK)) * 16 * DK * DK + int64_t(NBLK / 2 + 1) * 16 * NBLK + 4 * 16 * 4 * DK +
           7 * 16 * DK * DK + 4 * 4 * DK;
}
constexpr int64_t gp_mmb_scratch(int NBLK, int DK) { return 2 * gp_mmb_point_scratch(NBLK, DK); }

// LDS: region A | L2 | region B.  Region A holds the U images [PG][NBLK][DK][64] in steps 0 to 2, the waves' slots [W][PG][SB]
// in steps 3 and 4 (a [16][17] transpose tile, then the JB mean tiles over it) and the row images of w and of u [PG][MP][DP] in
// steps 6 and 7.  L2 and region B live through all steps: region B is the forward's (g becomes e in step 3, q becomes eb in
// step 6) with gC's diagonal, fmean and fm_bar behind it.
template <int NBLK, int DK>
struct GpMmBwdGeom {
    typedef GpBwdCfg<NBLK> C;
    static constexpr int PG = 2;
    static constexpr int DP = 4 * DK;
    static constexpr int MP = 16 * NBLK;
    static constexpr int JB = (4 * DK + 1 + 15) / 16;
    static constexpr int JD = (DP + 15) / 16;
    static constexpr int UOP = NBLK * DK * 64;
    static constexpr int LT = DP * DP;
    static constexpr int SB = JB * 256 > 272 ? JB * 256 : 272;
    static constexpr int RA = PG * UOP > C::W * PG * SB ? PG * UOP : C::W * PG * SB;
    static constexpr int RBD = 2 * PG * LT + 3 * PG * DP + 2 * PG * MP + 4 * PG + DP + 3 * PG * 16;
    static constexpr int LDS_DOUBLES = RA + PG * LT + RBD;
    static constexpr int H = NBLK / 2;
    static constexpr int64_t PSCR = gp_mmb_point_scratch(NBLK, DK);
    static constexpr int64_t SCRATCH = gp_mmb_scratch(NBLK, DK);
    static_assert(C::W == gp_mmb_waves(NBLK), "the waves of a tile height");
    static_assert(PSCR == int64_t(C::W) * LT + int64_t(H + 1) * MP + 4 * 16 * DP + 7 * LT + 4 * DP, "scratch sections");
    static_assert(LDS_DOUBLES <= 163840 / 8, "LDS budget");
};

__device__ __forceinline__ int mmb_cidx(int row, int col) { return (row >> 2) * 64 + (row & 3) * 16 + col; }

template <int NBLK, int RB, int DK>
__global__ __launch_bounds__(64 * ((NBLK + RB - 1) / RB)) void gp_moment_match_bwd_kernel(GpMmBwdArgs a)
{
    typedef GpMmBwdGeom<NBLK, DK> G;
    constexpr int W = (NBLK + RB - 1) / RB, NT = 64 * W, MP = G::MP, DP = G::DP, JB = G::JB, JD = G::JD, PG = G::PG;
    constexpr int UOP = G::UOP, LT = G::LT, SB = G::SB, H = G::H;
    // sections of a point's scratch
    constexpr int64_t XW = 0, EROW = XW + int64_t(W) * LT, HR = EROW + int64_t(H + 1) * MP, AHS = HR + 16 * DP;
    constexpr int64_t YHS = AHS + 16 * DP, HBS = YHS + 16 * DP, G2 = HBS + 16 * DP, GWU = G2 + LT, P12 = GWU + 2 * LT;
    constexpr int64_t MX = P12 + 2 * LT, VEC = MX + 2 * LT;
    static_assert(VEC + 4 * DP == G::PSCR, "scratch sections");

    extern __shared__ double lds[];
    double* Uop = lds;                                  // [PG][NBLK][DK][64]
    double* slot = lds;                                 // [W][PG][SB], over the above
    double* img = lds;                                  // [PG][MP][DP], over the above
    double* L2t = lds + G::RA;                          // [PG][DP][DP]
    double* L1t = L2t + PG * LT;                        // [PG][DP][DP]
    double* Sg = L1t + PG * LT;                         // [PG][DP][DP]  S~, both triangles
    double* inv1 = Sg + PG * LT;                        // [PG][DP]
    double* inv2 = inv1 + PG * DP;                      // [PG][DP]
    double* mt = inv2 + PG * DP;                        // [PG][DP]      m~
    double* qv = mt + PG * DP;                          // [PG][MP]      q, from step 6 eb
    double* gv = qv + PG * MP;                          // [PG][MP]      g, from step 3 e
    double* cst = gv + PG * MP;                         // [PG][4]       c1, log c2, info of factor 1, of factor 2
    double* il = cst + 4 * PG;                          // [DP]
    double* gd = il + DP;                               // [PG][16]      diag gC
    double* fmv = gd + PG * 16;                         // [PG][16]      fmean
    double* fbv = fmv + PG * 16;                        // [PG][16]      fm_bar

    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, g = l >> 4, nl = l & 15;
    const int M = a.M, D = a.D, Do = a.Do;
    const double sig2 = a.scal[CBFSSM_SCAL_SIGMA2];
    const double logv = log(sig2);
    const bool haveC = a.gfcov != nullptr;
    double* scr = a.scratch + int64_t(blockIdx.x) * G::SCRATCH;

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
            __syncthreads();                            // the previous group's readers of the LDS and of the scratch are done

            // ---- 0: m~, diag gC, and the two factorisations of a point on one wave (the forward's step 0)
            for (int i = tid; i < PG * DP; i += NT) {
                const int pp = i / DP, k = i - pp * DP;
                const int64_t p = pbase + pp;
                mt[i] = (k < D && p < a.npts) ? a.mean[p * D + k] * il[k] : 0.0;
            }
            for (int i = tid; i < PG * 16; i += NT) {
                const int pp = i >> 4, d = i & 15;
                const int64_t p = pbase + pp;
                gd[i] = (haveC && d < Do && p < a.npts) ? a.gfcov[(p * Do + d) * Do + d] : 0.0;
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

            // ---- 1: w_i, u_i by forward substitution, q_i, g_i, the U image (the forward's step 1)
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

            // ---- 2: the tiles of E of this wave's column blocks, and the mean part of its rows
            d4 Tacc[RB][PG][JD], macc[PG][JB];
            double ecol[RB][PG], Ub[RB][PG][JD][4];
#pragma unroll
            for (int pp = 0; pp < PG; ++pp) {
#pragma unroll
                for (int i = 0; i < RB; ++i) {
                    ecol[i][pp] = 0.0;
#pragma unroll
                    for (int t = 0; t < JD; ++t) {
                        Tacc[i][pp][t] = d4{0, 0, 0, 0};
#pragma unroll
                        for (int s = 0; s < 4; ++s) Ub[i][pp][t][s] = 0.0;
                    }
                }
#pragma unroll
                for (int jb = 0; jb < JB; ++jb) macc[pp][jb] = d4{0, 0, 0, 0};
            }
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                if (ok[i]) {
                    const int jb = rbs[i];
                    if (haveC) {
                        const bool colok = (16 * jb + nl) < M;
                        double Uj[PG][DK], Zj[DK], gj[PG], lc2[PG], Gj[PG][4];
#pragma unroll
                        for (int s = 0; s < DK; ++s) Zj[s] = 0.5 * a.Zp[(jb * DK + s) * 64 + l];
#pragma unroll
                        for (int pp = 0; pp < PG; ++pp) {
#pragma unroll
                            for (int s = 0; s < DK; ++s) Uj[pp][s] = Uop[pp * UOP + (jb * DK + s) * 64 + l];
                            gj[pp] = gv[pp * MP + 16 * jb + nl];
                            lc2[pp] = cst[pp * 4 + 1];
                            // the B operand of Qbar's product: (Gs alpha_jb^T)[d = 4 s + g][col = nl]
                            const int64_t p = pbase + pp;
#pragma unroll
                            for (int s = 0; s < 4; ++s) Gj[pp][s] = 0.0;
                            if (p < a.npts) {
                                const double* gC = a.gfcov + p * Do * Do;
                                for (int e = 0; e < Do; ++e) {
                                    const double ae = a.alpha[e * MP + 16 * jb + nl];
#pragma unroll
                                    for (int s = 0; s < 4; ++s) {
                                        const int d = 4 * s + g;
                                        if (d < Do) Gj[pp][s] = fma(0.5 * (gC[d * Do + e] + gC[e * Do + d]), ae, Gj[pp][s]);
                                    }
                                }
                            }
                            // the B operand of G_half = T_jb U_jb: U[16 jb + 4 s + g][k2 = 16 t + nl]
#pragma unroll
                            for (int t = 0; t < JD; ++t) {
                                const int k2 = 16 * t + nl;
                                if (k2 < DP) {
#pragma unroll
                                    for (int s = 0; s < 4; ++s)
                                        Ub[i][pp][t][s] = Uop[pp * UOP + (jb * DK + (k2 >> 2)) * 64 + (k2 & 3) * 16 + 4 * s + g];
                                }
                            }
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
                                ali[r] = a.alpha[(4 * r + g) * MP + 16 * ib + nl];      // A operand: alpha[row = nl][d = 4 r + g]
                                rowok[r] = colok && row < M;
                            }
#pragma unroll
                            for (int s = 0; s < DK; ++s) zz = CBF_MFMA(a.Zp[(ib * DK + s) * 64 + l], Zj[s], zz);
                            d4 Q[PG], Qb[PG];
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
                                Qb[pp] = d4{0, 0, 0, 0};
#pragma unroll
                                for (int s = 0; s < 4; ++s) Qb[pp] = CBF_MFMA(ali[s], Gj[pp][s], Qb[pp]);
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
                                        for (int r = 0; r < 4; ++r) Qb[pp][r] = fma(-gd[pp * 16 + d], wv[r], Qb[pp][r]);
                                }
                            }
#pragma unroll
                            for (int pp = 0; pp < PG; ++pp) {
                                d4 E;
#pragma unroll
                                for (int r = 0; r < 4; ++r) E[r] = rowok[r] ? Qb[pp][r] * Q[pp][r] : 0.0;
                                ecol[i][pp] += (E[0] + E[1]) + (E[2] + E[3]);
                                double rs[4];
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    double v = E[r];
                                    v += __shfl_xor(v, 1);
                                    v += __shfl_xor(v, 2);
                                    v += __shfl_xor(v, 4);
                                    v += __shfl_xor(v, 8);
                                    rs[r] = v;
                                }
                                if (nl < 4) {
                                    const double v = (nl == 0) ? rs[0] : ((nl == 1) ? rs[1] : ((nl == 2) ? rs[2] : rs[3]));
                                    scr[pp * G::PSCR + EROW + o * MP + 16 * ib + 4 * nl + g] = v;
                                }
                                // T_jb += U_ib^T E: A operand U[16 ib + 4 r + g][k = 16 t + nl], the tile as it stands is B
#pragma unroll
                                for (int t = 0; t < JD; ++t) {
                                    const int k = 16 * t + nl;
                                    const double* Ua = Uop + pp * UOP + (ib * DK + ((k < DP) ? (k >> 2) : 0)) * 64 + (k & 3) * 16 + g;
#pragma unroll
                                    for (int r = 0; r < 4; ++r) {
                                        const double ua = (k < DP) ? Ua[4 * r] : 0.0;
                                        Tacc[i][pp][t] = CBF_MFMA(ua, E[r], Tacc[i][pp][t]);
                                    }
                                }
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
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int pp = 0; pp < PG; ++pp) ecol[i][pp] = gp_sum_groups(ecol[i][pp]);
            __syncthreads();                            // every wave is done with the U images and with g: the slots are free

            // ---- 3: G_half of this wave's column blocks into its scratch slot, e's column sums, the mean tiles into the LDS slot
#pragma unroll
            for (int pp = 0; pp < PG; ++pp) {
                double* sl = slot + (w * PG + pp) * SB;
                if (haveC) {
                    d4 X[JD][JD];
#pragma unroll
                    for (int t1 = 0; t1 < JD; ++t1)
#pragma unroll
                        for (int t2 = 0; t2 < JD; ++t2) X[t1][t2] = d4{0, 0, 0, 0};
#pragma unroll
                    for (int i = 0; i < RB; ++i) {
                        if (ok[i]) {
#pragma unroll
                            for (int t1 = 0; t1 < JD; ++t1) {
                                double rT[4];
#pragma unroll
                                for (int r = 0; r < 4; ++r) sl[(4 * r + g) * 17 + nl] = Tacc[i][pp][t1][r];
                                __builtin_amdgcn_wave_barrier();
#pragma unroll
                                for (int s = 0; s < 4; ++s) rT[s] = sl[nl * 17 + 4 * s + g];
                                __builtin_amdgcn_wave_barrier();
#pragma unroll
                                for (int t2 = 0; t2 < JD; ++t2)
#pragma unroll
                                    for (int s = 0; s < 4; ++s) X[t1][t2] = CBF_MFMA(rT[s], Ub[i][pp][t2][s], X[t1][t2]);
                            }
                            if (g == 0) gv[pp * MP + 16 * rbs[i] + nl] = ecol[i][pp];
                        }
                    }
                    double* xw = scr + pp * G::PSCR + XW + w * LT;
#pragma unroll
                    for (int t1 = 0; t1 < JD; ++t1)
#pragma unroll
                        for (int t2 = 0; t2 < JD; ++t2)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int k1 = 16 * t1 + 4 * r + g, k2 = 16 * t2 + nl;
                                if (k1 < DP && k2 < DP) xw[k1 * DP + k2] = X[t1][t2][r];
                            }
                }
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int j2 = 0; j2 < JB; ++j2)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sl[j2 * 256 + r * 64 + l] = macc[pp][j2][r];
            }
            __syncthreads();

            // ---- 4: the slots in a fixed order: e, fmean, H, U^T E U
            for (int it = tid; it < PG * MP; it += NT) {
                const int pp = it / MP, m = it - pp * MP;
                double e = 0.0;
                if (haveC) {
                    e = gv[it];
                    const double* er = scr + pp * G::PSCR + EROW + m;
                    for (int o = 0; o <= H; ++o) e += er[o * MP];
                }
                gv[it] = e;
            }
            for (int it = tid; it < PG * 16 * (DP + 1); it += NT) {
                const int pp = it / (16 * (DP + 1)), q = it - pp * 16 * (DP + 1);
                const int d = q / (DP + 1), k = q - d * (DP + 1);
                const int col = (k == DP) ? D : k;
                double acc = 0.0;
                if (d < Do && (k == DP || k < D)) {
                    const int off = (col >> 4) * 256 + mmb_cidx(d, col & 15);
                    for (int ww = 0; ww < W; ++ww) acc += slot[(ww * PG + pp) * SB + off];
                }
                if (k == DP) fmv[pp * 16 + d] = acc;
                else scr[pp * G::PSCR + HR + d * DP + k] = acc;
            }
            for (int it = tid; it < PG * LT; it += NT) {
                const int pp = it / LT, q = it - pp * LT;
                const int k1 = q / DP, k2 = q - k1 * DP;
                double acc = 0.0;
                if (haveC && k1 < D && k2 < D) {
                    const double* xw = scr + pp * G::PSCR + XW;
                    for (int ww = 0; ww < W; ++ww) acc += xw[ww * LT + k1 * DP + k2] + xw[ww * LT + k2 * DP + k1];
                }
                scr[pp * G::PSCR + G2 + q] = acc;
            }
            __syncthreads();

            // ---- 5: per (point, d): fm_bar, AH = A^-1 H, Yh = l o gX, Hb = A^-1 S~ Yh
            for (int it = tid; it < PG * 16; it += NT) {
                const int pp = it >> 4, d = it & 15;
                const int64_t p = pbase + pp;
                const bool live = d < Do && p < a.npts;
                const double* L1 = L1t + pp * LT;
                double* ps = scr + pp * G::PSCR;
                double fb = 0.0;
                if (live) {
                    if (a.gfmean) fb = a.gfmean[p * Do + d];
                    if (haveC) {
                        const double* gC = a.gfcov + p * Do * Do;
                        for (int e = 0; e < Do; ++e) fb = fma(-(gC[d * Do + e] + gC[e * Do + d]), fmv[pp * 16 + e], fb);
                    }
                }
                fbv[it] = fb;
                double y[DP], yh[DP], t[DP];
#pragma unroll
                for (int i = 0; i < DP; ++i) {
                    y[i] = ps[HR + d * DP + i];
                    yh[i] = (live && a.gxcov && i < D) ? a.gxcov[(p * Do + d) * D + i] / il[i] : 0.0;
                    t[i] = 0.0;
                }
                const double* Sp = Sg + pp * LT;
#pragma unroll
                for (int j = 0; j < DP; ++j) {
                    if (j < D) {
#pragma unroll
                        for (int k = 0; k < DP; ++k) t[k] = fma(Sp[j * DP + k], yh[j], t[k]);
                    }
                }
#pragma unroll
                for (int j = 0; j < DP; ++j) {
                    if (j < D) {
                        y[j] *= inv1[pp * DP + j];
                        t[j] *= inv1[pp * DP + j];
#pragma unroll
                        for (int i = j + 1; i < DP; ++i) {
                            y[i] = fma(-L1[j * DP + i], y[j], y[i]);
                            t[i] = fma(-L1[j * DP + i], t[j], t[i]);
                        }
                    }
                }
#pragma unroll
                for (int j = DP - 1; j >= 0; --j) {
                    if (j < D) {
                        y[j] *= inv1[pp * DP + j];
                        t[j] *= inv1[pp * DP + j];
#pragma unroll
                        for (int i = 0; i < j; ++i) {
                            y[i] = fma(-L1[i * DP + j], y[j], y[i]);
                            t[i] = fma(-L1[i * DP + j], t[j], t[i]);
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < DP; ++i) {
                    ps[AHS + d * DP + i] = y[i];
                    ps[YHS + d * DP + i] = yh[i];
                    ps[HBS + d * DP + i] = t[i];
                }
            }
            __syncthreads();

            // ---- 6, 7: the row images of w (with eb) and of u (with e), and their Gram sums in the order of the rows
#pragma unroll 1
            for (int pass = 0; pass < 2; ++pass) {
                for (int it = tid; it < PG * MP; it += NT) {
                    const int pp = it / MP, m = it - pp * MP;
                    const double* Lx = (pass ? L2t : L1t) + pp * LT;
                    const double* ivx = (pass ? inv2 : inv1) + pp * DP;
                    double r[DP], u[DP];
#pragma unroll
                    for (int k = 0; k < DP; ++k) r[k] = (m < M && k < D) ? a.Zs[m * D + k] - mt[pp * DP + k] : 0.0;
#pragma unroll
                    for (int i = 0; i < DP; ++i) u[i] = r[i];
#pragma unroll
                    for (int j = 0; j < DP; ++j) {
                        if (j < D) {
                            u[j] *= ivx[j];
#pragma unroll
                            for (int i = j + 1; i < DP; ++i) u[i] = fma(-Lx[j * DP + i], u[j], u[i]);
                        }
                    }
#pragma unroll
                    for (int k = 0; k < DP; ++k) img[it * DP + k] = u[k];
                    if (pass == 0) {
                        const double* hb = scr + pp * G::PSCR + HBS;
                        double qb = 0.0;
                        for (int d = 0; d < Do; ++d) {
                            double c = fbv[pp * 16 + d];
#pragma unroll
                            for (int k = 0; k < DP; ++k) c = fma(r[k], hb[d * DP + k], c);
                            qb = fma(a.alpha[d * MP + m], c, qb);
                        }
                        qv[it] = (m < M) ? qb * qv[it] : 0.0;
                    }
                }
                __syncthreads();
                const double* wt = pass ? gv : qv;
                for (int it = tid; it < PG * DP * (DP + 1); it += NT) {
                    const int pp = it / (DP * (DP + 1)), q = it - pp * DP * (DP + 1);
                    const int k1 = q / (DP + 1), k2 = q - k1 * (DP + 1);
                    const double* im = img + pp * MP * DP;
                    const double* wp = wt + pp * MP;
                    double* ps = scr + pp * G::PSCR;
                    double acc = 0.0, tot = 0.0;
                    if (k2 == DP) {
                        for (int m = 0; m < M; ++m) acc = fma(wp[m], im[m * DP + k1], acc);
                        ps[VEC + pass * DP + k1] = acc;
                    } else {
                        for (int m = 0; m < M; ++m) {
                            acc = fma(wp[m] * im[m * DP + k1], im[m * DP + k2], acc);
                            tot += wp[m];
                        }
                        if (pass == 0) acc = (k1 == k2) ? acc - tot : acc;
                        else acc = 0.25 * (acc + ps[G2 + k1 * DP + k2]) - ((k1 == k2) ? 0.5 * tot : 0.0);
                        ps[GWU + pass * LT + k1 * DP + k2] = acc;
                    }
                }
                __syncthreads();
            }

            // ---- 8, 9: L^-T G, then L^-T (L^-T G)^T, column by column; in round 0 also the two vectors
#pragma unroll 1
            for (int round = 0; round < 2; ++round) {
                for (int it = tid; it < PG * 2 * (DP + 1); it += NT) {
                    const int pp = it / (2 * (DP + 1)), q = it - pp * 2 * (DP + 1);
                    const int which = q / (DP + 1), c = q - which * (DP + 1);
                    const double* Lx = (which ? L2t : L1t) + pp * LT;
                    const double* ivx = (which ? inv2 : inv1) + pp * DP;
                    double* ps = scr + pp * G::PSCR;
                    if (c == DP ? round == 1 : c >= D) continue;
                    double x[DP];
#pragma unroll
                    for (int k = 0; k < DP; ++k) {
                        if (c == DP) x[k] = ps[VEC + which * DP + k];
                        else if (round == 0) x[k] = ps[GWU + which * LT + k * DP + c];
                        else x[k] = ps[P12 + which * LT + k * DP + c];
                    }
#pragma unroll
                    for (int j = DP - 1; j >= 0; --j) {
                        if (j < D) {
                            x[j] *= ivx[j];
#pragma unroll
                            for (int i = 0; i < j; ++i) x[i] = fma(-Lx[i * DP + j], x[j], x[i]);
                        }
                    }
#pragma unroll
                    for (int k = 0; k < DP; ++k) {
                        if (c == DP) ps[VEC + (2 + which) * DP + k] = x[k];
                        else if (round == 0) ps[P12 + which * LT + c * DP + k] = x[k];
                        else ps[MX + which * LT + c * DP + k] = x[k];
                    }
                }
                __syncthreads();
            }

            // ---- 10: Sbar~, and the stores
            for (int it = tid; it < PG * DP; it += NT) {
                const int pp = it / DP, k = it - pp * DP;
                const int64_t p = pbase + pp;
                if (k >= D || p >= a.npts) continue;
                const double* ps = scr + pp * G::PSCR;
                double rsum = -ps[VEC + 2 * DP + k] - ps[VEC + 3 * DP + k];
                for (int d = 0; d < Do; ++d) rsum = fma(ps[HBS + d * DP + k], fmv[pp * 16 + d], rsum);
                const bool bad = (cst[pp * 4 + 2] + cst[pp * 4 + 3]) != 0.0;
                a.gmean[p * D + k] = bad ? __builtin_nan("") : -rsum * il[k];
                if (k == 0 && a.info) a.info[p] = (cst[pp * 4 + 2] != 0.0) ? 1.0 : cst[pp * 4 + 3];
            }
            if (a.gcov) {
                for (int it = tid; it < PG * LT; it += NT) {
                    const int pp = it / LT, q = it - pp * LT;
                    const int i = q / DP, j = q - i * DP;
                    const int64_t p = pbase + pp;
                    if (i >= D || j >= D || p >= a.npts) continue;
                    const double* ps = scr + pp * G::PSCR;
                    const bool bad = (cst[pp * 4 + 2] + cst[pp * 4 + 3]) != 0.0;
                    double val = 0.0;
                    if (j <= i) {
                        double sij = 0.5 * ps[MX + j * DP + i] + ps[MX + LT + j * DP + i];
                        double sji = 0.5 * ps[MX + i * DP + j] + ps[MX + LT + i * DP + j];
                        for (int d = 0; d < Do; ++d) {
                            const double ci = ps[YHS + d * DP + i] - ps[HBS + d * DP + i];
                            const double cj = ps[YHS + d * DP + j] - ps[HBS + d * DP + j];
                            sij = fma(ci, ps[AHS + d * DP + j], sij);
                            sji = fma(cj, ps[AHS + d * DP + i], sji);
                        }
                        val = ((i == j) ? sij : (sij + sji)) * il[i] * il[j];
                    }
                    a.gcov[(p * D + i) * D + j] = bad ? __builtin_nan("") : val;
                }
            }
        }
    }
}

template <int NBLK, int DK>
int launch_gp_mmb_k(const GpMmBwdArgs& a, unsigned nwg, hipStream_t st)
{
    typedef GpBwdCfg<NBLK> C;
    const size_t lds = size_t(GpMmBwdGeom<NBLK, DK>::LDS_DOUBLES) * sizeof(double);
    auto k = gp_moment_match_bwd_kernel<NBLK, C::RB, DK>;
    int rc = set_lds(k, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k, dim3(nwg), dim3(64 * C::W), lds, st, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -int(e) - 1000;
}

template <int NBLK>
int launch_gp_mmb_n(int DK, const GpMmBwdArgs& a, unsigned nwg, hipStream_t st)
{
    switch (DK) {
        case 2: return launch_gp_mmb_k<NBLK, 2>(a, nwg, st);
        case 4: return launch_gp_mmb_k<NBLK, 4>(a, nwg, st);
        case 6: return launch_gp_mmb_k<NBLK, 6>(a, nwg, st);
    }
    return -2;
}

}  // namespace cbfssm

#define CBF_GPMMB_DECLARE(NB)                                                                    \
    namespace cbfssm {                                                                           \
    int launch_gp_mmb_nb##NB(int DK, const GpMmBwdArgs& a, unsigned nwg, hipStream_t st);        \
    }

#define CBF_GPMMB_INSTANTIATE(NB)                                                                \
    namespace cbfssm {                                                                           \
    int launch_gp_mmb_nb##NB(int DK, const GpMmBwdArgs& a, unsigned nwg, hipStream_t st)         \
    {                                                                                            \
        return launch_gp_mmb_n<NB>(DK, a, nwg, st);                                              \
    }                                                                                            \
    }
