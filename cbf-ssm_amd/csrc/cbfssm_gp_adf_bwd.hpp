// The adjoint of GPModel.adf (gp_adf_kernel, cbfssm_gp_adf.hpp) with respect to the inputs of the call -- m0, P0, a, y, var_x
// and var_y; the model is a constant -- from the cotangents of means, covs and loglik: the whole time loop in ONE launch, one
// workgroup per 16 chains, the steps in reverse.  The forward saves nothing new: pmeans, pcovs, means and covs are its
// results, and the moments of the GP are recomputed by the adjoint of moment_match itself.
//
// A step t, with (mb, Pb) the adjoint of the belief behind it (Pb symmetric; an incoming covs cotangent is symmetrised once):
//
//   U  (VALU, gp_ekf_bwd_kernel's lane mapping: one lane per (chain, row), 16 lanes side by side are a chain, wave barriers
//      only, three [16][16][17] tiles and three [16][17] vectors over region A of the chain phase, dead behind a barrier)
//        carry  of step t + 1, where there is one: mb = mb- + gmean[:Do];  ga[t + 1] = gmean[Do:];
//               Pb = Pb- + unfold(gcov[:Do, :Do]) (a strictly lower entry halved and mirrored); then + gmeans[t], sym(gcovs[t])
//        S1     the Dy scalar updates again from pmeans[t], pcovs[t], keeping g_j = P[:, j] / s_j, s_j, delta_j
//        S2     their adjoint, last update first, formula for formula gp_ekf_bwd_kernel's: gy[t], the var_y sum, (mb-, Pb-)
//        T      m- = m + f, P- = P + Cx + Cx^T + F + diag(var_x):  the var_x sum += diag Pb-;  the direct terms mb-, Pb- wait
//               in the lane's own 17 doubles of `work`;  the moment-match problem of the step is staged as plain arrays in
//               the workgroup's block of `work`:  x = concat(means[t - 1], a[t]) (16, D),  S = blockdiag(covs[t - 1], 0)
//               (16, D, D)  ((m0, P0) at t = 0),  gfmean = mb-,  gfcov = Pb-,  gxcov = [2 Pb- | 0]
//   G  the per-pair body of gp_moment_match_bwd_kernel (steps 0 to 10, restated below as gp_adfb_pair), eight pairs, on those
//      arrays; gmean (16, D) and gcov (16, D, D), lower-triangle convention, go back to the block
//
// Behind the loop the carry of step 0 is the result: gm0 = mb, ga[0], gP0 = fold(Pb) -- twice the strictly lower entries, the
// diagonal as it is, explicit zeros above.  The var_x and var_y sums of a workgroup go to its slot of `work` and a second,
// tiny launch adds the slots in the order of the workgroups.  No atomics, no spin waits, workgroup barriers only, one writer
// per entry: two calls are bitwise identical and a chain's gradients do not depend on the other chains of the call.
// info[n] != 0 (the forward flagged the chain): its U lanes run on zeros, its staged problem is zero, its rows of gm0, gP0, ga
// and gy are NaN by select and both variance sums are NaN.  Chains >= N run on zeros and store nothing.  A y entry at
// cond = 0 is chosen away by a select and may be NaN; its gradient is exactly 0.
#pragma once
#include "../../include/cbfssm_hip.h"
#include "cbfssm_gp_bwd.hpp"
#include "cbfssm_gp_mm_bwd.hpp"

namespace cbfssm {

struct GpAdfBwdArgs {
    GpMmBwdArgs mm;          // the pack's sections, alpha, the W_d tiles, M, D, Do; the arrays are the workgroup's, set in the kernel
    const double* m0;        // (N, Do)
    const double* P0;        // (N, Do, Do), lower triangle read, or null: zero
    const double* a;         // (T, N, D - Do)
    const double* y;         // (T, N, Dy)
    const double* cond;      // (T, N) 0 / 1 or null
    const double* var_y;     // (Dy)
    const double* means;     // (T, N, Do)      as the forward left them
    const double* covs;      // (T, N, Do, Do)
    const double* pmeans;    // (T, N, Do)
    const double* pcovs;     // (T, N, Do, Do)
    const double* info;      // (N)
    const double* gmeans;    // (T, N, Do) or null
    const double* gcovs;     // (T, N, Do, Do) or null (need not be symmetric)
    const double* gloglik;   // (N) or null
    double* gm0;             // (N, Do)
    double* gP0;             // (N, Do, Do) or null
    double* ga;              // (T, N, D - Do)
    double* gy;              // (T, N, Dy)
    double* block;           // [workgroup][gp_adfb_block]
    double* sums;            // [workgroup][32]   d / d var_x by state dimension, then d / d var_y
    int N, T, Dy;
};

// doubles of one workgroup's block of `work`: the chain phase's scratch, the staged problem (x, S, gfmean, gfcov, gxcov), its
// results (gmean, gcov), and per (chain, row) lane the row of Pb- and the entry of mb- that wait for the next step
constexpr int64_t gp_adfb_block(int NBLK, int DK)
{
    return gp_mmb_scratch(NBLK, DK) + 2 * (16 * 4 * DK + 16 * 16 * DK * DK) + 256 + 4096 + 256 * 4 * DK + 4096 + 256;
}

// LDS: region A | L2 | region B of GpMmBwdGeom, region A widened to the U phase's tiles where those are larger.  At 20 row
// blocks and DK 6 region A is the chain phase's 15 360 doubles, the tiles take 13 872, and 112 doubles of the CU's LDS are left.
template <int NBLK, int DK>
struct GpAdfBwdGeom {
    typedef GpMmBwdGeom<NBLK, DK> G;
    static constexpr int PD = 17;
    static constexpr int CT = 16 * 16 * PD;
    static constexpr int UT = 3 * CT + 3 * 16 * PD;
    static constexpr int RA = G::RA > UT ? G::RA : UT;
    static constexpr int LDS_DOUBLES = RA + G::PG * G::LT + G::RBD;
    static constexpr int IL = 3 * G::PG * G::LT + 3 * G::PG * G::DP + 2 * G::PG * G::MP + 4 * G::PG;   // 1 / l, from the L2 block
    static constexpr int64_t XS = G::SCRATCH, SS = XS + 16 * G::DP, GF = SS + 16 * G::LT, GC = GF + 256, GX = GC + 4096;
    static constexpr int64_t GM = GX + 256 * G::DP, GS = GM + 16 * G::DP, WP = GS + 16 * G::LT, WM = WP + 4096;
    static constexpr int64_t BLOCK = WM + 256;
    static_assert(BLOCK == gp_adfb_block(NBLK, DK), "block sections");
    static_assert(UT >= 2 * 64 * G::C::W, "the variance sums go through region A");
    static_assert(LDS_DOUBLES <= 163840 / 8, "LDS budget");
};

__device__ __forceinline__ double adfb_red16(double v)
{
    v += __shfl_xor(v, 8, 16);
    v += __shfl_xor(v, 4, 16);
    v += __shfl_xor(v, 2, 16);
    v += __shfl_xor(v, 1, 16);
    return v;
}

// Steps 0 to 10 of gp_moment_match_bwd_kernel (cbfssm_gp_mm_bwd.hpp) for the pair of points pbase, pbase + 1 of the arrays in
// `a`, restated line for line as cbfssm_gp_adf.hpp restates the forward's: lifting the text out of that kernel into a shared
// __device__ template changed the registers and the scratch of its 24 instantiations, so that header stays as it is.  `lds`
// is region A and `rb` the L2 block with region B behind it; `scr` is the workgroup's scratch.  ok, rbs, alj and czj are the
// wave's row blocks with their alpha rows and exponent terms, loaded once per launch by the caller, which also fills il and
// holds the workgroup barrier that frees the LDS and the scratch of the previous pair.
template <int NBLK, int RB, int DK>
__device__ __forceinline__ void gp_adfb_pair(const GpMmBwdArgs& a, const int64_t pbase, double* lds, double* rb, double* scr,
                                            const bool (&ok)[RB], const int (&rbs)[RB], const double (&alj)[RB][4],
                                            const double (&czj)[RB], const double sig2, const double logv)
{
    typedef GpMmBwdGeom<NBLK, DK> G;
    constexpr int W = (NBLK + RB - 1) / RB, NT = 64 * W, MP = G::MP, DP = G::DP, JB = G::JB, JD = G::JD, PG = G::PG;
    constexpr int UOP = G::UOP, LT = G::LT, SB = G::SB, H = G::H;
    // sections of a point's scratch
    constexpr int64_t XW = 0, EROW = XW + int64_t(W) * LT, HR = EROW + int64_t(H + 1) * MP, AHS = HR + 16 * DP;
    constexpr int64_t YHS = AHS + 16 * DP, HBS = YHS + 16 * DP, G2 = HBS + 16 * DP, GWU = G2 + LT, P12 = GWU + 2 * LT;
    constexpr int64_t MX = P12 + 2 * LT, VEC = MX + 2 * LT;
    static_assert(VEC + 4 * DP == G::PSCR, "scratch sections");

    double* Uop = lds;                                  // [PG][NBLK][DK][64]
    double* slot = lds;                                 // [W][PG][SB], over the above
    double* img = lds;                                  // [PG][MP][DP], over the above
    double* L2t = rb;                                   // [PG][DP][DP]
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
    static_assert(GpAdfBwdGeom<NBLK, DK>::IL == 3 * PG * LT + 3 * PG * DP + 2 * PG * MP + 4 * PG, "il behind the L2 block");

    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, g = l >> 4, nl = l & 15;
    const int M = a.M, D = a.D, Do = a.Do;
    const bool haveC = a.gfcov != nullptr;

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

template <int NBLK, int RB, int DK>
__global__ __launch_bounds__(64 * ((NBLK + RB - 1) / RB)) void gp_adf_bwd_kernel(GpAdfBwdArgs a)
{
    typedef GpAdfBwdGeom<NBLK, DK> A;
    typedef GpMmBwdGeom<NBLK, DK> G;
    constexpr int W = (NBLK + RB - 1) / RB, NT = 64 * W, MP = G::MP, DP = G::DP, PG = G::PG, PD = A::PD, CT = A::CT;
    constexpr int TPT = (256 + NT - 1) / NT;            // (chain, row) lanes per thread

    extern __shared__ double lds[];
    double* rb = lds + A::RA;
    double* il = rb + A::IL;                            // [DP]
    double* tA = lds;                                   // U phase: P- of S1
    double* tB = tA + CT;                               //   g_j of S1 / S2
    double* tD = tB + CT;                               //   the rows of the covariance adjoint
    double* sS = tD + CT;                               //   s_j     [n][j]
    double* sD = sS + 16 * PD;                          //   delta_j [n][j]
    double* hv = sD + 16 * PD;                          //   gb / 2 s [n][i]

    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, g = l >> 4, nl = l & 15;
    const int D = a.mm.D, Do = a.mm.Do, Dy = a.Dy, N = a.N, T = a.T;
    const int Da = D - Do;
    const int64_t p0 = int64_t(blockIdx.x) * 16;
    const double sig2 = a.mm.scal[CBFSSM_SCAL_SIGMA2];
    const double logv = log(sig2);
    const double nan = __builtin_nan("");
    double* blk = a.block + int64_t(blockIdx.x) * A::BLOCK;

    // the chain phase's view of the block: a call of 16 points
    double* sx = blk + A::XS;                           // (16, D)
    double* sc = blk + A::SS;                           // (16, D, D)
    double* sgf = blk + A::GF;                          // (16, Do)
    double* sgC = blk + A::GC;                          // (16, Do, Do)
    double* sgX = blk + A::GX;                          // (16, Do, D)
    GpMmBwdArgs b = a.mm;
    b.mean = sx; b.cov = sc; b.gfmean = sgf; b.gfcov = sgC; b.gxcov = sgX;
    b.gmean = blk + A::GM; b.gcov = blk + A::GS; b.info = nullptr; b.scratch = blk; b.npts = 16; b.nblocks = 1;

    bool ok[RB];
    int rbs[RB];
    double alj[RB][4], czj[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        ok[i] = (w * RB + i) < NBLK;
        rbs[i] = ok[i] ? (w * RB + i) : (NBLK - 1);
#pragma unroll
        for (int r = 0; r < 4; ++r) alj[i][r] = a.mm.alpha[nl * MP + 16 * rbs[i] + 4 * r + g];
        czj[i] = 0.5 * (a.mm.cz[16 * rbs[i] + nl] - logv);
    }
    for (int i = tid; i < DP; i += NT) il[i] = a.mm.invl[i];        // (made visible by the barrier of the first pair)
    double gvx = 0.0, gvy = 0.0;                        // sums of diag Pb- and of sb over this thread's (chain, dim = tid & 15) lanes

    for (int t = T - 1; t >= 0; --t) {
        __syncthreads();                                // the later step's gmean and gcov are whole; region A is free
        const bool first = (t == T - 1);
        const double* mprev = t > 0 ? a.means + int64_t(t - 1) * N * Do : a.m0;
        const double* Pprev = t > 0 ? a.covs + int64_t(t - 1) * N * Do * Do : a.P0;

        // ---- U: whole waves (lane ids < 256), a chain's 16 lanes side by side.  Every row lives in LDS and the loops over the
        // columns are rolled, as in gp_ekf_bwd_kernel
#pragma unroll 1
        for (int k2 = 0; k2 < TPT; ++k2) {
            const int id = tid + k2 * NT;
            if (id < 256) {                             // (wave uniform: 256 is a multiple of 64)
                const int n = id >> 4, i = id & 15;
                const int64_t p = p0 + n;
                const bool valid = p < N;
                const bool dead = valid && a.info[p] != 0.0;
                const bool live = valid && !dead;
                const bool act = live && (i < Do);
                const int64_t pc = valid ? p : 0;
                const int64_t tn = int64_t(t) * N + pc;
                const int64_t ob = tn * Do, o = ob + i;
                double* wPr = blk + A::WP + id * 16;
                double* wMr = blk + A::WM + id;
                const double* gmr = b.gmean + n * D;
                const double* gcr = b.gcov + n * D * D;
                double* Pw = tA + n * 16 * PD;
                double* Gt = tB + n * 16 * PD;
                double* Pb = tD + n * 16 * PD;          // row i: this lane's row of the covariance adjoint
                const bool dc = live && (a.cond ? (a.cond[tn] != 0.0) : true);
                const double ll = (a.gloglik && live) ? a.gloglik[p] : 0.0;

                // the carry of step t + 1, then this step's cotangents
                double mb = 0.0;
                if (!first) {
                    mb = wMr[0] + (act ? gmr[i] : 0.0);
                    if (valid) {
                        double* gar = a.ga + (int64_t(t + 1) * N + p) * Da;
                        for (int k = i; k < Da; k += 16) gar[k] = dead ? nan : gmr[Do + k];
                    }
                }
                if (a.gmeans && act) mb += a.gmeans[o];
#pragma unroll 2
                for (int q = 0; q < 16; ++q) {
                    const bool in = act && q < Do;
                    double v = 0.0;
                    if (!first) {
                        v = wPr[q];
                        if (in) v += (q == i) ? gcr[i * D + i] : 0.5 * ((q < i) ? gcr[i * D + q] : gcr[q * D + i]);
                    }
                    if (a.gcovs && in) v += 0.5 * (a.gcovs[o * Do + q] + a.gcovs[(ob + q) * Do + i]);
                    Pb[i * PD + q] = v;
                    Pw[i * PD + q] = in ? a.pcovs[o * Do + q] : 0.0;
                }

                // S1: the scalar updates of the forward step again (row j is not read after update j: its lane leaves it)
                {
                    double mi = act ? a.pmeans[o] : 0.0;
                    const double yv = (live && i < Dy) ? a.y[tn * Dy + i] : 0.0;
                    __builtin_amdgcn_wave_barrier();
#pragma unroll 1
                    for (int j = 0; j < Dy; ++j) {
                        const double* rj = Pw + j * PD;
                        const double s = rj[j] + a.var_y[j];
                        const double pij = rj[i];
                        const double rs = 1.0 / s;
                        const double dl = __shfl(yv, j, 16) - __shfl(mi, j, 16);
                        const double gi = pij * rs;
                        Gt[j * PD + i] = gi;
                        if (i == 0) {
                            sS[n * PD + j] = s;
                            sD[n * PD + j] = dc ? dl : 0.0;
                        }
                        mi = dc ? mi + gi * dl : mi;
                        if (dc && i != j) {
#pragma unroll 4
                            for (int q = 0; q < 16; ++q) Pw[i * PD + q] -= (pij * rj[q]) * rs;
                        }
                        __builtin_amdgcn_wave_barrier();
                    }
                }

                // S2: their adjoint, last update first
                double gyv = 0.0;
#pragma unroll 1
                for (int j = Dy - 1; j >= 0; --j) {
                    const double* gr = Gt + j * PD;
                    const double s = sS[n * PD + j], dl = sD[n * PD + j];
                    const double rs = 1.0 / s;
                    const double gi = gr[i];
                    double u = 0.0;
#pragma unroll 4
                    for (int q = 0; q < 16; ++q) u = fma(Pb[i * PD + q], gr[q], u);
                    const double gPg = adfb_red16(gi * u);
                    const double gm = adfb_red16(gi * mb);
                    const double gb = dl * mb - 2.0 * s * u;
                    const double gbg = adfb_red16(gb * gi);
                    const double db = gm - ll * dl * rs;
                    const double sb = 0.0 - gPg - gbg * rs - 0.5 * ll * (rs - dl * dl * rs * rs);
                    const double h = dc ? 0.5 * gb * rs : 0.0;
                    const bool me = (i == j);
                    hv[n * PD + i] = h;
                    __builtin_amdgcn_wave_barrier();
                    if (me) {                           // row j: the mirror of the column, the own entry twice, and sb
#pragma unroll 4
                        for (int q = 0; q < 16; ++q) Pb[i * PD + q] += hv[n * PD + q];
                        Pb[i * PD + j] += h + (dc ? sb : 0.0);
                        if (dc) {
                            mb -= db;
                            gyv = db;
                            gvy += sb;
                        }
                    } else {
                        Pb[i * PD + j] += h;
                    }
                    __builtin_amdgcn_wave_barrier();
                }
                if (valid && i < Dy) a.gy[tn * Dy + i] = dead ? nan : gyv;

                // T: the var_x sum, the direct terms, and the moment-match problem of this step
                gvx += Pb[i * PD + i];
                if (dead) { gvx = nan; gvy = nan; }
                wMr[0] = mb;
#pragma unroll 4
                for (int q = 0; q < 16; ++q) wPr[q] = Pb[i * PD + q];
                if (i < Do) {
                    sx[n * D + i] = act ? mprev[pc * Do + i] : 0.0;
                    sgf[n * Do + i] = act ? mb : 0.0;
                    double* gC = sgC + (n * Do + i) * Do;
                    double* gX = sgX + (n * Do + i) * D;
#pragma unroll 1
                    for (int q = 0; q < D; ++q) {
                        const double v = (act && q < Do) ? Pb[i * PD + (q < 16 ? q : 0)] : 0.0;
                        if (q < Do) gC[q] = v;
                        gX[q] = 2.0 * v;
                    }
                }
                for (int k = i; k < Da; k += 16)
                    sx[n * D + Do + k] = live ? a.a[tn * Da + k] : 0.0;
                for (int r = i; r < D; r += 16) {       // rows i and 16 + i of S = blockdiag(P, 0)
                    double* sr = sc + (n * D + r) * D;
                    const bool in = live && r < Do && Pprev != nullptr;
#pragma unroll 1
                    for (int q = 0; q < D; ++q) {
                        double v = 0.0;
                        if (in && q < Do) v = (q <= r) ? Pprev[(pc * Do + r) * Do + q] : Pprev[(pc * Do + q) * Do + r];
                        sr[q] = v;
                    }
                }
            }
        }

        // ==== G: the input adjoint of moment_match on the staged problem, two chains at a time
        for (int pgi = 0; pgi < 16 / PG; ++pgi) {
            if (p0 + pgi * PG >= N) break;
            __syncthreads();                            // the staged arrays are whole; the previous pair's readers are done
            gp_adfb_pair<NBLK, RB, DK>(b, int64_t(pgi * PG), lds, rb, blk, ok, rbs, alj, czj, sig2, logv);
        }
    }
    __syncthreads();

    // ---- the carry of step 0 is the result: gm0, ga[0], gP0 = fold(Pb)
    if (T > 0) {
#pragma unroll 1
        for (int k2 = 0; k2 < TPT; ++k2) {
            const int id = tid + k2 * NT;
            if (id < 256) {
                const int n = id >> 4, i = id & 15;
                const int64_t p = p0 + n;
                if (p < N) {
                    const bool dead = a.info[p] != 0.0;
                    const double* wPr = blk + A::WP + id * 16;
                    const double* gmr = b.gmean + n * D;
                    const double* gcr = b.gcov + n * D * D;
                    if (i < Do) a.gm0[p * Do + i] = dead ? nan : blk[A::WM + id] + gmr[i];
                    for (int k = i; k < Da; k += 16) a.ga[p * Da + k] = dead ? nan : gmr[Do + k];
                    if (a.gP0 && i < Do) {              // the function of tril(P0) + tril(P0, -1)^T
                        double* gp = a.gP0 + (p * Do + i) * Do;
#pragma unroll 1
                        for (int q = 0; q < Do; ++q) {
                            const double v = (q < i) ? 2.0 * wPr[q] + gcr[i * D + q] : ((q == i) ? wPr[i] + gcr[i * D + i] : 0.0);
                            gp[q] = dead ? nan : v;
                        }
                    }
                }
            }
        }
    }

    // ---- this workgroup's variance sums, over its chains in a fixed order
    lds[tid] = gvx;
    lds[NT + tid] = gvy;
    __syncthreads();
    if (tid < 32) {
        const double* r = lds + ((tid < 16) ? 0 : NT) + (tid & 15);
        double s = 0.0;
        for (int k = 0; k < NT / 16; ++k) s += r[16 * k];
        a.sums[int64_t(blockIdx.x) * 32 + tid] = s;
    }
}

template <int NBLK, int DK>
int launch_gp_adfb_k(const GpAdfBwdArgs& a, hipStream_t st)
{
    typedef GpBwdCfg<NBLK> C;
    const size_t lds = size_t(GpAdfBwdGeom<NBLK, DK>::LDS_DOUBLES) * sizeof(double);
    auto k = gp_adf_bwd_kernel<NBLK, C::RB, DK>;
    int rc = set_lds(k, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k, dim3(unsigned((a.N + 15) / 16)), dim3(64 * C::W), lds, st, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -int(e) - 1000;
}

template <int NBLK>
int launch_gp_adfb_n(int DK, const GpAdfBwdArgs& a, hipStream_t st)
{
    switch (DK) {
        case 2: return launch_gp_adfb_k<NBLK, 2>(a, st);
        case 4: return launch_gp_adfb_k<NBLK, 4>(a, st);
        case 6: return launch_gp_adfb_k<NBLK, 6>(a, st);
    }
    return -2;
}

}  // namespace cbfssm

#define CBF_GPADFB_DECLARE(NB)                                                                   \
    namespace cbfssm {                                                                           \
    int launch_gp_adfb_nb##NB(int DK, const GpAdfBwdArgs& a, hipStream_t st);                    \
    }

#define CBF_GPADFB_INSTANTIATE(NB)                                                               \
    namespace cbfssm {                                                                           \
    int launch_gp_adfb_nb##NB(int DK, const GpAdfBwdArgs& a, hipStream_t st)                     \
    {                                                                                            \
        return launch_gp_adfb_n<NB>(DK, a, st);                                                  \
    }                                                                                            \
    }
