// Adjoint of the extended Kalman filter over one sparse GP (gp_ekf_kernel, cbfssm_gp_ekf.hpp): d loss / d (m0, P0, a, y,
// var_x, var_y and the GP parameters) from the cotangents of means, covs and loglik, the whole time loop in ONE launch, one
// workgroup per 16 chains, the steps in reverse.  The forward under grad (the EMIT / SAVEJ form of gp_ekf_kernel) leaves per
// step m- (pmeans), P- (pcovs), A P (cross) and the Jacobian J (jac); the kernel tile and A2 = K^-1 k are recomputed.
//
// A step, with (mb, Pb) the adjoint of the belief behind it (Pb symmetric; an incoming covs cotangent is symmetrised once):
//
//   covariance part (VALU, the forward's lane mapping: one lane per (chain, row), 16 lanes side by side are a chain, wave
//   barriers only; every row lives in LDS inside the part, with rolled loops over the columns, and Pb in a per-lane row of
//   `work` between two steps; the lane id is made opaque once per step so that no address term of the part is hoisted out
//   of the time loop and held in registers across the GP part -- that, not the rows, is what spilled)
//     S1  the Dy scalar updates again from m-, P-, keeping g_j = P[:, j] / s_j, s_j, delta_j
//     S2  j = Dy - 1 .. 0 where cond:  u = Pb g;  gb = delta mb - 2 s u;  db = g^T mb - lb delta / s
//                                      sb = -g^T u - gb^T g / s - lb (1 / s - delta^2 / s^2) / 2
//                                      mb[j] -= db;  gy[t][j] = db;  gvar_y[j] += sb;  Pb += sym((gb / s) e_j^T) + sb e_j e_j^T
//     T1  Fm = mb;  Fv = diag Pb (also d / d var_x);  Jb = 2 Pb (A P);  Jh[d][i] = Jb[d][i] / l_i
//         xsub[i] = sum_d Jh[d][i] fmean[d];  jj[i] = sum_d Jb[d][i] J[d][i]          (x~bar and lengthscale terms of J)
//     T2  B = Pb A;  Pb <- A^T B as the lower triangle plus its mirror (bitwise symmetric)
//
//   GP part (f64 MFMA): phases B to G of gp_filter_bwd_kernel.  B, C, E, the tail of F and the slab write are the shared body of
//   cbfssm_gp_tile.hpp (GpWave); phase F keeps its own text around the shared products and transposes, for the terms of Jb:
//     C_d[m][n] = sum_i Jh_n[d][i] (Z~[m][i] - x~[i][n])      per output dimension d, DK MFMAs per row block
//     alphabar[m][d] += sum_n k[m][n] C_d[m][n];   Kbar += sum_d alpha[m][d] C_d   before Ebar = Kbar o K
//     Zbar~[m][i] += sum_d sum_n (alpha[m][d] k[m][n]) Jh_n[d][i];   x~bar[i][n] -= xsub;   lengthscale sum += jj
//   The state rows of the input adjoint plus Fm are the next mb (gm0 at the first step), the other rows ga[t].
//
// alpha = K^-1 mu is explicit in the forward, so alphabar is folded once per launch: mubar += K^-1 alphabar and
// Kinvbar += alphabar mu^T (the slab's section, or one more stash slot per workgroup at stash heights).
// No atomics, no spin waits, one writer per output entry: two calls are bitwise identical.  Padded chains carry zero
// adjoints and the rows m >= M of every tile are zero: both contribute exact zeros.  A y entry at cond = 0 is chosen away
// by a select and may be NaN.
#pragma once
#include "../../include/cbfssm_hip.h"
#include "cbfssm_gp_bwd.hpp"

namespace cbfssm {

struct GpEkfBwdArgs {
    PackPtrs pk;
    RevPackPtrs rk;
    const double* m0;        // (N, Do)
    const double* a;         // (T, N, D - Do)
    const double* y;         // (T, N, Dy)
    const double* cond;      // (T, N) 0 / 1 or null
    const double* var_y;     // (Dy)
    const double* alpha;     // [16][16 NBLK]  (K^-1 mu)[m][d] at [d][m]
    const double* means;     // (T, N, Do)
    const double* pmeans;    // (T, N, Do)
    const double* pcovs;     // (T, N, Do, Do)
    const double* cross;     // (T, N, Do, Do)
    const double* jac;       // (T, N, Do, Do)  J[d][i]
    const double* gmeans;    // (T, N, Do) or null
    const double* gcovs;     // (T, N, Do, Do) or null (need not be symmetric)
    const double* gloglik;   // (N) or null
    double* gm0;             // (N, Do)
    double* gP0;             // (N, Do, Do) or null
    double* ga;              // (T, N, D - Do)
    double* gy;              // (T, N, Dy)
    double* gpart;           // [workgroup][slab]
    int64_t slab;
    double* stash_a;         // stash heights: [slot][NBLK][4][64]; slot = workgroup T + step, the fold at fold_slot0 + workgroup
    double* stash_k;
    int64_t fold_slot0;
    double* wP;              // [workgroup][256 lanes][16]   the lanes' rows of Pb between two steps
    double* wJ;              // [workgroup][16 d][16 i][16 n] Jh of the current step
    int N, T, M, D, Do, Dy;
};

// LDS: xq | Fm | Fv | carry | xsub | jj | red | 1 / l | overlay.  The overlay is the GP part's Kt | A2t | part, or the
// covariance part's four [16][16][17] tiles (P- / new Pb; g_j / A P / B; J; Pb) and three [16][17] vectors, which is the
// larger at every height: 20 080 doubles at DK 6 (157 KB), one workgroup per CU.
template <int NBLK, int DK>
struct GpEkfBwdGeom {
    typedef GpBwdCfg<NBLK> C;
    static constexpr int JB = (4 * DK + 1 + 15) / 16;
    static constexpr int PD = 17;
    static constexpr int MP = 16 * NBLK;
    static constexpr int PSL = JB * 256;
    static constexpr int CT = 16 * 16 * PD;
    static constexpr int SMALL = 4 * DK * PD + 5 * 16 * PD + 64 + 4 * DK;
    static constexpr int GP = 2 * MP * PD + C::W * PSL;
    static constexpr int COV = 4 * CT + 3 * 16 * PD;
    static constexpr int LDS_DOUBLES = SMALL + (GP > COV ? GP : COV);
    static_assert(LDS_DOUBLES <= 163840 / 8, "LDS budget");
    static_assert(C::W * PSL >= 2 * 64 * C::W, "the var_x / var_y sums go through the partial tiles");
};

__device__ __forceinline__ double ekf_red16(double v)
{
    v += __shfl_xor(v, 8, 16);
    v += __shfl_xor(v, 4, 16);
    v += __shfl_xor(v, 2, 16);
    v += __shfl_xor(v, 1, 16);
    return v;
}

template <int NBLK, int RB, int DK, bool STASH>
__global__ __launch_bounds__(64 * ((NBLK + RB - 1) / RB)) void gp_ekf_bwd_kernel(GpEkfBwdArgs a)
{
    typedef GpEkfBwdGeom<NBLK, DK> G;
    typedef GpWave<NBLK, RB, DK> WV;
    constexpr int W = WV::W, NT = WV::NT, MP = WV::MP;
    constexpr int JB = G::JB;
    constexpr int NG = 4 * JB;                          // 4-row groups of the input-adjoint tile
    constexpr int GPW = (NG + W - 1) / W;               // groups per wave in phase G
    constexpr int PD = 17, PSL = G::PSL, CT = G::CT;
    constexpr int TPT = (256 + NT - 1) / NT;            // (chain, row) lanes per thread
    constexpr int SJ = (DK < 4) ? DK : 4;               // k-steps that hold state columns (Do <= 16)

    extern __shared__ double lds[];
    double* xq = lds;                                   // [4 DK][17] scaled inputs x~[j][n]
    double* Fm = xq + 4 * DK * PD;                      // [16][17]  d loss / d fmean [d][n]
    double* Fv = Fm + 16 * PD;                          // [16][17]
    double* carry = Fv + 16 * PD;                       // [16][17]  adjoint of the mean handed to the earlier step [d][n]
    double* xsub = carry + 16 * PD;                     // [16][17]  sum_d Jh[d][i] fmean[d]  at [i][n]
    double* jjt = xsub + 16 * PD;                       // [16][17]  sum_d Jb[d][i] J[d][i]   at [i][n]
    double* red = jjt + 16 * PD;                        // 64
    double* il = red + 64;                              // [4 DK]  1 / lengthscale
    double* ov = il + 4 * DK;
    double* Kt = ov;                                    // [MP][17]  kernel tile, then Ebar / Em transposes
    double* A2t = Kt + MP * PD;                         // [MP][17]  A2 transposes, then the A2bar tile
    double* part = A2t + MP * PD;                       // [W][PSL]  per-wave partial tiles of (Z~)^T Ebar
    double* tA = ov;                                    // covariance part: P- of S1, the new Pb of T2
    double* tB = tA + CT;                               //   g_j of S1 / S2, then A P, the product tiles, B
    double* tC = tB + CT;                               //   J
    double* sS = tC + CT;                               //   s_j     [n][j]
    double* sD = sS + 16 * PD;                          //   delta_j [n][j]
    double* hv = sD + 16 * PD;                          //   gb / 2 s [n][i]
    double* tD = hv + 16 * PD;                          //   the rows of the covariance adjoint inside the part

    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, g = l >> 4, nl = l & 15;
    const int M = a.M, D = a.D, Do = a.Do, Dy = a.Dy, N = a.N, T = a.T;
    const int Da = D - Do;
    const int64_t p0 = int64_t(blockIdx.x) * 16;
    double* wJb = a.wJ + int64_t(blockIdx.x) * 4096;

    WV wv;
    wv.setup(a.pk, tid);

    // ---- accumulators of the parameter adjoints (all steps of this workgroup)
    GpAdjAcc<NBLK, RB, JB, STASH> acc;
    acc.zero();
    d4 gAl[RB];                                         // alphabar, folded into mubar and Kinvbar behind the time loop
#pragma unroll
    for (int i = 0; i < RB; ++i) gAl[i] = d4{0, 0, 0, 0};
    double glx[GPW];
#pragma unroll
    for (int k2 = 0; k2 < GPW; ++k2) glx[k2] = 0.0;
    double gsig = 0.0, glogsig = 0.0;
    double gvx = 0.0, gvy = 0.0;                        // sums of Fv and of sb over this thread's (chain, dim = tid & 15) lanes
    double ilg[GPW];
#pragma unroll
    for (int k2 = 0; k2 < GPW; ++k2) {
        const int j = 4 * (w + k2 * W) + g;
        ilg[k2] = (j < D) ? a.pk.invl[j] : 0.0;
    }
    for (int i = tid; i < 4 * DK; i += NT) il[i] = a.pk.invl[i];
    for (int i = tid; i < 16 * PD; i += NT) { carry[i] = 0.0; xsub[i] = 0.0; jjt[i] = 0.0; }

    for (int sp = T - 1; sp >= 0; --sp) {
        const int t = sp;
        __syncthreads();                                // the previous step's readers of every tile are done; carry complete
        for (int i = tid; i < 4 * DK * 16; i += NT) {
            const int j = i >> 4, n = i & 15;
            const int64_t p = p0 + n;
            double v = 0.0;
            if (j < D && p < N) {
                if (j < Do) v = (sp == 0) ? a.m0[p * Do + j] : a.means[(int64_t(t - 1) * N + p) * Do + j];
                else v = a.a[(int64_t(t) * N + p) * Da + (j - Do)];
                v *= a.pk.invl[j];
            }
            xq[j * PD + n] = v;
        }

        // ---- the covariance part: whole waves (lane ids < 256), a chain's 16 lanes side by side.  Every row lives in LDS and
        // the loops over the columns are rolled: the part needs a handful of registers beside the accumulators of the GP part
#pragma unroll 1
        for (int k2 = 0; k2 < TPT; ++k2) {
            int id = tid + k2 * NT;
            asm volatile("" : "+v"(id));                // (per step: nothing derived from the lane id is kept across the GP part)
            if (id < 256) {                             // (wave uniform: 256 is a multiple of 64)
                const int n = id >> 4, i = id & 15;
                const int64_t p = p0 + n;
                const bool valid = p < N;
                const bool act = valid && (i < Do);
                const int64_t tn = int64_t(t) * N + (valid ? p : 0);
                const int64_t ob = tn * Do, o = ob + i;
                double* wPr = a.wP + (int64_t(blockIdx.x) * 256 + id) * 16;
                double* Pw = tA + n * 16 * PD;
                double* Gt = tB + n * 16 * PD;
                double* Jt = tC + n * 16 * PD;
                double* Pb = tD + n * 16 * PD;          // row i: this lane's row of the covariance adjoint
                const bool dc = valid && (a.cond ? (a.cond[tn] != 0.0) : true);
                const double ll = (a.gloglik && valid) ? a.gloglik[p] : 0.0;
                const bool first = (sp == T - 1);

                double mb = carry[i * PD + n];
                if (a.gmeans && act) mb += a.gmeans[o];
#pragma unroll 2
                for (int q = 0; q < 16; ++q) {
                    double v = first ? 0.0 : wPr[q];
                    if (a.gcovs && act && q < Do) v += 0.5 * (a.gcovs[o * Do + q] + a.gcovs[(ob + q) * Do + i]);
                    Pb[i * PD + q] = v;
                    Pw[i * PD + q] = (act && q < Do) ? a.pcovs[o * Do + q] : 0.0;
                }

                // S1: the scalar updates of the forward step again (row j is not read after update j: its lane leaves it)
                {
                    double mi = act ? a.pmeans[o] : 0.0;
                    const double yv = (valid && i < Dy) ? a.y[tn * Dy + i] : 0.0;
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
                    const double gPg = ekf_red16(gi * u);
                    const double gm = ekf_red16(gi * mb);
                    const double gb = dl * mb - 2.0 * s * u;
                    const double gbg = ekf_red16(gb * gi);
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
                if (valid && i < Dy) a.gy[tn * Dy + i] = gyv;

                // T1: the upstream adjoints of the GP and the terms of Jb = 2 Pb (A P)
                const double fvv = Pb[i * PD + i];
                Fm[i * PD + n] = mb;
                Fv[i * PD + n] = fvv;
                gvx += fvv;
                double* Ct = Gt;
#pragma unroll 2
                for (int q = 0; q < 16; ++q) {
                    const bool in = act && (q < Do);
                    Ct[i * PD + q] = in ? a.cross[o * Do + q] : 0.0;
                    Jt[i * PD + q] = in ? a.jac[o * Do + q] : 0.0;
                }
                double fmi = 0.0;
                if (act) fmi = a.pmeans[o] - ((sp == 0) ? a.m0[p * Do + i] : a.means[(int64_t(t - 1) * N + p) * Do + i]);
                __builtin_amdgcn_wave_barrier();
#pragma unroll 4
                for (int q = 0; q < 16; ++q) {
                    double jb = 0.0;
#pragma unroll
                    for (int k = 0; k < 16; ++k) jb = fma(Pb[i * PD + k], Ct[k * PD + q], jb);
                    jb *= 2.0;
                    const double jh = (q < 4 * DK) ? jb * il[q < 4 * DK ? q : 0] : 0.0;
                    wJb[(i * 16 + q) * 16 + n] = jh;
                    const double sx = ekf_red16(jh * fmi);              // sum over the chain's rows d = i
                    const double sj = ekf_red16(jb * Jt[i * PD + q]);
                    if (i == q) {
                        xsub[q * PD + n] = sx;
                        jjt[q * PD + n] = sj;
                    }
                }
                __builtin_amdgcn_wave_barrier();        // the chain's lanes have read A P

                // T2: Pb <- A^T Pb A, A = I + J
#pragma unroll 4
                for (int q = 0; q < 16; ++q) {
                    double bb = Pb[i * PD + q];
#pragma unroll
                    for (int k = 0; k < 16; ++k) bb = fma(Pb[i * PD + k], Jt[k * PD + q], bb);
                    Ct[i * PD + q] = bb;
                }
                __builtin_amdgcn_wave_barrier();
#pragma unroll 1
                for (int j = 0; j <= i; ++j) {
                    double v = Ct[i * PD + j];
#pragma unroll
                    for (int k = 0; k < 16; ++k) v = fma(Jt[k * PD + i], Ct[k * PD + j], v);
                    Pw[i * PD + j] = v;
                    Pw[j * PD + i] = v;
                }
                __builtin_amdgcn_wave_barrier();
                if (sp > 0) {
#pragma unroll 4
                    for (int q = 0; q < 16; ++q) wPr[q] = Pw[i * PD + q];
                } else if (a.gP0 && act) {              // the function of tril(P0) + tril(P0, -1)^T
                    double* gp = a.gP0 + (p * Do + i) * Do;
#pragma unroll 1
                    for (int q = 0; q < Do; ++q) {
                        const double v = Pw[i * PD + q];
                        gp[q] = (q < i) ? 2.0 * v : ((q == i) ? v : 0.0);
                    }
                }
            }
        }
        __syncthreads();                                // Fm, Fv, xsub, jj, Jh and xq are whole; the overlay is free

        // ---- B: kernel tile (rows of this wave)
        d4 kreg[RB];
        wv.kernel_tile(xq, Kt, M, kreg);
        __syncthreads();

        // ---- C: A2 rows of this wave (K^-1 streams from L2 as the A-operand image of the pack)
        d4 a2[RB];
        wv.image_times_tile(wv.bop, Kt, a2);

        // ---- E: A2bar, and the parameter adjoints that contract over the 16 chains; stash slot = workgroup * T + step
        GpUpstream up;
        wv.load_upstream(Fm, Fv, up, gsig);
        wv.template phase_E<STASH>(a.rk, up, Kt, A2t, a2, kreg, int64_t(blockIdx.x) * T + sp, a.stash_a, a.stash_k, acc);
        __syncthreads();

        // ---- F: Kbar with the terms of Jb (this kernel's own), then the shared Ebar, input adjoint partials, Zbar~
        d4 ebar[RB];
        {
            // the terms of Jb, one output dimension at a time (no prefetch, and the K^-1 product folded into kc first: the
            // loop's live registers are what spills at two row blocks per wave)
            d4 kc[RB];                                  // K^-1 A2bar - A2 colsum(Fv), then the terms of Jb on top
            wv.kbar(A2t, a2, up.fvsum, kc);
            double bxs[SJ];
#pragma unroll
            for (int s = 0; s < SJ; ++s) bxs[s] = xq[(4 * s + g) * PD + nl];
#pragma unroll 1
            for (int d = 0; d < Do; ++d) {
                double cB[SJ], cT[4];
                {
                    const double* src = wJb + d * 256;
#pragma unroll
                    for (int s = 0; s < SJ; ++s) cB[s] = src[(4 * s + g) * 16 + nl];            // B[k = i][col n]
#pragma unroll
                    for (int s = 0; s < 4; ++s) cT[s] = src[nl * 16 + 4 * s + g];               // B[k = n][col i]
                }
                double cx = 0.0;                        // sum_i Jh_n[d][i] x~[i][n]
#pragma unroll
                for (int s = 0; s < SJ; ++s) cx = fma(cB[s], bxs[s], cx);
                cx = gp_sum_groups(cx);
#pragma unroll
                for (int i = 0; i < RB; ++i) {
                    if (wv.ok[i]) {
                        d4 cd = {0.0 - cx, 0.0 - cx, 0.0 - cx, 0.0 - cx};
#pragma unroll
                        for (int s = 0; s < SJ; ++s) cd = CBF_MFMA(wv.Zreg[i][s], cB[s], cd);
                        const double* alp = a.alpha + d * MP + 16 * wv.rbs[i] + g;
                        d4 em;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const double al = alp[4 * r];
                            const double v = ekf_red16(kreg[i][r] * cd[r]);
                            gAl[i][r] += (nl == d) ? v : 0.0;                         // alphabar[m][d] += sum_n k C_d
                            kc[i][r] = fma(al, cd[r], kc[i][r]);
                            em[r] = al * kreg[i][r];
                        }
                        double emT[4];
                        double* ownk = Kt + 16 * wv.rbs[i] * PD;   // the K tile is dead behind the barrier that ends phase E
                        wv.store_c(ownk, em);
                        __builtin_amdgcn_wave_barrier();
                        wv.load_a(ownk, emT);
                        __builtin_amdgcn_wave_barrier();
#pragma unroll
                        for (int s = 0; s < 4; ++s) acc.gZ[i][0] = CBF_MFMA(emT[s], cT[s], acc.gZ[i][0]);   // Zbar~[m][i] += Em_d[m][n] Jh_n[d][i]
                    }
                }
            }
            wv.ebar_of(kc, kreg, M, ebar);
        }
        wv.phase_F_tail(a.rk.ZT, Kt, xq, part, ebar, D, acc.gZ);
        __syncthreads();

        // ---- G: input adjoint of this step: state rows + Fm -> carry (gm0 at the first step), the others -> ga[t]
        {
            const int64_t p = p0 + nl;
            const bool pvalid = p < N;
            double esum = 0.0;                          // colsum of Ebar for this lane's chain = row D of the xbar tile
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
                        if (j < Do) xb -= xsub[j * PD + nl];                       // x~ inside J
                        glx[k2] += xb * xt + ((j < Do) ? jjt[j * PD + nl] : 0.0);  // lengthscale adjoint (inputs, 1 / l of J)
                        const double gx = xb * ilg[k2];
                        if (j < Do) {
                            const double cv = gx + Fm[j * PD + nl];                // m enters m- directly and through the GP
                            if (sp == 0) a.gm0[p * Do + j] = cv;
                            else carry[j * PD + nl] = cv;
                        } else {
                            a.ga[(int64_t(t) * N + p) * Da + (j - Do)] = gx;
                        }
                    }
                    if (j == D && pvalid) glogsig += xb;
                }
            }
        }
    }

    // ---- alpha = K^-1 mu:  mubar += K^-1 alphabar,  Kinvbar += alphabar mu^T
    __syncthreads();
#pragma unroll
    for (int i = 0; i < RB; ++i)
        if (wv.ok[i]) {
#pragma unroll
            for (int r = 0; r < 4; ++r) Kt[(16 * wv.rbs[i] + 4 * r + g) * PD + nl] = gAl[i][r];
        }
    __syncthreads();
    wv.image_times_tile_fin(wv.bop, Kt, [&](int i, d4 f0, d4 f1) {
        if (wv.ok[i]) {
            acc.gMu[i] = acc.gMu[i] + f0 + f1;
            double abT[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) abT[s] = Kt[(16 * wv.rbs[i] + nl) * PD + 4 * s + g];   // A[row m'][k = d]
            if constexpr (STASH) {
                const int64_t slot = a.fold_slot0 + blockIdx.x;
                double* pa = a.stash_a + (slot * NBLK + wv.rbs[i]) * 256 + l;
                double* pk = a.stash_k + (slot * NBLK + wv.rbs[i]) * 256 + l;
                const double* mBp = a.rk.muB + wv.rbs[i] * 256 + l;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    pa[s * 64] = abT[s];
                    pk[s * 64] = mBp[s * 64];                                            // B[k = d][col m]
                }
            } else {
#pragma unroll
                for (int c2 = 0; c2 < NBLK; ++c2) {
                    const double* mBp = a.rk.muB + c2 * 256 + l;
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc.gB[i][c2] = CBF_MFMA(abT[s], mBp[s * 64], acc.gB[i][c2]);
                }
            }
        }
    });

    // ---- write this workgroup's slab
    __syncthreads();
    double* slab = a.gpart + int64_t(blockIdx.x) * a.slab;
    wv.template write_slab<STASH>(slab, acc);
    const double gv[2] = {gvx, gvy};                    // d loss / d var_x [0, 16) and d loss / d var_y [16, 32) by state dim
    wv.template write_state_sums<STASH>(slab, part, gv);
    wv.template write_sums<STASH>(slab, glx, gsig, glogsig, red);
}

template <int NBLK, int DK>
int launch_gp_ekf_bwd_k(const GpEkfBwdArgs& a, hipStream_t st)
{
    typedef GpBwdCfg<NBLK> C;
    const size_t lds = size_t(GpEkfBwdGeom<NBLK, DK>::LDS_DOUBLES) * sizeof(double);
    auto k = gp_ekf_bwd_kernel<NBLK, C::RB, DK, C::STASH>;
    int rc = set_lds(k, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k, dim3(unsigned((a.N + 15) / 16)), dim3(64 * C::W), lds, st, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -int(e) - 1000;
}

template <int NBLK>
int launch_gp_ekf_bwd_n(int DK, const GpEkfBwdArgs& a, hipStream_t st)
{
    switch (DK) {
        case 2: return launch_gp_ekf_bwd_k<NBLK, 2>(a, st);
        case 4: return launch_gp_ekf_bwd_k<NBLK, 4>(a, st);
        case 6: return launch_gp_ekf_bwd_k<NBLK, 6>(a, st);
    }
    return -2;
}

}  // namespace cbfssm

#define CBF_GPEKFBWD_DECLARE(NB)                                                                 \
    namespace cbfssm {                                                                           \
    int launch_gp_ekf_bwd_nb##NB(int DK, const GpEkfBwdArgs& a, hipStream_t st);                 \
    }

#define CBF_GPEKFBWD_INSTANTIATE(NB)                                                             \
    namespace cbfssm {                                                                           \
    int launch_gp_ekf_bwd_nb##NB(int DK, const GpEkfBwdArgs& a, hipStream_t st)                  \
    {                                                                                            \
        return launch_gp_ekf_bwd_n<NB>(DK, a, st);                                               \
    }                                                                                            \
    }
