// Extended Kalman filter over the transition of one sparse GP: a Gaussian belief (m, P) per chain, carried through time by
// the local linear model of GPModel.predict (gp_tf.py:132-161) in the recurrence of CBF-SSM (cbfssm.py:199-221), and
// conditioned on observations of the first Dy state dimensions (cbfssm.py:245-251), as ONE launch:
//
//   x = concat(m, a[t]);  f, fv = predict(x);  J = d fmean / d x [:, :Do];  A = I + J
//   m- = m + f;  P- = A P A^T + diag(fv + var_x)
//   where cond[t, n] != 0, for j = 0 .. Dy - 1 in this order (exact for the diagonal R = diag(var_y); no Dy x Dy solve):
//       s = P-[j][j] + var_y[j];  delta = y[t][n][j] - m-[j]
//       m- <- m- + P-[:, j] delta / s;  P-[i][k] <- P-[i][k] - (P-[i][j] P-[k][j]) / s;  loglik[n] -= (log(2 pi s) + delta^2 / s) / 2
//   m, P <- m-, P-;  means[t][n] = m;  covs[t][n] = P
//
// The GP part of a step is that of gp_linearize_kernel (cbfssm_gp_lin.hpp) without its variance Jacobian: the wave layout
// GpBwdCfg<NBLK> and, from the shared body (cbfssm_gp_tile.hpp, GpWave), the row-block setup, the kernel tile (phase B), A2
// and fvar0 in the form layout->gp_form asks for; per output dimension d Em_d = alpha_d o k and its (Z~)^T product, the
// waves' partial tiles summed in a fixed order.  What differs:
//
//   - one workgroup owns 16 chains for all T steps (the column block is fixed, the time loop is inside, as in
//     gp_rollout_kernel); the scaled GP input of the next step is written straight into the LDS operand tile xq;
//   - of the reduced tile only the state columns i < Do (the first input row block) and the ones row D (fmean) are
//     formed; they go to a Jacobian tile J[n][d][i] and to fm[d][n], fv[d][n] in LDS instead of to memory;
//   - the covariance tile P[n][i][k] stays in LDS for the whole launch.
//
// The covariance part of a step runs on the VALU, one lane per (chain n, row i): 16 lanes side by side hold one chain, so
// a chain never leaves its wave and the part needs no workgroup barrier inside:
//
//   C1  b[l] = sum_k A[i][k] P[k][l]                       row i of A P, 16 registers
//   C2  P-[i][j] = sum_l b[l] A[j][l] (+ fv + var_x at j = i) for j <= i, stored at [i][j] AND [j][i]: bitwise symmetric
//   C3  the scalar updates: row j is read back from LDS by the 16 lanes, the own row is held in registers and updated as
//       p[k] - (P[j][i] P[j][k]) / s, a commutative product, so the symmetry survives; delta through a 16-lane shuffle;
//       sum log(2 pi s) through LogProd (one log per lane and launch)
//
// The f64 MFMA units were not used for A P A^T: see DESIGN.md 3.2h.  The Jacobian tile shares the space of the kernel
// tile (dead once A2 exists; U_d is not formed without the variance Jacobian).
//
// No atomics, no spin wait (A of the two-triangular form goes through an LDS tile and workgroup barriers, as in
// gp_linearize_kernel): every output entry has one writer, two calls are bitwise identical, and a chain's results do not
// depend on the other chains of the call.  Rows m >= M are zero in every operand image; chains >= N repeat chain N - 1 and
// store nothing.  A y entry at cond = 0 is chosen away by a select and may be NaN.
#pragma once
#include "../../include/cbfssm_hip.h"
#include "cbfssm_gp_bwd.hpp"

namespace cbfssm {

struct GpEkfArgs {
    PackPtrs pk;
    RevPackPtrs rk;
    const double* m0;      // (N, Do)
    const double* P0;      // (N, Do, Do), lower triangle read, or null: zero
    const double* a;       // (T, N, D - Do) (unused when D == Do)
    const double* y;       // (T, N, Dy): entries at cond = 0 are never used (they may be NaN)
    const double* cond;    // (T, N) 0 / 1, or null: condition everywhere
    const double* var_x;   // (Do) or null
    const double* var_y;   // (Dy)
    const double* alpha;   // [16][16 NBLK]  (K^-1 mu)[m][d] at [d][m], zero padded (gp_lin_alpha_kernel)
    double* means;         // (T, N, Do)
    double* covs;          // (T, N, Do, Do)
    double* loglik;        // (N)
    double* pmeans;        // (T, N, Do)      m- of every step, before conditioning   (these three: all or none; GPModel.eks)
    double* pcovs;         // (T, N, Do, Do)  P- of every step, or null
    double* cross;         // (T, N, Do, Do)  A_t P_{t-1}: row i is b[] of C1, or null
    int N, T, M, D, Do, Dy, tri;
    double* jac;           // (T, N, Do, Do)  J[d][i] of every step, or null (with the three above: the forward under grad)
};

// LDS: xq | KJ | T1 | red0 | 1 / l | P | fm | fv.  KJ is the kernel tile [16 NBLK][17] and, once A2 exists, the Jacobian tile
// [16 chains][16 d][17].  T1 is A = L^-1 k of the two-triangular form while A2 is formed and the per-wave partial tiles
// afterwards: per wave the mean tile [16 JB][17] (row = input index, row D = column sum) and 16 partial sums of A2^2 s2_d.
// 16 528 doubles at 20 row blocks / DK 6; a Jacobian tile of its own would make that 20 880.
template <int NBLK, int DK>
struct GpEkfGeom {
    typedef GpBwdCfg<NBLK> C;
    static constexpr int JB = (4 * DK + 1 + 15) / 16;
    static constexpr int PD = 17;
    static constexpr int MP = 16 * NBLK;
    static constexpr int PT = 16 * JB * PD;             // one partial tile
    static constexpr int PW = PT + 16;                  // per wave
    static constexpr int CT = 16 * 16 * PD;             // covariance tile, Jacobian tile
    static constexpr int KJ = (MP * PD > CT) ? MP * PD : CT;
    static constexpr int T1 = (MP * PD > C::W * PW) ? MP * PD : C::W * PW;
    static constexpr int LDS_DOUBLES = 4 * DK * PD + KJ + T1 + C::W * 16 + 4 * DK + CT + 2 * 16 * PD;
    static_assert(LDS_DOUBLES <= 163840 / 8, "LDS budget");
};

// per (chain, row) lane of the covariance part: what it carries from step to step
struct EkfLane {
    double m, lin;
    LogProd lp;
};

// EMIT: the form behind GPModel.eks, which also stores cross, pmeans and pcovs (a compile-time flag: the stores cost the plain
// form up to 4 VGPRs and 31 spilled SGPRs as a run-time branch, and GPModel.ekf 0.2 % -- profiles/gp_eks/README.md)
// SAVEJ: the form behind gp_ekf under grad, which stores the Jacobian tile as well (cbfssm_gp_ekf_bwd.hpp)
template <int NBLK, int RB, int DK, bool EMIT, bool SAVEJ = false>
__global__ __launch_bounds__(64 * ((NBLK + RB - 1) / RB)) void gp_ekf_kernel(GpEkfArgs a)
{
    constexpr bool BREG = (RB == 1);                    // K^-1 rows of the wave in VGPRs (2 KS = 8 NBLK <= 56 registers)
    typedef GpEkfGeom<NBLK, DK> G;
    typedef GpWave<NBLK, RB, DK, BREG> WV;
    constexpr int W = WV::W, NT = WV::NT, MP = WV::MP;
    constexpr int JB = G::JB, PD = G::PD, PT = G::PT, PW = G::PW, CT = G::CT;
    constexpr int TPT = (256 + NT - 1) / NT;            // (chain, row) lanes per thread: 4, 2 or 1

    extern __shared__ double lds[];
    double* xq = lds;                                   // [4 DK][17] scaled inputs x~[j][n]
    double* Kt = xq + 4 * DK * PD;                      // [MP][17]  kernel tile, then:
    double* Jt = Kt;                                    // [16][16][17]  J[n][d][i] = d fmean[n][d] / d x[n][i], i < Do
    double* A2t = Kt + G::KJ;                           // [MP][17]  A of the two-triangular form, then:
    double* part = A2t;                                 // [W][PW]   per-wave partial tiles
    double* red0 = A2t + G::T1;                         // [W][16]   per-wave parts of sigma^2 - fvar0
    double* il = red0 + W * 16;                         // [4 DK]    1 / lengthscale (zero padded)
    double* Pt = il + 4 * DK;                           // [16][16][17]  P[n][i][k]; rows and columns >= Do stay zero
    double* fmt = Pt + CT;                              // [16][17]  fmean[d][n] of this step
    double* fvt = fmt + 16 * PD;                        // [16][17]  fvar[d][n]

    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, g = l >> 4, nl = l & 15;
    const int M = a.M, D = a.D, Do = a.Do, Dy = a.Dy, N = a.N, T = a.T;
    const int naux = D - Do;
    const int c0 = blockIdx.x * 16;
    const double sig2 = a.pk.scal[CBFSSM_SCAL_SIGMA2];

    WV wv;
    wv.setup(a.pk, tid);
    wv.setup_forms(a.pk);
    wv.hold_kinv(a.rk);                                 // BREG: the wave's K^-1 rows and (Z / l)^T operands in VGPRs
    // of the (Z~)^T E tile the state rows (first input row block) and the ones row D are used
    const bool jb_used1 = D >= 16;

    // ---- the (chain, row) lanes of the covariance part: lane id = 16 n + i, the 16 rows of a chain side by side in a wave
    EkfLane ln[TPT];
    int lc[TPT];                                        // chain of the call (clamped), for loads and stores
    double lvx[TPT], lil[TPT];
    for (int i = tid; i < 4 * DK; i += NT) il[i] = a.pk.invl[i];
    for (int i = tid; i < 4 * DK * PD; i += NT) xq[i] = 0.0;
    for (int i = tid; i < CT; i += NT) Pt[i] = 0.0;
    __syncthreads();
#pragma unroll
    for (int k2 = 0; k2 < TPT; ++k2) {
        const int id = tid + k2 * NT, n = (id >> 4) & 15, i = id & 15;
        const bool act = (id < 256) && (i < Do);
        const int ic = act ? i : 0;
        lc[k2] = min(c0 + n, N - 1);
        lvx[k2] = a.var_x ? a.var_x[ic] : 0.0;
        lil[k2] = a.pk.invl[ic];
        ln[k2].m = act ? a.m0[int64_t(lc[k2]) * Do + ic] : 0.0;
        ln[k2].lin = 0.0;
        ln[k2].lp.init();
        if (act) {
            double* Pn = Pt + n * 16 * PD;
            xq[i * PD + n] = ln[k2].m * lil[k2];
            if (a.P0) {
                const double* src = a.P0 + (int64_t(lc[k2]) * Do + i) * Do;
                for (int j = 0; j <= i; ++j) {
                    const double v = src[j];
                    Pn[i * PD + j] = v;
                    Pn[j * PD + i] = v;
                }
            }
        }
    }
    for (int i = tid; i < 16 * naux; i += NT) {
        const int ja = i >> 4, n = i & 15;
        xq[(Do + ja) * PD + n] = a.a[int64_t(min(c0 + n, N - 1)) * naux + ja] * a.pk.invl[Do + ja];
    }

    const int rows = Do + 1, items = 16 * rows;         // of the reduced tile: the state rows and the column sum, 16 chains

    for (int t = 0; t < T; ++t) {
        const bool has_next = (t + 1 < T);
        __syncthreads();                                // xq and P complete; the previous step's readers of J / fm / fv are done

        // this step's observation and mask, issued ahead of the GP work
        double yv[TPT], cnd[TPT];
#pragma unroll
        for (int k2 = 0; k2 < TPT; ++k2) {
            const int i = (tid + k2 * NT) & 15;
            const int64_t tc = int64_t(t) * N + lc[k2];
            yv[k2] = a.y[tc * Dy + (i < Dy ? i : 0)];
            cnd[k2] = a.cond ? a.cond[tc] : 1.0;
        }

        // ---- kernel tile (rows of this wave): the shared phase B
        d4 kreg[RB];
        wv.kernel_tile(xq, Kt, M, kreg);
        __syncthreads();

        // ---- A2 of this wave's rows and this wave's part of sigma^2 - fvar0: the shared A2 step
        d4 a2[RB];
        const double v0 = gp_sum_groups(wv.a2_forms(a.tri, Kt, A2t, kreg, a2));
        if (g == 0) red0[w * 16 + nl] = v0;
        __syncthreads();                                // every wave is done reading the kernel tile and A: both are free

        // ---- per output dimension; alpha[:, d] and s2[:, d] of this wave's rows are fetched one dimension ahead
        d4 aln[RB], s2n[RB];
        auto fetch = [&](int d) {
#pragma unroll
            for (int i = 0; i < RB; ++i) {
                const double* sBp = a.rk.s2B + wv.rbs[i] * 256 + (d >> 2) * 64 + 16 * (d & 3) + g;   // s2[16 rb + g + 4 r][d]
                const double* alp = a.alpha + d * MP + 16 * wv.rbs[i] + g;
#pragma unroll
                for (int r = 0; r < 4; ++r) { aln[i][r] = alp[4 * r]; s2n[i][r] = sBp[4 * r]; }
            }
        };
        fetch(0);
#pragma unroll 1
        for (int d = 0; d < Do; ++d) {
            // 1: Em_d and this wave's part of sum_m A2^2 s2_d (alpha and s2 are then free for the next dimension)
            d4 em[RB];
            double vs = 0.0;
#pragma unroll
            for (int i = 0; i < RB; ++i) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double u = wv.ok[i] ? a2[i][r] * s2n[i][r] : 0.0;
                    em[i][r] = aln[i][r] * kreg[i][r];
                    vs = fma(a2[i][r], u, vs);
                }
            }
            if (d + 1 < Do) fetch(d + 1);
            vs = gp_sum_groups(vs);
            __syncthreads();                            // the previous dimension's partial tiles are read

            // 2: the partial ZT products of Em_d over this wave's rows
            double* pw = part + w * PW;
            if (g == 0) pw[PT + nl] = vs;
            {
                d4 xm[JB];
#pragma unroll
                for (int jb = 0; jb < JB; ++jb) xm[jb] = d4{0, 0, 0, 0};
#pragma unroll
                for (int i = 0; i < RB; ++i) {
                    if (wv.ok[i]) {
                        const double* ZTp = a.rk.ZT + wv.rbs[i] * JB * 256 + l;
#pragma unroll
                        for (int jb = 0; jb < JB; ++jb) {
                            if (jb == 0 || jb_used1) {
#pragma unroll
                                for (int r = 0; r < 4; ++r)
                                    xm[jb] = CBF_MFMA(BREG ? wv.ztr[jb * 4 + r] : ZTp[(jb * 4 + r) * 64], em[i][r], xm[jb]);   // rows j, k = m
                            }
                        }
                    }
                }
#pragma unroll
                for (int jb = 0; jb < JB; ++jb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) pw[(16 * jb + 4 * r + g) * PD + nl] = xm[jb][r];
            }
            __syncthreads();                            // the partial tiles are whole

            // 3: the waves' partial tiles in a fixed order, the epilogue of linearize, into the Jacobian tile
            for (int it = tid; it < items; it += NT) {
                const int n = it / rows, jj = it - n * rows;
                const int j = (jj < Do) ? jj : D;
                const double* tp = part + n;
                double xb = 0.0;
                for (int ww = 0; ww < W; ++ww) xb += tp[ww * PW + j * PD];
                if (jj == Do) {
                    fmt[d * PD + n] = xb;               // the ones row: sum_m alpha[m][d] k[m][n]
                    continue;
                }
                double es = 0.0;
                for (int ww = 0; ww < W; ++ww) es += tp[ww * PW + D * PD];
                Jt[(n * 16 + d) * PD + j] = (xb - xq[j * PD + n] * es) * il[j];
            }
            if (tid < 16) {
                double s0 = 0.0, s1 = 0.0;
                for (int ww = 0; ww < W; ++ww) {
                    s0 += red0[ww * 16 + tid];
                    s1 += part[ww * PW + PT + tid];
                }
                fvt[d * PD + tid] = (sig2 - s0) + s1;
            }
        }
        __syncthreads();                                // J, fm, fv are whole; xq is free

        // ---- the covariance part: whole waves (lane ids < 256)
#pragma unroll
        for (int k2 = 0; k2 < TPT; ++k2) {
            const int id = tid + k2 * NT;
            if (id < 256) {                             // (wave uniform: 256 is a multiple of 64)
                const int n = id >> 4, i = id & 15;
                const bool act = i < Do;
                double* Pn = Pt + n * 16 * PD;
                const double* Jn = Jt + n * 16 * PD;
                const bool dc = (cnd[k2] != 0.0);
                double mi = ln[k2].m + (act ? fmt[i * PD + n] : 0.0);
                const double qi = act ? (fvt[i * PD + n] + lvx[k2]) : 0.0;

                // C1: row i of A P
                double b[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) b[q] = 0.0;
#pragma unroll 1
                for (int k = 0; k < Do; ++k) {
                    double aik = act ? Jn[i * PD + k] : 0.0;
                    if (k == i) aik += 1.0;
                    const double* pk = Pn + k * PD;
#pragma unroll
                    for (int q = 0; q < 16; ++q) b[q] = fma(aik, pk[q], b[q]);
                }
                __builtin_amdgcn_wave_barrier();        // the chain's 16 lanes have read P before one of them writes it
                const bool st = act && (c0 + n < N);
                const int64_t o = (int64_t(t) * N + lc[k2]) * Do + i;
                if (EMIT && st) {                       // A_t P_{t-1} for the smoother: its transpose is Cov(x_{t-1}, x_t | y_{0..t-1})
                    double* cr = a.cross + o * Do;
#pragma unroll
                    for (int q = 0; q < 16; ++q)
                        if (q < Do) cr[q] = b[q];
                }
                if constexpr (SAVEJ) {
                    if (st) {
                        double* jc = a.jac + o * Do;
#pragma unroll
                        for (int q = 0; q < 16; ++q)
                            if (q < Do) jc[q] = Jn[i * PD + q];
                    }
                }

                // C2: the lower triangle of A P A^T + diag, mirrored
                const int jend = act ? i : -1;
#pragma unroll 1
                for (int j = 0; j <= jend; ++j) {
                    const double* aj = Jn + j * PD;
                    double p = 0.0;
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        double ajq = (q < Do) ? aj[q] : 0.0;
                        if (q == j) ajq += 1.0;
                        p = fma(b[q], ajq, p);
                    }
                    if (j == i) p += qi;
                    Pn[i * PD + j] = p;
                    Pn[j * PD + i] = p;
                }
                __builtin_amdgcn_wave_barrier();

                // C3: the scalar updates; the own row in registers, row j from LDS
                double pr[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) pr[q] = Pn[i * PD + q];
                if (EMIT && st) {                       // the predicted moments, before conditioning
                    a.pmeans[o] = mi;
                    double* pc = a.pcovs + o * Do;
#pragma unroll
                    for (int q = 0; q < 16; ++q)
                        if (q < Do) pc[q] = pr[q];
                }
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
#pragma unroll
                for (int q = 0; q < 16; ++q) Pn[i * PD + q] = pr[q];
                ln[k2].m = mi;

                // the stores and the next scaled GP input
                if (act) {
                    if (st) {
                        a.means[o] = mi;
                        double* cv = a.covs + o * Do;
#pragma unroll
                        for (int q = 0; q < 16; ++q)
                            if (q < Do) cv[q] = pr[q];
                    }
                    if (has_next) xq[i * PD + n] = mi * lil[k2];
                }
            }
        }
        if (has_next) {
            for (int i = tid; i < 16 * naux; i += NT) {
                const int ja = i >> 4, n = i & 15;
                xq[(Do + ja) * PD + n] = a.a[(int64_t(t + 1) * N + min(c0 + n, N - 1)) * naux + ja] * il[Do + ja];
            }
        }
    }

    // ---- loglik[n] = -1/2 sum over the conditioned (step, j) of log(2 pi s) + delta^2 / s: every lane of a chain holds it
#pragma unroll
    for (int k2 = 0; k2 < TPT; ++k2) {
        const int id = tid + k2 * NT;
        if (id < 256 && (id & 15) == 0 && c0 + (id >> 4) < N)
            a.loglik[lc[k2]] = 0.0 - 0.5 * (ln[k2].lp.log() + ln[k2].lin);
    }
}

template <int NBLK, int DK>
int launch_gp_ekf_k(const GpEkfArgs& a, hipStream_t st)
{
    typedef GpBwdCfg<NBLK> C;
    const size_t lds = size_t(GpEkfGeom<NBLK, DK>::LDS_DOUBLES) * sizeof(double);
    auto k = a.jac ? gp_ekf_kernel<NBLK, C::RB, DK, true, true>
                   : (a.pcovs ? gp_ekf_kernel<NBLK, C::RB, DK, true> : gp_ekf_kernel<NBLK, C::RB, DK, false>);
    int rc = set_lds(k, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k, dim3(unsigned((a.N + 15) / 16)), dim3(64 * C::W), lds, st, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -int(e) - 1000;
}

template <int NBLK>
int launch_gp_ekf_n(int DK, const GpEkfArgs& a, hipStream_t st)
{
    switch (DK) {
        case 2: return launch_gp_ekf_k<NBLK, 2>(a, st);
        case 4: return launch_gp_ekf_k<NBLK, 4>(a, st);
        case 6: return launch_gp_ekf_k<NBLK, 6>(a, st);
    }
    return -2;
}

}  // namespace cbfssm

#define CBF_GPEKF_DECLARE(NB)                                                                    \
    namespace cbfssm {                                                                           \
    int launch_gp_ekf_nb##NB(int DK, const GpEkfArgs& a, hipStream_t st);                        \
    }

#define CBF_GPEKF_INSTANTIATE(NB)                                                                \
    namespace cbfssm {                                                                           \
    int launch_gp_ekf_nb##NB(int DK, const GpEkfArgs& a, hipStream_t st)                         \
    {                                                                                            \
        return launch_gp_ekf_n<NB>(DK, a, st);                                                   \
    }                                                                                            \
    }
