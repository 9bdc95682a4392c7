// Local linear model of one sparse GP: the Jacobians of GPModel.predict (gp_tf.py:132-161) with respect to its inputs,
// what tf.gradients(fmean[:, d], Xnew) and tf.gradients(fvar[:, d], Xnew) give per output dimension d, in one launch.
//
//   k = K(Z, x_n),  A2 = K^-1 k,  alpha = K^-1 mu (M x Do, loop invariant),  s2_d = zeta_var[:, d],  z~ = Z / l,  x~ = x / l
//
//   d k[m] / d x[i]  = k[m] (z~[m][i] - x~[i]) / l_i
//   dmean[n][d][i]   = ( sum_m z~[m][i] Em_d[m][n] - x~[n][i] sum_m Em_d[m][n] ) / l_i,   Em_d = alpha[:, d] o k
//   dvar[n][d][i]    = ( sum_m z~[m][i] Ev_d[m][n] - x~[n][i] sum_m Ev_d[m][n] ) / l_i,   Ev_d = 2 (K^-1 (A2 o s2_d) - A2) o k
//
// This is gp_predict_bwd_kernel (cbfssm_gp_bwd.hpp) with the upstream adjoint Fm = e_d or Fv = e_d: for the mean
// Kbar = K^-1 (mu_d 1^T) = alpha_d 1^T needs no product per block, for the variance Kbar = 2 (K^-1 (A2 o s2_d) - A2) needs
// one K^-1 product per output dimension, and both end in the (Z~)^T E product against the pack's ZT image, whose ones row
// (row D) gives the column sum of E -- for the mean that column sum is fmean[n][d] itself.
//
// The skeleton is that of gp_fullq_fwd_kernel (cbfssm_gp_fullq.hpp): the wave layout GpBwdCfg<NBLK>, the persistent grid
// stride over 16-point column blocks, and from the shared body (cbfssm_gp_tile.hpp, GpWave) the row-block setup, the kernel
// tile (phase B), A2 and fvar0 in the form layout->gp_form asks for, and the K^-1 products.  Per column block and output
// dimension, between two workgroup barriers:
//
//   1  U_d = A2 o s2_d, this wave's rows -> the LDS tile the kernel tile left (every wave keeps its k rows in VGPRs)
//   2  this wave's rows of K^-1 U_d (the dense K^-1 image in both GP forms, as the adjoint kernels do)            MFMA
//      Em_d = alpha_d o k,  Ev_d = 2 (K^-1 U_d - A2) o k: one multiply per accumulator entry, outside the MFMA loops
//      partial (Z~)^T E over this wave's rows, all JB input row blocks -> this wave's partial tiles in LDS        MFMA
//   3  the partial tiles summed over the waves in a fixed order, x~ colsum subtracted, scaled by 1 / l_i, stored with the
//      input index fastest (runs of D doubles per point and dimension)
//
// With one row block per wave (up to seven row blocks) the wave's rows of the K^-1 image (used 1 + Do times per column block)
// and of the ZT image stay in VGPRs for the whole launch, as the pass kernels keep K^-1; above that they stream from L2.
//
// The contraction over m spans the waves.  Partial products over the wave's own rows followed by a fixed-order sum through
// LDS were chosen over dealing the ZT products of an E tile to the waves: the ZT product of one output dimension is JB
// output blocks, so a deal would keep one or two waves busy on 4 NBLK dependent MFMAs each while the others wait, and it
// needs the same two barriers per dimension (E tile written / E tile free again).  No atomics: every output entry has one
// writer, and two calls are bitwise identical.  Rows m >= M are zero in every operand image; points >= npts are computed on
// zero inputs and never stored; input columns i >= D are never stored.
#pragma once
#include "../../include/cbfssm_hip.h"
#include "cbfssm_gp_bwd.hpp"

namespace cbfssm {

struct GpLinArgs {
    PackPtrs pk;
    RevPackPtrs rk;
    const double* X;       // (npts, D)
    const double* alpha;   // [16][16 NBLK]  (K^-1 mu)[m][d] at [d][m], zero padded (gp_lin_alpha_kernel)
    double* fmean;         // (npts, Do) or null
    double* fvar;          // (npts, Do) or null
    double* dmean;         // (npts, Do, D)
    double* dvar;          // (npts, Do, D) or null: mean only, no K^-1 product per output dimension
    int64_t npts;
    int64_t nblocks;       // ceil(npts / 16)
    int M, D, Do, tri;
};

// LDS: xq | T0 | T1 | red0 | 1 / l.  T0 [16 NBLK][17] is the kernel tile and, once A2 exists, the U_d tile.  T1 is A = L^-1 k of
// the two-triangular form while A2 is formed and the per-wave partial tiles afterwards: per wave the mean tile and the
// variance tile [16 JB][17] each (row = input index, row D = column sum) and 16 partial sums of A2^2 s2_d.  Five separate
// [16 NBLK][17] tiles would be 27 200 doubles at 20 row blocks; this layout is 17 072 there.
template <int NBLK, int DK>
struct GpLinGeom {
    typedef GpBwdCfg<NBLK> C;
    static constexpr int JB = (4 * DK + 1 + 15) / 16;
    static constexpr int PD = 17;
    static constexpr int MP = 16 * NBLK;
    static constexpr int PT = 16 * JB * PD;             // one partial tile
    static constexpr int PW = 2 * PT + 16;              // per wave
    static constexpr int T1 = (MP * PD > C::W * PW) ? MP * PD : C::W * PW;
    static constexpr int LDS_DOUBLES = 4 * DK * PD + MP * PD + T1 + C::W * 16 + 4 * DK;
    static_assert(LDS_DOUBLES <= 163840 / 8, "LDS budget");
};

template <int NBLK, int RB, int DK>
__global__ __launch_bounds__(64 * ((NBLK + RB - 1) / RB)) void gp_linearize_kernel(GpLinArgs a)
{
    constexpr bool BREG = (RB == 1);                    // K^-1 rows of the wave in VGPRs (2 KS = 8 NBLK <= 56 registers)
    typedef GpLinGeom<NBLK, DK> G;
    typedef GpWave<NBLK, RB, DK, BREG> WV;
    constexpr int W = WV::W, NT = WV::NT, MP = WV::MP;
    constexpr int JB = G::JB, PD = G::PD, PT = G::PT, PW = G::PW;

    extern __shared__ double lds[];
    double* xq = lds;                                   // [4 DK][17] scaled inputs x~[j][n]
    double* Kt = xq + 4 * DK * PD;                      // [MP][17]  kernel tile, then U_d = A2 o s2_d
    double* A2t = Kt + MP * PD;                         // [MP][17]  A of the two-triangular form, then:
    double* part = A2t;                                 // [W][PW]   per-wave partial tiles
    double* red0 = A2t + G::T1;                         // [W][16]   per-wave parts of sigma^2 - fvar0
    double* il = red0 + W * 16;                         // [4 DK]    1 / lengthscale (zero padded), for step 3

    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, g = l >> 4, nl = l & 15;
    const int M = a.M, D = a.D, Do = a.Do;
    const double sig2 = a.pk.scal[CBFSSM_SCAL_SIGMA2];
    const bool want_var = a.dvar != nullptr;

    WV wv;
    wv.setup(a.pk, tid);
    wv.setup_forms(a.pk);
    wv.hold_kinv(a.rk);                                 // BREG: the wave's K^-1 rows and (Z / l)^T operands in VGPRs
    for (int i = tid; i < 4 * DK; i += NT) il[i] = a.pk.invl[i];       // (made visible by the barriers of the first block)
    // step 3: (D + 1) rows (the inputs and the column sum) of 16 points, per tile
    const int rows = D + 1, per = 16 * rows, items = (want_var ? 2 : 1) * per;

    for (int64_t cb = blockIdx.x; cb < a.nblocks; cb += gridDim.x) {
        const int64_t p0 = cb * 16;
        __syncthreads();                                // the previous block's readers of xq / part / red0 are done
        for (int i = tid; i < 4 * DK * 16; i += NT) {
            const int j = i >> 4, n = i & 15;
            const int64_t p = p0 + n;
            double v = 0.0;
            if (j < D && p < a.npts) v = a.X[p * D + j] * il[j];
            xq[j * PD + n] = v;
        }
        __syncthreads();

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
            // 1: U_d, this wave's part of sum_m A2^2 s2_d, and Em_d (alpha and s2 are then free for the next dimension)
            d4 em[RB];
            double vs = 0.0;
#pragma unroll
            for (int i = 0; i < RB; ++i) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double u = wv.ok[i] ? a2[i][r] * s2n[i][r] : 0.0;
                    em[i][r] = aln[i][r] * kreg[i][r];
                    vs = fma(a2[i][r], u, vs);
                    if (want_var && wv.ok[i]) Kt[(16 * wv.rbs[i] + g + 4 * r) * PD + nl] = u;
                }
            }
            if (d + 1 < Do) fetch(d + 1);
            vs = gp_sum_groups(vs);
            __syncthreads();                            // U_d is whole; the previous dimension's partial tiles are read

            // 2: the partial ZT products of Em_d, then Ev_d on this wave's rows and its partial ZT products (the mean's
            // operands and results are dead before the K^-1 product starts)
            double* pw = part + w * PW;
            if (g == 0) pw[2 * PT + nl] = vs;
            {
                d4 xm[JB];
#pragma unroll
                for (int jb = 0; jb < JB; ++jb) xm[jb] = d4{0, 0, 0, 0};
#pragma unroll
                for (int i = 0; i < RB; ++i) {
                    if (wv.ok[i]) {
                        const double* ZTp = a.rk.ZT + wv.rbs[i] * JB * 256 + l;
#pragma unroll
                        for (int jb = 0; jb < JB; ++jb)
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                xm[jb] = CBF_MFMA(BREG ? wv.ztr[jb * 4 + r] : ZTp[(jb * 4 + r) * 64], em[i][r], xm[jb]);   // rows j, k = m
                    }
                }
#pragma unroll
                for (int jb = 0; jb < JB; ++jb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) pw[(16 * jb + 4 * r + g) * PD + nl] = xm[jb][r];
            }
            if (want_var) {
                d4 ev[RB];
                wv.kinv_times(Kt, ev);
#pragma unroll
                for (int i = 0; i < RB; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) ev[i][r] = 2.0 * (ev[i][r] - a2[i][r]) * kreg[i][r];
                d4 xv[JB];
#pragma unroll
                for (int jb = 0; jb < JB; ++jb) xv[jb] = d4{0, 0, 0, 0};
#pragma unroll
                for (int i = 0; i < RB; ++i) {
                    if (wv.ok[i]) {
                        const double* ZTp = a.rk.ZT + wv.rbs[i] * JB * 256 + l;
#pragma unroll
                        for (int jb = 0; jb < JB; ++jb)
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                xv[jb] = CBF_MFMA(BREG ? wv.ztr[jb * 4 + r] : ZTp[(jb * 4 + r) * 64], ev[i][r], xv[jb]);
                    }
                }
#pragma unroll
                for (int jb = 0; jb < JB; ++jb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) pw[PT + (16 * jb + 4 * r + g) * PD + nl] = xv[jb][r];
            }
            __syncthreads();                            // the partial tiles are whole; every wave is done reading U_d

            // 3: the waves' partial tiles in a fixed order, the epilogue, the stores (input index fastest)
            for (int it = tid; it < items; it += NT) {
                const int kind = it >= per, rem = it - kind * per;
                const int n = rem / rows, j = rem - n * rows;
                const int64_t p = p0 + n;
                const double* t = part + kind * PT + n;
                double xb = 0.0;
                for (int ww = 0; ww < W; ++ww) xb += t[ww * PW + j * PD];
                if (p >= a.npts) continue;
                if (j == D) {
                    if (kind == 0 && a.fmean) a.fmean[p * Do + d] = xb;      // the ones row: sum_m alpha[m][d] k[m][n]
                    continue;
                }
                double es = 0.0;
                for (int ww = 0; ww < W; ++ww) es += t[ww * PW + D * PD];
                const double v = (xb - xq[j * PD + n] * es) * il[j];
                (kind ? a.dvar : a.dmean)[(p * Do + d) * D + j] = v;
            }
            if (a.fvar && tid < 16 && p0 + tid < a.npts) {
                double s0 = 0.0, s1 = 0.0;
                for (int ww = 0; ww < W; ++ww) {
                    s0 += red0[ww * 16 + tid];
                    s1 += part[ww * PW + 2 * PT + tid];
                }
                a.fvar[(p0 + tid) * Do + d] = (sig2 - s0) + s1;
            }
        }
    }
}

template <int NBLK, int DK>
int launch_gp_lin_k(const GpLinArgs& a, unsigned nwg, hipStream_t st)
{
    typedef GpBwdCfg<NBLK> C;
    const size_t lds = size_t(GpLinGeom<NBLK, DK>::LDS_DOUBLES) * sizeof(double);
    auto k = gp_linearize_kernel<NBLK, C::RB, DK>;
    int rc = set_lds(k, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k, dim3(nwg), dim3(64 * C::W), lds, st, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -int(e) - 1000;
}

template <int NBLK>
int launch_gp_lin_n(int DK, const GpLinArgs& a, unsigned nwg, hipStream_t st)
{
    switch (DK) {
        case 2: return launch_gp_lin_k<NBLK, 2>(a, nwg, st);
        case 4: return launch_gp_lin_k<NBLK, 4>(a, nwg, st);
        case 6: return launch_gp_lin_k<NBLK, 6>(a, nwg, st);
    }
    return -2;
}

}  // namespace cbfssm

#define CBF_GPLIN_DECLARE(NB)                                                                    \
    namespace cbfssm {                                                                           \
    int launch_gp_lin_nb##NB(int DK, const GpLinArgs& a, unsigned nwg, hipStream_t st);          \
    }

#define CBF_GPLIN_INSTANTIATE(NB)                                                                \
    namespace cbfssm {                                                                           \
    int launch_gp_lin_nb##NB(int DK, const GpLinArgs& a, unsigned nwg, hipStream_t st)           \
    {                                                                                            \
        return launch_gp_lin_n<NB>(DK, a, nwg, st);                                              \
    }                                                                                            \
    }
