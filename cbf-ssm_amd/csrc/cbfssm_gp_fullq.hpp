// Batch adjoint of the full-covariance conditional (gp_tf.py:68-100 with q_sqrt of shape (Do, M, M), and the
// zeta_std.ndims == 3 branch of GPModel.predict, gp_tf.py:150-159): q(z_d) = N(f_d, S_d), S_d = L_d L_d^T, L_d = tril(q_sqrt[d]).
//
//   fvar[n][d] = sigma^2 - k_n^T a_n + a_n^T S_d a_n,   a_n = K^-1 k_n
//
// This is gp_predict_bwd_kernel (cbfssm_gp_bwd.hpp) on the same shared phases (cbfssm_gp_tile.hpp: setup, B, C, F, the
// slab; of E the transposes and the Kinvbar step), with one term of phase E replaced and one result added, which are its own:
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
    typedef GpWave<NBLK, RB, DK> WV;
    constexpr int W = WV::W, NT = WV::NT, MP = WV::MP;
    constexpr int JB = WV::JB;
    constexpr int NG = 4 * JB;                          // 4-row groups of the input-adjoint tile
    constexpr int GPW = (NG + W - 1) / W;               // groups per wave in phase G
    constexpr int PD = 17;
    constexpr int PSL = JB * 256;

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

    WV wv;
    wv.setup(a.pk, tid);

    // ---- accumulators of the parameter adjoints (all column blocks of this workgroup)
    GpAdjAcc<NBLK, RB, JB, STASH> acc;
    acc.zero();                                         // (gS2 stays zero: no diagonal sigma_z^2 in the full form)
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

        // ---- B: kernel tile (rows of this wave)
        d4 kreg[RB];
        wv.kernel_tile(xq, Kt, M, kreg);
        __syncthreads();

        // ---- C: A2 rows of this wave (K^-1 streams from L2 as the A-operand image of the pack)
        d4 a2[RB];
        wv.image_times_tile(wv.bop, Kt, a2);

        // ---- D': A2 of the whole block where every wave reads it, and as this column block's C-layout image (W_d)
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            if (wv.ok[i]) {
                double* own = A2t + 16 * wv.rbs[i] * PD;
                double* pi = a.a2img + (cb * NBLK + wv.rbs[i]) * 256 + l;
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
            for (int i = 0; i < RB; ++i) sop[i] = a.Sp + (int64_t(d) * NBLK + wv.rbs[i]) * WV::KS * 64 + l;
            d4 sa[RB];
            wv.image_times_tile(sop, A2t, sa);
            const double fvd = Fv[d * PD + nl];
#pragma unroll
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) sq[i][r] = fma(sa[i][r], fvd, sq[i][r]);
        }
        __syncthreads();                                // every wave is done reading the A2 tile: phase E overwrites it

        // ---- E: A2bar with the S_d term, and the parameter adjoints that contract over the 16 points (no s2bar); the
        // transposes and the Kinvbar step are the shared pieces, stash slot = column block
        GpUpstream up;
        wv.template load_upstream<false>(Fm, Fv, up, gsig);
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            if (wv.ok[i]) {
                const double* mBp = a.rk.muB + wv.rbs[i] * 256 + l;
                double mv[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) mv[s] = mBp[s * 64];
                d4 T1 = {0, 0, 0, 0};
#pragma unroll
                for (int s = 0; s < 4; ++s) T1 = CBF_MFMA(mv[s], up.fmB[s], T1);
                d4 a2bar;
#pragma unroll
                for (int r = 0; r < 4; ++r) a2bar[r] = T1[r] + 2.0 * sq[i][r] - kreg[i][r] * up.fvsum;
                double a2T[4], abT[4];
                double* own = A2t + 16 * wv.rbs[i] * PD;
                wv.load_a(own, a2T);                    // (phase D' left A2 in these rows)
                __builtin_amdgcn_wave_barrier();
                wv.store_c(own, a2bar);                 // stays: A2bar tile of phase F
#pragma unroll
                for (int s = 0; s < 4; ++s) acc.gMu[i] = CBF_MFMA(a2T[s], up.fmT[s], acc.gMu[i]);   // mubar[m][d] += A2[m][n] Fm[d][n]
                __builtin_amdgcn_wave_barrier();
                wv.load_a(own, abT);
                wv.template kinv_adjoint<STASH>(i, abT, Kt, cb, a.stash_a, a.stash_k, acc.gB[i]);
            }
        }
        __syncthreads();

        // ---- F: Kbar, Ebar, input adjoint partials, Zbar~
        d4 ebar[RB];
        wv.kbar(A2t, a2, up.fvsum, ebar);
        wv.ebar_of(ebar, kreg, M, ebar);
        wv.phase_F_tail(a.rk.ZT, Kt, xq, part, ebar, D, acc.gZ);
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
    wv.template write_slab<STASH>(slab, acc);
    __syncthreads();
    wv.template write_sums<STASH>(slab, glx, gsig, glogsig, red);
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

template <int NBLK, int RB, int DK>
__global__ __launch_bounds__(64 * ((NBLK + RB - 1) / RB)) void gp_fullq_fwd_kernel(GpFqFwdArgs a)
{
    typedef GpWave<NBLK, RB, DK> WV;
    constexpr int W = WV::W, NT = WV::NT, MP = WV::MP;
    constexpr int PD = 17;

    extern __shared__ double lds[];
    double* xq = lds;                                   // [4 DK][17] scaled inputs x~[j][n]
    double* Kt = xq + 4 * DK * PD;                      // [MP][17]  kernel tile
    double* A2t = Kt + MP * PD;                         // [MP][17]  A (two-triangular form), then A2
    double* red = A2t + MP * PD;                        // [W][17][16] per-wave column partials: slot d < Do, slot 16 = fvar0

    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, g = l >> 4, nl = l & 15;
    const int M = a.M, D = a.D, Do = a.Do;
    const double sig2 = a.pk.scal[CBFSSM_SCAL_SIGMA2];

    WV wv;
    wv.setup(a.pk, tid);
    wv.setup_forms(a.pk);

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

        // ---- kernel tile (rows of this wave): the shared phase B
        d4 kreg[RB];
        wv.kernel_tile(xq, Kt, M, kreg);
        __syncthreads();

        // ---- A2 of this wave's rows and this wave's part of sigma^2 - fvar0 (the shared A2 step), A2 -> LDS
        d4 a2[RB];
        double v0 = wv.a2_forms(a.tri, Kt, A2t, kreg, a2);
        if (a.tri) __syncthreads();                     // every wave has read A before A2 takes its place
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            if (wv.ok[i]) {
#pragma unroll
                for (int r = 0; r < 4; ++r) A2t[(16 * wv.rbs[i] + g + 4 * r) * PD + nl] = a2[i][r];
            }
        }
        v0 = gp_sum_groups(v0);
        if (g == 0) red[(w * 17 + 16) * 16 + nl] = v0;
        __syncthreads();

        // ---- per output dimension: rows of S_d A2, then sum_m a2 (S_d A2) over this wave's rows
#pragma unroll 1
        for (int d = 0; d < Do; ++d) {
            const double* sop[RB];
#pragma unroll
            for (int i = 0; i < RB; ++i) sop[i] = a.Sp + (int64_t(d) * NBLK + wv.rbs[i]) * WV::KS * 64 + l;
            d4 sa[RB];
            wv.image_times_tile(sop, A2t, sa);
            double v = 0.0;
#pragma unroll
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) v = fma(a2[i][r], sa[i][r], v);
            v = gp_sum_groups(v);
            if (g == 0) red[(w * 17 + d) * 16 + nl] = v;
        }

        // ---- fmean^T = mu^T A2 on the last wave: the pack's mean image read as an A operand (row d, k = m)
        if (w == W - 1) {
            d4 fm[2] = {d4{0, 0, 0, 0}, d4{0, 0, 0, 0}};
#pragma unroll 1
            for (int s = 0; s < wv.KSr; ++s) fm[s & 1] = CBF_MFMA(a.pk.muA[s * 64 + l], A2t[(4 * s + g) * PD + nl], fm[s & 1]);
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

