// Batch adjoint of GPModel.predict (gp_tf.py:132-161): what tf.gradients gives a caller who builds a model of their own
// around one sparse GP (cbfssm/model/voliro.py:106-123 calls gp_f.predict once over all B T points).
//
// The algebra of one 16-point column block is what rev_kernel (cbfssm_adjoint.hpp) does inside one time step, with the
// kernel tile and A2 = K^-1 K recomputed and without the recurrence: the upstream adjoints Fm = d loss / d fmean and
// Fv = d loss / d fvar come from the caller, and the input adjoint leaves the kernel instead of being carried.
//
//   B   K tile of this wave's rows (MFMA + exp) -> LDS
//   C   A2 = K^-1 K                                                                                        MFMA
//   E   A2bar = mu Fm + 2 A2 o (s2 Fv) - K o colsum(Fv)
//       mubar += A2 Fm^T,  s2bar += (A2 o A2) Fv^T,  Kinvbar += A2bar K^T   (k-dim = the 16 points)        MFMA
//   F   Kbar = K^-1 A2bar - A2 o colsum(Fv);  Ebar = Kbar o K
//       xbar~ = Z~^T Ebar - x~ o colsum(Ebar) for ALL input rows,  Zbar~ += Ebar x~^T                      MFMA
//   G   gX = xbar~ / lengthscale (every entry written once), lengthscale / variance sums
//
// Workgroups are persistent over the column blocks (grid stride) and keep the parameter adjoints in VGPRs across their
// blocks; they leave once, as one partial slab per workgroup in the Slab<> layout of the time-loop adjoints, so
// cbfssm_reduce_partials_f64 and the K_mm -> Cholesky -> K^-1 tail take them as they are.  No atomics: the points do not
// interact, every output has one writer, and two calls are bitwise identical.
// Tile heights above seven row blocks (M > 112) cannot hold the Kinvbar accumulator (NBLK x NBLK x 256 doubles per
// workgroup) in registers: they write the two MFMA operand images of Kinvbar += A2bar K^T per column block -- the stash
// images of the time-loop adjoints, slot = column block -- and cbfssm_stash_contract_f64 contracts them.
#pragma once
#include "cbfssm_adjoint.hpp"
#include "cbfssm_inst.hpp"
#include "cbfssm_gp_tile.hpp"

namespace cbfssm {

struct GpBwdArgs {
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
    int M, D, Do;
};

template <int NBLK>
struct GpBwdCfg {
    static constexpr bool STASH = (NBLK > 7);
    static constexpr int RB = STASH ? 2 : 1;
    static constexpr int W = (NBLK + RB - 1) / RB;
    // persistent workgroups: enough to fill the 256 compute units with the waves a tile height brings
    static constexpr int MAXWG = (NBLK <= 2) ? 1024 : ((NBLK <= 7) ? 512 : 256);
};

template <int NBLK, int DK>
struct GpBwdGeom {
    typedef GpBwdCfg<NBLK> C;
    static constexpr int JB = (4 * DK + 1 + 15) / 16;
    static constexpr int PD = 17;
    static constexpr int LDS_DOUBLES = 4 * DK * PD + 2 * (16 * NBLK) * PD + 2 * 16 * PD + C::W * JB * 256 + 64;
    static constexpr int SLAB = Slab<NBLK, JB, C::STASH>::total;
    static_assert(LDS_DOUBLES <= 163840 / 8, "LDS budget");
};

template <int NBLK, int RB, int DK, bool STASH>
__global__ __launch_bounds__(64 * ((NBLK + RB - 1) / RB)) void gp_predict_bwd_kernel(GpBwdArgs a)
{
    typedef GpWave<NBLK, RB, DK> WV;
    constexpr int W = WV::W, NT = WV::NT, MP = WV::MP;
    constexpr int JB = WV::JB;
    constexpr int NG = 4 * JB;                          // 4-row groups of the input-adjoint tile
    constexpr int GPW = (NG + W - 1) / W;               // groups per wave in phase G
    constexpr int PD = WV::PD;
    constexpr int PSL = WV::PSL;

    extern __shared__ double lds[];
    double* xq = lds;                                   // [4 DK][17] scaled inputs x~[j][n]
    double* Kt = xq + 4 * DK * PD;                      // [MP][17]  kernel tile, then Ebar transposes
    double* A2t = Kt + MP * PD;                         // [MP][17]  A2 transposes, then the A2bar tile
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
    acc.zero();
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

        // ---- E: A2bar, and the parameter adjoints that contract over the 16 points; stash slot = column block
        GpUpstream up;
        wv.load_upstream(Fm, Fv, up, gsig);
        wv.template phase_E<STASH>(a.rk, up, Kt, A2t, a2, kreg, cb, a.stash_a, a.stash_k, acc);
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
int launch_gp_bwd_k(const GpBwdArgs& a, unsigned nwg, hipStream_t st)
{
    typedef GpBwdCfg<NBLK> C;
    typedef GpBwdGeom<NBLK, DK> G;
    const size_t lds = size_t(G::LDS_DOUBLES) * sizeof(double);
    auto k = gp_predict_bwd_kernel<NBLK, C::RB, DK, C::STASH>;
    int rc = set_lds(k, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k, dim3(nwg), dim3(64 * C::W), lds, st, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -int(e) - 1000;
}

template <int NBLK>
int launch_gp_bwd_n(int DK, const GpBwdArgs& a, unsigned nwg, hipStream_t st)
{
    switch (DK) {
        case 2: return launch_gp_bwd_k<NBLK, 2>(a, nwg, st);
        case 4: return launch_gp_bwd_k<NBLK, 4>(a, nwg, st);
        case 6: return launch_gp_bwd_k<NBLK, 6>(a, nwg, st);
    }
    return -2;
}

}  // namespace cbfssm

#define CBF_GPBWD_DECLARE(NB)                                                                    \
    namespace cbfssm {                                                                           \
    int launch_gp_bwd_nb##NB(int DK, const GpBwdArgs& a, unsigned nwg, hipStream_t st);          \
    }

#define CBF_GPBWD_INSTANTIATE(NB)                                                                \
    namespace cbfssm {                                                                           \
    int launch_gp_bwd_nb##NB(int DK, const GpBwdArgs& a, unsigned nwg, hipStream_t st)           \
    {                                                                                            \
        return launch_gp_bwd_n<NB>(DK, a, nwg, st);                                              \
    }                                                                                            \
    }

#define CBF_FOR_EACH_GPBWD_NBLK(X) X(1) X(2) X(4) X(7) X(10) X(13) X(16) X(20)
