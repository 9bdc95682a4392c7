// Host side of GPModel.linearize (cbfssm_gp_lin.hpp): argument checks, the pre-kernel that forms alpha = K^-1 mu once per
// call, and the launch.  The pre-kernel is a plain library kernel (one output entry per thread, fixed summation order); it
// is not tuned: M Do <= 5120 dot products of length M.
#include <hip/hip_runtime.h>
#include <cstring>
#include "../../include/cbfssm_hip.h"
#include "cbfssm_gp_lin.hpp"
#include "cbfssm_gp_host.hpp"

CBF_FOR_EACH_GPBWD_NBLK(CBF_GPLIN_DECLARE)

namespace cbfssm {

static int gp_lin_maxwg(int NBLK)
{
    switch (NBLK) {
#define X(NB) case NB: return GpBwdCfg<NB>::MAXWG;
        CBF_FOR_EACH_GPBWD_NBLK(X)
#undef X
    }
    return 0;
}

static int dispatch_gp_lin(int NBLK, int DK, const GpLinArgs& a, unsigned nwg, hipStream_t st)
{
    switch (NBLK) {
#define X(NB) case NB: return launch_gp_lin_nb##NB(DK, a, nwg, st);
        CBF_FOR_EACH_GPBWD_NBLK(X)
#undef X
    }
    return -3;
}

// alpha[d][m] = (K^-1 mu)[m][d] for d < 16, m < 16 NBLK, zero in the padding.  One workgroup per output dimension.
//   dense form:           alpha_d = Kinv mu_d
//   two-triangular form:  alpha_d = G (G^T mu_d),  G = L^-T (upper triangular: the pack's Linvt) -- the order of the
//                         reference's two triangular solves (gp_tf.py:137,145), which keeps its accuracy when K_mm is
//                         ill-conditioned and the entries of K^-1 are large
// mu is read from its operand image: mu[m][d] at muB[(m / 16) 256 + (d / 4) 64 + 16 (d % 4) + m % 16].
__global__ __launch_bounds__(256) void gp_lin_alpha_kernel(const double* Kinv, const double* G, const double* muB, int M, int Do,
                                                           int MP, int tri, double* alpha)
{
    __shared__ double mu[CBFSSM_MAX_M], t[CBFSSM_MAX_M];
    const int tid = threadIdx.x, d = blockIdx.x;
    double* out = alpha + d * MP;
    if (d >= Do) {
        for (int m = tid; m < MP; m += 256) out[m] = 0.0;
        return;
    }
    for (int m = tid; m < M; m += 256) mu[m] = muB[(m >> 4) * 256 + (d >> 2) * 64 + 16 * (d & 3) + (m & 15)];
    __syncthreads();
    if (tri) {
        for (int j = tid; j < M; j += 256) {
            double s = 0.0;
            for (int i = 0; i <= j; ++i) s = fma(G[i * M + j], mu[i], s);
            t[j] = s;
        }
        __syncthreads();
        for (int m = tid; m < MP; m += 256) {
            double s = 0.0;
            if (m < M)
                for (int j = m; j < M; ++j) s = fma(G[m * M + j], t[j], s);
            out[m] = s;
        }
    } else {
        for (int m = tid; m < MP; m += 256) {
            double s = 0.0;
            if (m < M)
                for (int j = 0; j < M; ++j) s = fma(Kinv[m * M + j], mu[j], s);
            out[m] = s;
        }
    }
}

}  // namespace cbfssm

using namespace cbfssm;

extern "C" {

int64_t cbfssm_gp_linearize_work_elems(const cbfssm_pack_layout* L)
{
    if (!gp_layout_ok(L)) return -1;
    return int64_t(16) * 16 * L->NBLK;
}

int cbfssm_gp_linearize_f64(const cbfssm_pack_layout* L, const double* pack, const double* X, int64_t npts, double* fmean,
                            double* fvar, double* dmean, double* dvar, double* work, void* stream)
{
    if (!L) return fail(-1, "null layout");
    if (!gp_layout_ok(L))
        return fail(-3, "gp_linearize limits: M <= %d, D <= 24, Do <= %d, and a layout of cbfssm_gp_pack_layout (M=%d D=%d Do=%d)",
                    CBFSSM_MAX_M, CBFSSM_MAX_DOUT, L->M, L->D, L->Do);
    if (npts < 0 || npts > (int64_t(1) << 34)) return fail(-1, "bad npts");
    if (!pack || !X || !dmean || !work) return fail(-1, "null pointer");
    if (npts == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int tri = (L->gp_form == CBFSSM_GP_FORM_TRI);
    hipLaunchKernelGGL(gp_lin_alpha_kernel, dim3(16), dim3(256), 0, st, pack + L->Kinv, pack + L->Linvt, pack + L->muB, L->M,
                       L->Do, 16 * L->NBLK, tri, work);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-int(e) - 1000, "gp_linearize: alpha launch failed");
    GpLinArgs a;
    memset(&a, 0, sizeof(a));
    gp_pack_ptrs(L, pack, a.pk, a.rk);
    a.X = X; a.alpha = work; a.fmean = fmean; a.fvar = fvar; a.dmean = dmean; a.dvar = dvar;
    a.npts = npts; a.nblocks = (npts + 15) / 16;
    a.M = L->M; a.D = L->D; a.Do = L->Do; a.tri = tri;
    const int64_t cap = gp_lin_maxwg(L->NBLK);                   // persistent over the column blocks beyond that
    const unsigned nwg = unsigned(a.nblocks < cap ? a.nblocks : cap);
    int rc = dispatch_gp_lin(L->NBLK, L->DK, a, nwg, st);
    if (rc) return fail(rc, "gp_linearize launch failed (NBLK=%d DK=%d rc=%d)", L->NBLK, L->DK, rc);
    return 0;
}

}  // extern "C"
