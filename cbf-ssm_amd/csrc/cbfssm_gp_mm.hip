// Host side of GPModel.moment_match (cbfssm_gp_mm.hpp): argument checks, the two pre-kernels that form alpha = K^-1 mu
// (gp_lin_alpha_kernel, cbfssm_gp_lin.hip) and the tiles of W_d = K^-1 - K^-1 diag(zeta_var[:, d]) K^-1 once per call, and
// the launch.
#include <hip/hip_runtime.h>
#include <cstring>
#include "../../include/cbfssm_hip.h"
#include "cbfssm_gp_mm.hpp"
#include "cbfssm_gp_host.hpp"

CBF_FOR_EACH_GPBWD_NBLK(CBF_GPMM_DECLARE)

namespace cbfssm {

static int gp_mm_maxwg(int NBLK)
{
    switch (NBLK) {
#define X(NB) case NB: return GpBwdCfg<NB>::MAXWG;
        CBF_FOR_EACH_GPBWD_NBLK(X)
#undef X
    }
    return 0;
}

static int dispatch_gp_mm(int NBLK, int DK, const GpMmArgs& a, unsigned nwg, hipStream_t st)
{
    switch (NBLK) {
#define X(NB) case NB: return launch_gp_mm_nb##NB(DK, a, nwg, st);
        CBF_FOR_EACH_GPBWD_NBLK(X)
#undef X
    }
    return -3;
}

// One wave per 16 x 16 tile (ib, jb) and output dimension d of W_d = K^-1 - K^-1 diag(s2_d) K^-1, the product on the f64
// MFMA units, stored in the accumulator layout the main kernel multiplies its Q tiles with:
//   Wimg[((d NBLK + ib) NBLK + jb) 256 + r 64 + lane] = W_d[16 ib + 4 r + lane / 16][16 jb + lane % 16],  zero beyond M.
// s2 is read from its operand image: s2[m][d] at s2B[(m / 16) 256 + (d / 4) 64 + 16 (d % 4) + m % 16].
__global__ __launch_bounds__(64) void gp_mm_w_kernel(const double* Kinv, const double* s2B, int M, int NBLK, double* Wimg)
{
    const int l = threadIdx.x, g = l >> 4, nl = l & 15;
    const int ib = blockIdx.x / NBLK, jb = blockIdx.x - ib * NBLK, d = blockIdx.y;
    const int row = 16 * ib + nl, col = 16 * jb + nl;
    d4 acc = {0, 0, 0, 0};
    for (int k0 = 0; k0 < M; k0 += 4) {
        const int k = k0 + g;
        double av = 0.0, bv = 0.0;
        if (k < M) {
            const double s2 = s2B[(k >> 4) * 256 + (d >> 2) * 64 + 16 * (d & 3) + (k & 15)];
            if (row < M) av = Kinv[row * M + k] * s2;
            if (col < M) bv = Kinv[k * M + col];
        }
        acc = CBF_MFMA(av, bv, acc);
    }
    double* out = Wimg + ((int64_t(d) * NBLK + ib) * NBLK + jb) * 256 + l;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int rr = 16 * ib + 4 * r + g;
        out[r * 64] = (rr < M && col < M) ? Kinv[rr * M + col] - acc[r] : 0.0;
    }
}

}  // namespace cbfssm

using namespace cbfssm;

extern "C" {

int64_t cbfssm_gp_moment_match_work_elems(const cbfssm_pack_layout* L)
{
    if (!gp_layout_ok(L)) return -1;
    return int64_t(16) * 16 * L->NBLK + int64_t(L->Do) * L->NBLK * L->NBLK * 256;
}

int cbfssm_gp_moment_match_f64(const cbfssm_pack_layout* L, const double* pack, const double* mean, const double* cov,
                               int64_t npts, double* fmean, double* fcov, double* xcov, double* info, double* work,
                               void* stream)
{
    if (!L) return fail(-1, "null layout");
    if (!gp_layout_ok(L))
        return fail(-3, "gp_moment_match limits: M <= %d, D <= 24, Do <= %d, and a layout of cbfssm_gp_pack_layout (M=%d D=%d Do=%d)",
                    CBFSSM_MAX_M, CBFSSM_MAX_DOUT, L->M, L->D, L->Do);
    if (npts < 0 || npts > (int64_t(1) << 34)) return fail(-1, "bad npts");
    if (!pack || !mean || !fmean || !fcov || !info || !work) return fail(-1, "null pointer");
    if (npts == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int tri = (L->gp_form == CBFSSM_GP_FORM_TRI);
    double* alpha = work;
    double* Wimg = work + int64_t(16) * 16 * L->NBLK;
    hipLaunchKernelGGL(gp_lin_alpha_kernel, dim3(16), dim3(256), 0, st, pack + L->Kinv, pack + L->Linvt, pack + L->muB, L->M,
                       L->Do, 16 * L->NBLK, tri, alpha);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-int(e) - 1000, "gp_moment_match: alpha launch failed");
    hipLaunchKernelGGL(gp_mm_w_kernel, dim3(L->NBLK * L->NBLK, L->Do), dim3(64), 0, st, pack + L->Kinv, pack + L->s2B, L->M,
                       L->NBLK, Wimg);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(-int(e) - 1000, "gp_moment_match: W launch failed");
    GpMmArgs a;
    memset(&a, 0, sizeof(a));
    a.Zp = pack + L->Zp; a.cz = pack + L->cz; a.invl = pack + L->invl; a.scal = pack + L->scal; a.Zs = pack + L->Zs;
    a.ZT = pack + L->ZT; a.alpha = alpha; a.Wimg = Wimg;
    a.mean = mean; a.cov = cov; a.fmean = fmean; a.fcov = fcov; a.xcov = xcov; a.info = info;
    a.npts = npts; a.nblocks = (npts + 15) / 16;
    a.M = L->M; a.D = L->D; a.Do = L->Do;
    const int64_t cap = gp_mm_maxwg(L->NBLK);                    // persistent over the point groups beyond that
    const unsigned nwg = unsigned(a.nblocks < cap ? a.nblocks : cap);
    int rc = dispatch_gp_mm(L->NBLK, L->DK, a, nwg, st);
    if (rc) return fail(rc, "gp_moment_match launch failed (NBLK=%d DK=%d rc=%d)", L->NBLK, L->DK, rc);
    return 0;
}

}  // extern "C"
