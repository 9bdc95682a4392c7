// Host side of the input adjoint of GPModel.moment_match (cbfssm_gp_mm_bwd.hpp): argument checks, the forward's two
// pre-kernels (alpha = K^-1 mu, the tiles of W_d) once per call, and the one adjoint launch.
#include <hip/hip_runtime.h>
#include <cstring>
#include "../../include/cbfssm_hip.h"
#include "cbfssm_gp_mm_bwd.hpp"
#include "cbfssm_gp_host.hpp"

CBF_FOR_EACH_GPBWD_NBLK(CBF_GPMMB_DECLARE)

namespace cbfssm {

static int gp_mmb_maxwg(int NBLK)
{
    switch (NBLK) {
#define X(NB) case NB: return GpBwdCfg<NB>::MAXWG;
        CBF_FOR_EACH_GPBWD_NBLK(X)
#undef X
    }
    return 0;
}

static int dispatch_gp_mmb(int NBLK, int DK, const GpMmBwdArgs& a, unsigned nwg, hipStream_t st)
{
    switch (NBLK) {
#define X(NB) case NB: return launch_gp_mmb_nb##NB(DK, a, nwg, st);
        CBF_FOR_EACH_GPBWD_NBLK(X)
#undef X
    }
    return -3;
}

// the forward's sections of `work`: alpha [16][16 NBLK], then the W_d tiles
static int64_t gp_mmb_fwd_elems(const cbfssm_pack_layout* L)
{
    return int64_t(16) * 16 * L->NBLK + int64_t(L->Do) * L->NBLK * L->NBLK * 256;
}

}  // namespace cbfssm

using namespace cbfssm;

extern "C" {

int64_t cbfssm_gp_moment_match_bwd_work_elems(const cbfssm_pack_layout* L)
{
    if (!gp_layout_ok(L)) return -1;
    return gp_mmb_fwd_elems(L) + int64_t(gp_mmb_maxwg(L->NBLK)) * gp_mmb_scratch(L->NBLK, L->DK);
}

int cbfssm_gp_moment_match_bwd_f64(const cbfssm_pack_layout* L, const double* pack, const double* mean, const double* cov,
                                   int64_t npts, const double* gfmean, const double* gfcov, const double* gxcov,
                                   double* gmean, double* gcov, double* info, double* work, void* stream)
{
    if (!L) return fail(-1, "null layout");
    if (!gp_layout_ok(L))
        return fail(-3, "gp_moment_match_bwd limits: M <= %d, D <= 24, Do <= %d, and a layout of cbfssm_gp_pack_layout (M=%d D=%d Do=%d)",
                    CBFSSM_MAX_M, CBFSSM_MAX_DOUT, L->M, L->D, L->Do);
    if (npts < 0 || npts > (int64_t(1) << 34)) return fail(-1, "bad npts");
    if (!pack || !mean || !gmean || !work) return fail(-1, "null pointer");
    if (!gfmean && !gfcov && !gxcov) return fail(-1, "gp_moment_match_bwd: no cotangent");
    if ((cov == nullptr) != (gcov == nullptr)) return fail(-1, "gp_moment_match_bwd: gcov goes with cov");
    if (npts == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int tri = (L->gp_form == CBFSSM_GP_FORM_TRI);
    double* alpha = work;
    double* Wimg = work + int64_t(16) * 16 * L->NBLK;
    hipLaunchKernelGGL(gp_lin_alpha_kernel, dim3(16), dim3(256), 0, st, pack + L->Kinv, pack + L->Linvt, pack + L->muB, L->M,
                       L->Do, 16 * L->NBLK, tri, alpha);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-int(e) - 1000, "gp_moment_match_bwd: alpha launch failed");
    hipLaunchKernelGGL(gp_mm_w_kernel, dim3(L->NBLK * L->NBLK, L->Do), dim3(64), 0, st, pack + L->Kinv, pack + L->s2B, L->M,
                       L->NBLK, Wimg);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(-int(e) - 1000, "gp_moment_match_bwd: W launch failed");
    GpMmBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.Zp = pack + L->Zp; a.cz = pack + L->cz; a.invl = pack + L->invl; a.scal = pack + L->scal; a.Zs = pack + L->Zs;
    a.ZT = pack + L->ZT; a.alpha = alpha; a.Wimg = Wimg;
    a.mean = mean; a.cov = cov; a.gfmean = gfmean; a.gfcov = gfcov; a.gxcov = gxcov;
    a.gmean = gmean; a.gcov = gcov; a.info = info; a.scratch = work + gp_mmb_fwd_elems(L);
    a.npts = npts; a.nblocks = (npts + 15) / 16;
    a.M = L->M; a.D = L->D; a.Do = L->Do;
    const int64_t cap = gp_mmb_maxwg(L->NBLK);                   // persistent over the point groups beyond that
    const unsigned nwg = unsigned(a.nblocks < cap ? a.nblocks : cap);
    int rc = dispatch_gp_mmb(L->NBLK, L->DK, a, nwg, st);
    if (rc) return fail(rc, "gp_moment_match_bwd launch failed (NBLK=%d DK=%d rc=%d)", L->NBLK, L->DK, rc);
    return 0;
}

}  // extern "C"
