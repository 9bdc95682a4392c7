// Host side of the input adjoint of GPModel.adf (cbfssm_gp_adf_bwd.hpp): the argument checks of cbfssm_gp_adf_f64, the
// forward's two pre-kernels (alpha = K^-1 mu, the tiles of W_d) once per call, the one reverse-time launch, and the sum of
// the workgroups' var_x / var_y slots in the order of the workgroups.
#include <hip/hip_runtime.h>
#include <cstring>
#include "../../include/cbfssm_hip.h"
#include "cbfssm_gp_adf_bwd.hpp"
#include "cbfssm_gp_host.hpp"

CBF_FOR_EACH_GPBWD_NBLK(CBF_GPADFB_DECLARE)

namespace cbfssm {

static int64_t gp_adfb_block_of(int NBLK, int DK)
{
    switch (NBLK) {
#define X(NB) case NB: return DK == 2 ? gp_adfb_block(NB, 2) : (DK == 4 ? gp_adfb_block(NB, 4) : gp_adfb_block(NB, 6));
        CBF_FOR_EACH_GPBWD_NBLK(X)
#undef X
    }
    return 0;
}

static int dispatch_gp_adfb(int NBLK, int DK, const GpAdfBwdArgs& a, hipStream_t st)
{
    switch (NBLK) {
#define X(NB) case NB: return launch_gp_adfb_nb##NB(DK, a, st);
        CBF_FOR_EACH_GPBWD_NBLK(X)
#undef X
    }
    return -3;
}

// the forward's sections of `work`: alpha [16][16 NBLK], then the W_d tiles
static int64_t gp_adfb_fwd_elems(const cbfssm_pack_layout* L)
{
    return int64_t(16) * 16 * L->NBLK + int64_t(L->Do) * L->NBLK * L->NBLK * 256;
}

// gvar_x[j] (j < Do, where asked for) and gvar_y[j] (j < Dy): the workgroups' slots in their order
__global__ void gp_adfb_fold_kernel(const double* sums, int64_t nwg, double* gvar_x, int Do, double* gvar_y, int Dy)
{
    const int tid = threadIdx.x, j = tid & 15;
    double* out = (tid < 16) ? gvar_x : gvar_y;
    if (tid >= 32 || !out || j >= ((tid < 16) ? Do : Dy)) return;
    double s = 0.0;
    for (int64_t k = 0; k < nwg; ++k) s += sums[k * 32 + tid];
    out[j] = s;
}

}  // namespace cbfssm

using namespace cbfssm;

extern "C" {

int64_t cbfssm_gp_adf_bwd_work_elems(const cbfssm_pack_layout* L, int64_t N)
{
    if (!gp_layout_ok(L, GP_NEED_STATE) || N < 0) return -1;
    const int64_t nwg = (N + 15) / 16;
    return gp_adfb_fwd_elems(L) + nwg * (gp_adfb_block_of(L->NBLK, L->DK) + 32);
}

int cbfssm_gp_adf_bwd_f64(const cbfssm_pack_layout* L, const double* pack, const double* m0, const double* P0, const double* a,
                          const double* y, const double* cond, const double* var_x, const double* var_y, int Dy,
                          const double* means, const double* covs, const double* pmeans, const double* pcovs,
                          const double* info, const double* gmeans, const double* gcovs, const double* gloglik, int64_t N,
                          int64_t T, double* gm0, double* gP0, double* ga, double* gy, double* gvar_x, double* gvar_y,
                          double* work, void* stream)
{
    if (int rc = gp_ekf_check_sizes("gp_adf_bwd", L, Dy, N, T)) return rc;
    if (!pack || !m0 || !y || !var_y || !means || !covs || !pmeans || !pcovs || !info || !gm0 || !gy || !gvar_y || !work)
        return fail(-1, "null pointer");
    if (L->D > L->Do && (!a || !ga)) return fail(-1, "null a or ga with D > Do");
    if (!gmeans && !gcovs && !gloglik) return fail(-1, "gp_adf_bwd: no cotangent");
    if ((P0 == nullptr) != (gP0 == nullptr)) return fail(-1, "gp_adf_bwd: gP0 goes with P0");
    if ((var_x == nullptr) != (gvar_x == nullptr)) return fail(-1, "gp_adf_bwd: gvar_x goes with var_x");
    if (N == 0 || T == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int tri = (L->gp_form == CBFSSM_GP_FORM_TRI);
    const int64_t nwg = (N + 15) / 16;
    double* alpha = work;
    double* Wimg = work + int64_t(16) * 16 * L->NBLK;
    hipLaunchKernelGGL(gp_lin_alpha_kernel, dim3(16), dim3(256), 0, st, pack + L->Kinv, pack + L->Linvt, pack + L->muB, L->M,
                       L->Do, 16 * L->NBLK, tri, alpha);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-int(e) - 1000, "gp_adf_bwd: alpha launch failed");
    hipLaunchKernelGGL(gp_mm_w_kernel, dim3(L->NBLK * L->NBLK, L->Do), dim3(64), 0, st, pack + L->Kinv, pack + L->s2B, L->M,
                       L->NBLK, Wimg);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(-int(e) - 1000, "gp_adf_bwd: W launch failed");
    GpAdfBwdArgs k;
    memset(&k, 0, sizeof(k));
    k.mm.Zp = pack + L->Zp; k.mm.cz = pack + L->cz; k.mm.invl = pack + L->invl; k.mm.scal = pack + L->scal;
    k.mm.Zs = pack + L->Zs; k.mm.ZT = pack + L->ZT; k.mm.alpha = alpha; k.mm.Wimg = Wimg;
    k.mm.M = L->M; k.mm.D = L->D; k.mm.Do = L->Do;
    k.m0 = m0; k.P0 = P0; k.a = a; k.y = y; k.cond = cond; k.var_y = var_y;
    k.means = means; k.covs = covs; k.pmeans = pmeans; k.pcovs = pcovs; k.info = info;
    k.gmeans = gmeans; k.gcovs = gcovs; k.gloglik = gloglik;
    k.gm0 = gm0; k.gP0 = gP0; k.ga = ga; k.gy = gy;
    k.block = work + gp_adfb_fwd_elems(L);
    k.sums = k.block + nwg * gp_adfb_block_of(L->NBLK, L->DK);
    k.N = int(N); k.T = int(T); k.Dy = Dy;
    int rc = dispatch_gp_adfb(L->NBLK, L->DK, k, st);
    if (rc) return fail(rc, "gp_adf_bwd launch failed (NBLK=%d DK=%d rc=%d)", L->NBLK, L->DK, rc);
    hipLaunchKernelGGL(gp_adfb_fold_kernel, dim3(1), dim3(32), 0, st, k.sums, nwg, gvar_x, L->Do, gvar_y, Dy);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(-int(e) - 1000, "gp_adf_bwd: fold launch failed");
    return 0;
}

}  // extern "C"
