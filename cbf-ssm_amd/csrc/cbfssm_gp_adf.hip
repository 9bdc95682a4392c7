// Host side of GPModel.adf and GPModel.ads (cbfssm_gp_adf.hpp): the argument checks of cbfssm_gp_ekf_f64, the two
// pre-kernels of GPModel.moment_match that form alpha = K^-1 mu (gp_lin_alpha_kernel, cbfssm_gp_lin.hip) and the tiles of
// W_d (gp_mm_w_kernel, cbfssm_gp_mm.hip) once per call, and the time-loop launch: one workgroup per 16 chains.  ads chains
// the two smoother launches of GPModel.eks behind it on the same stream (gp_eks_sweep_launch, cbfssm_gp_eks.hip).
#include <hip/hip_runtime.h>
#include <cstring>
#include "../../include/cbfssm_hip.h"
#include "cbfssm_gp_adf.hpp"
#include "cbfssm_gp_host.hpp"

CBF_FOR_EACH_GPBWD_NBLK(CBF_GPADF_DECLARE)

namespace cbfssm {

static int dispatch_gp_adf(int NBLK, int DK, const GpAdfArgs& a, hipStream_t st)
{
    switch (NBLK) {
#define X(NB) case NB: return launch_gp_adf_nb##NB(DK, a, st);
        CBF_FOR_EACH_GPBWD_NBLK(X)
#undef X
    }
    return -3;
}

// info of ads: the forward pass's where that is non-zero, else the sweep's
__global__ void gp_ads_info_kernel(const double* sweep, double* info, int64_t N)
{
    const int64_t n = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (n < N && info[n] == 0.0) info[n] = sweep[n];
}

static int gp_adf_launch(const char* who, const cbfssm_pack_layout* L, const double* pack, const double* m0, const double* P0,
                         const double* a, const double* y, const double* cond, const double* var_x, const double* var_y,
                         int Dy, int64_t N, int64_t T, double* means, double* covs, double* loglik, double* pmeans,
                         double* pcovs, double* cross, double* info, double* work, hipStream_t st)
{
    const int tri = (L->gp_form == CBFSSM_GP_FORM_TRI);
    double* alpha = work;
    double* Wimg = work + int64_t(16) * 16 * L->NBLK;
    hipLaunchKernelGGL(gp_lin_alpha_kernel, dim3(16), dim3(256), 0, st, pack + L->Kinv, pack + L->Linvt, pack + L->muB, L->M,
                       L->Do, 16 * L->NBLK, tri, alpha);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-int(e) - 1000, "%s: alpha launch failed", who);
    hipLaunchKernelGGL(gp_mm_w_kernel, dim3(L->NBLK * L->NBLK, L->Do), dim3(64), 0, st, pack + L->Kinv, pack + L->s2B, L->M,
                       L->NBLK, Wimg);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(-int(e) - 1000, "%s: W launch failed", who);
    GpAdfArgs k;
    memset(&k, 0, sizeof(k));
    k.Zp = pack + L->Zp; k.cz = pack + L->cz; k.invl = pack + L->invl; k.scal = pack + L->scal; k.Zs = pack + L->Zs;
    k.ZT = pack + L->ZT; k.alpha = alpha; k.Wimg = Wimg;
    k.m0 = m0; k.P0 = P0; k.a = a; k.y = y; k.cond = cond; k.var_x = var_x; k.var_y = var_y;
    k.means = means; k.covs = covs; k.loglik = loglik; k.pmeans = pmeans; k.pcovs = pcovs; k.cross = cross; k.info = info;
    k.N = int(N); k.T = int(T); k.M = L->M; k.D = L->D; k.Do = L->Do; k.Dy = Dy;
    int rc = dispatch_gp_adf(L->NBLK, L->DK, k, st);
    if (rc) return fail(rc, "%s launch failed (NBLK=%d DK=%d rc=%d)", who, L->NBLK, L->DK, rc);
    return 0;
}

}  // namespace cbfssm

using namespace cbfssm;

extern "C" {

int64_t cbfssm_gp_adf_work_elems(const cbfssm_pack_layout* L)
{
    if (!gp_layout_ok(L, GP_NEED_STATE)) return -1;                // moment_match's limits and D >= Do
    return int64_t(16) * 16 * L->NBLK + int64_t(L->Do) * L->NBLK * L->NBLK * 256;
}

int cbfssm_gp_adf_f64(const cbfssm_pack_layout* L, const double* pack, const double* m0, const double* P0, const double* a,
                      const double* y, const double* cond, const double* var_x, const double* var_y, int Dy, int64_t N,
                      int64_t T, double* means, double* covs, double* loglik, double* pmeans, double* pcovs, double* cross,
                      double* info, double* work, void* stream)
{
    if (int rc = gp_ekf_check_sizes("gp_adf", L, Dy, N, T)) return rc;
    if (!pack || !m0 || !y || !var_y || !means || !covs || !loglik || !pmeans || !pcovs || !cross || !info || !work)
        return fail(-1, "null pointer");
    if (L->D > L->Do && !a) return fail(-1, "null a with D > Do");
    if (N == 0 || T == 0) return 0;
    return gp_adf_launch("gp_adf", L, pack, m0, P0, a, y, cond, var_x, var_y, Dy, N, T, means, covs, loglik, pmeans, pcovs,
                         cross, info, work, (hipStream_t)stream);
}

// cross is an input of the gains only: once they are formed, its first N entries carry the sweep's info to the kernel that
// merges it with the forward pass's (no buffer beyond the arguments)
int cbfssm_gp_ads_f64(const cbfssm_pack_layout* L, const double* pack, const double* m0, const double* P0, const double* a,
                      const double* y, const double* cond, const double* var_x, const double* var_y, int Dy, int64_t N,
                      int64_t T, double* means, double* covs, double* loglik, double* pmeans, double* pcovs, double* cross,
                      double* smeans, double* scovs, double* sm_init, double* sP_init, double* lag1, double* info,
                      double* work, void* stream)
{
    if (int rc = gp_ekf_check_sizes("gp_ads", L, Dy, N, T)) return rc;
    if (!pack || !m0 || !y || !var_y || !means || !covs || !loglik || !pmeans || !pcovs || !cross || !smeans || !scovs ||
        !sm_init || !sP_init || !info || !work)
        return fail(-1, "null pointer");
    if (L->D > L->Do && !a) return fail(-1, "null a with D > Do");
    if (N == 0 || T == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    int rc = gp_adf_launch("gp_ads", L, pack, m0, P0, a, y, cond, var_x, var_y, Dy, N, T, means, covs, loglik, pmeans, pcovs,
                           cross, info, work, st);
    if (rc) return rc;
    rc = gp_eks_sweep_launch("gp_ads", m0, P0, means, covs, pmeans, pcovs, cross, smeans, scovs, sm_init, sP_init, lag1, cross,
                             N, T, L->Do, st);
    if (rc) return rc;
    hipLaunchKernelGGL(gp_ads_info_kernel, dim3(unsigned((N + 255) / 256)), dim3(256), 0, st, cross, info, N);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-int(e) - 1000, "gp_ads: info launch failed");
    return 0;
}

}  // extern "C"
