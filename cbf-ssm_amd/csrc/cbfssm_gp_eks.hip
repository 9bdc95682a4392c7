// Host side of GPModel.eks (cbfssm_gp_eks.hpp): the argument checks of cbfssm_gp_ekf_f64, then four launches on one
// stream -- the alpha pre-kernel and gp_ekf_kernel in its EMIT form (cbfssm_gp_ekf.hip), gp_eks_gain_kernel over
// (four chains, step) and gp_eks_sweep_kernel, one wave per four chains.
#include <hip/hip_runtime.h>
#include "../../include/cbfssm_hip.h"
#include "cbfssm_gp_eks.hpp"
#include "cbfssm_gp_host.hpp"

namespace cbfssm {

// the two smoother launches behind a forward pass that left means, covs, pmeans, pcovs and cross (also behind GPModel.adf:
// cbfssm_gp_adf.hip)
int gp_eks_sweep_launch(const char* who, const double* m0, const double* P0, const double* means, const double* covs,
                        const double* pmeans, const double* pcovs, const double* cross, double* smeans, double* scovs,
                        double* sm_init, double* sP_init, double* lag1, double* info, int64_t N, int64_t T, int Do,
                        hipStream_t st)
{
    GpEksArgs k;
    k.m0 = m0; k.P0 = P0; k.means = means; k.covs = covs; k.pmeans = pmeans; k.pcovs = pcovs; k.cross = cross;
    k.smeans = smeans; k.scovs = scovs; k.sm_init = sm_init; k.sP_init = sP_init; k.lag1 = lag1; k.info = info;
    k.N = int(N); k.T = int(T); k.Do = Do;
    const unsigned groups = unsigned((N + EKS_CHAINS - 1) / EKS_CHAINS);
    hipLaunchKernelGGL(gp_eks_gain_kernel, dim3(groups, unsigned(T < 65535 ? T : 65535)), dim3(64), 0, st, k);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-int(e) - 1000, "%s: gain launch failed", who);
    hipLaunchKernelGGL(gp_eks_sweep_kernel, dim3(groups), dim3(64), 0, st, k);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(-int(e) - 1000, "%s: sweep launch failed", who);
    return 0;
}

}  // namespace cbfssm

using namespace cbfssm;

extern "C" {

int64_t cbfssm_gp_eks_work_elems(const cbfssm_pack_layout* L)
{
    if (!gp_layout_ok(L, GP_NEED_STATE)) return -1;
    return int64_t(16) * 16 * L->NBLK;                  // alpha = K^-1 mu of the forward kernel; the sweep needs none
}

int cbfssm_gp_eks_f64(const cbfssm_pack_layout* L, const double* pack, const double* m0, const double* P0, const double* a,
                      const double* y, const double* cond, const double* var_x, const double* var_y, int Dy, int64_t N,
                      int64_t T, double* means, double* covs, double* loglik, double* pmeans, double* pcovs, double* cross,
                      double* smeans, double* scovs, double* sm_init, double* sP_init, double* lag1, double* info,
                      double* work, void* stream)
{
    if (int rc = gp_ekf_check_sizes("gp_eks", L, Dy, N, T)) return rc;
    if (!pack || !m0 || !y || !var_y || !means || !covs || !loglik || !pmeans || !pcovs || !cross || !smeans || !scovs ||
        !sm_init || !sP_init || !info || !work)
        return fail(-1, "null pointer");
    if (L->D > L->Do && !a) return fail(-1, "null a with D > Do");
    if (N == 0 || T == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    int rc = gp_ekf_launch("gp_eks", L, pack, m0, P0, a, y, cond, var_x, var_y, Dy, N, T, means, covs, loglik, pmeans, pcovs,
                           cross, work, st);
    if (rc) return rc;
    return gp_eks_sweep_launch("gp_eks", m0, P0, means, covs, pmeans, pcovs, cross, smeans, scovs, sm_init, sP_init, lag1,
                               info, N, T, L->Do, st);
}

}  // extern "C"
