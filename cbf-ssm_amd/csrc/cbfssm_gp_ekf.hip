// Host side of GPModel.ekf (cbfssm_gp_ekf.hpp): argument checks, the pre-kernel of GPModel.linearize that forms
// alpha = K^-1 mu once per call (gp_lin_alpha_kernel, cbfssm_gp_lin.hip), and the launch: one workgroup per 16 chains.
#include <hip/hip_runtime.h>
#include <cstring>
#include "../../include/cbfssm_hip.h"
#include "cbfssm_gp_ekf.hpp"
#include "cbfssm_gp_host.hpp"

CBF_FOR_EACH_GPBWD_NBLK(CBF_GPEKF_DECLARE)

namespace cbfssm {

static int dispatch_gp_ekf(int NBLK, int DK, const GpEkfArgs& a, hipStream_t st)
{
    switch (NBLK) {
#define X(NB) case NB: return launch_gp_ekf_nb##NB(DK, a, st);
        CBF_FOR_EACH_GPBWD_NBLK(X)
#undef X
    }
    return -3;
}

// what cbfssm_gp_ekf_f64 and cbfssm_gp_eks_f64 (cbfssm_gp_eks.hip) refuse before they look at a pointer
int gp_ekf_check_sizes(const char* who, const cbfssm_pack_layout* L, int Dy, int64_t N, int64_t T)
{
    if (!L) return fail(-1, "null layout");
    if (N < 0 || T < 0 || Dy < 0) return fail(-1, "negative size");
    if (!gp_layout_ok(L, GP_NEED_STATE))
        return fail(-3, "%s limits: M <= %d, Do <= D <= 24, Do <= %d, and a layout of cbfssm_gp_pack_layout (M=%d D=%d Do=%d)",
                    who, CBFSSM_MAX_M, CBFSSM_MAX_DOUT, L->M, L->D, L->Do);
    if (Dy < 1 || Dy > L->Do) return fail(-3, "%s: 1 <= Dy <= Do (Dy=%d Do=%d)", who, Dy, L->Do);
    if (N > (int64_t(1) << 30) || T > (int64_t(1) << 24)) return fail(-3, "%s: N <= 2^30, T <= 2^24", who);
    return 0;
}

// the alpha pre-kernel and the filter launch; pmeans, pcovs, cross: all three or none (the smoother's inputs); jac: with
// those three, the forward under grad
static int gp_ekf_launch_j(const char* who, const cbfssm_pack_layout* L, const double* pack, const double* m0, const double* P0,
                           const double* a, const double* y, const double* cond, const double* var_x, const double* var_y,
                           int Dy, int64_t N, int64_t T, double* means, double* covs, double* loglik, double* pmeans,
                           double* pcovs, double* cross, double* jac, double* work, hipStream_t st)
{
    const int tri = (L->gp_form == CBFSSM_GP_FORM_TRI);
    hipLaunchKernelGGL(gp_lin_alpha_kernel, dim3(16), dim3(256), 0, st, pack + L->Kinv, pack + L->Linvt, pack + L->muB, L->M,
                       L->Do, 16 * L->NBLK, tri, work);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-int(e) - 1000, "%s: alpha launch failed", who);
    GpEkfArgs k;
    memset(&k, 0, sizeof(k));
    gp_pack_ptrs(L, pack, k.pk, k.rk);
    k.m0 = m0; k.P0 = P0; k.a = a; k.y = y; k.cond = cond; k.var_x = var_x; k.var_y = var_y; k.alpha = work;
    k.means = means; k.covs = covs; k.loglik = loglik; k.pmeans = pmeans; k.pcovs = pcovs; k.cross = cross;
    k.N = int(N); k.T = int(T); k.M = L->M; k.D = L->D; k.Do = L->Do; k.Dy = Dy; k.tri = tri;
    k.jac = jac;
    int rc = dispatch_gp_ekf(L->NBLK, L->DK, k, st);
    if (rc) return fail(rc, "%s launch failed (NBLK=%d DK=%d rc=%d)", who, L->NBLK, L->DK, rc);
    return 0;
}

int gp_ekf_launch(const char* who, const cbfssm_pack_layout* L, const double* pack, const double* m0, const double* P0,
                  const double* a, const double* y, const double* cond, const double* var_x, const double* var_y, int Dy,
                  int64_t N, int64_t T, double* means, double* covs, double* loglik, double* pmeans, double* pcovs,
                  double* cross, double* work, hipStream_t st)
{
    return gp_ekf_launch_j(who, L, pack, m0, P0, a, y, cond, var_x, var_y, Dy, N, T, means, covs, loglik, pmeans, pcovs, cross,
                           nullptr, work, st);
}

}  // namespace cbfssm

using namespace cbfssm;

extern "C" {

int64_t cbfssm_gp_ekf_work_elems(const cbfssm_pack_layout* L)
{
    if (!gp_layout_ok(L, GP_NEED_STATE)) return -1;
    return int64_t(16) * 16 * L->NBLK;
}

int cbfssm_gp_ekf_f64(const cbfssm_pack_layout* L, const double* pack, const double* m0, const double* P0, const double* a,
                      const double* y, const double* cond, const double* var_x, const double* var_y, int Dy, int64_t N,
                      int64_t T, double* means, double* covs, double* loglik, double* work, void* stream)
{
    if (int rc = gp_ekf_check_sizes("gp_ekf", L, Dy, N, T)) return rc;
    if (!pack || !m0 || !y || !var_y || !means || !covs || !loglik || !work) return fail(-1, "null pointer");
    if (L->D > L->Do && !a) return fail(-1, "null a with D > Do");
    if (N == 0 || T == 0) return 0;
    return gp_ekf_launch("gp_ekf", L, pack, m0, P0, a, y, cond, var_x, var_y, Dy, N, T, means, covs, loglik, nullptr, nullptr,
                         nullptr, work, (hipStream_t)stream);
}

// the forward under grad: the filter alone (no smoother launches), leaving what cbfssm_gp_ekf_bwd_f64 reads
int cbfssm_gp_ekf_save_f64(const cbfssm_pack_layout* L, const double* pack, const double* m0, const double* P0, const double* a,
                           const double* y, const double* cond, const double* var_x, const double* var_y, int Dy, int64_t N,
                           int64_t T, double* means, double* covs, double* loglik, double* pmeans, double* pcovs, double* cross,
                           double* jac, double* work, void* stream)
{
    if (int rc = gp_ekf_check_sizes("gp_ekf_save", L, Dy, N, T)) return rc;
    if (!pack || !m0 || !y || !var_y || !means || !covs || !loglik || !pmeans || !pcovs || !cross || !jac || !work)
        return fail(-1, "null pointer");
    if (L->D > L->Do && !a) return fail(-1, "null a with D > Do");
    if (N == 0 || T == 0) return 0;
    return gp_ekf_launch_j("gp_ekf_save", L, pack, m0, P0, a, y, cond, var_x, var_y, Dy, N, T, means, covs, loglik, pmeans,
                           pcovs, cross, jac, work, (hipStream_t)stream);
}

}  // extern "C"
