// Host side of the adjoint of GPModel.ekf (cbfssm_gp_ekf_bwd.hpp): argument checks, the alpha pre-kernel, the launch (one
// workgroup per 16 chains) and, at stash heights, the contraction of the K^-1 adjoint's operand images.
#include <hip/hip_runtime.h>
#include <cstring>
#include "../../include/cbfssm_hip.h"
#include "cbfssm_gp_ekf_bwd.hpp"
#include "cbfssm_gp_host.hpp"

CBF_FOR_EACH_GPBWD_NBLK(CBF_GPEKFBWD_DECLARE)

namespace cbfssm {

static int dispatch_gp_ekf_bwd(int NBLK, int DK, const GpEkfBwdArgs& a, hipStream_t st)
{
    switch (NBLK) {
#define X(NB) case NB: return launch_gp_ekf_bwd_nb##NB(DK, a, st);
        CBF_FOR_EACH_GPBWD_NBLK(X)
#undef X
    }
    return -3;
}

// the filter's limits (Do <= D) and what the adjoint needs of the layout: a slab, stash mode exactly above seven row
// blocks, a GP form
static const unsigned kNeeds = GP_NEED_ADJOINT | GP_NEED_FORM | GP_NEED_STATE;

// work: alpha | Pb rows | Jh | stash_a | stash_k | contraction scratch
static int64_t ekf_bwd_fixed_elems(const cbfssm_pack_layout* L, int64_t groups)
{
    return int64_t(16) * 16 * L->NBLK + 2 * groups * 4096;
}

}  // namespace cbfssm

using namespace cbfssm;

extern "C" {

int64_t cbfssm_gp_ekf_bwd_workgroups(const cbfssm_pack_layout* L, int64_t N)
{
    if (!gp_layout_ok(L, kNeeds) || N < 0 || N > (int64_t(1) << 30)) return -1;
    return (N + 15) / 16;
}

int64_t cbfssm_gp_ekf_bwd_work_elems(const cbfssm_pack_layout* L, int64_t N, int64_t T)
{
    if (!gp_layout_ok(L, kNeeds) || N < 0 || N > (int64_t(1) << 30) || T < 0 || T > (int64_t(1) << 24)) return -1;
    const int64_t groups = (N + 15) / 16;
    int64_t n = ekf_bwd_fixed_elems(L, groups);
    if (L->rev_stash) {
        const int64_t nslots = groups * (T + 1);        // one slot per step and one for the alpha fold
        n += 2 * nslots * L->NBLK * 256 + cbfssm_stash_contract_work_elems(L, nslots);
    }
    return n;
}

int cbfssm_gp_ekf_bwd_f64(const cbfssm_pack_layout* L, const double* pack, const double* m0, const double* P0, const double* a,
                          const double* y, const double* cond, const double* var_x, const double* var_y, int Dy,
                          const double* means, const double* covs, const double* pmeans, const double* pcovs,
                          const double* cross, const double* jac, const double* gmeans, const double* gcovs,
                          const double* gloglik, int64_t N, int64_t T, double* gm0, double* gP0, double* ga, double* gy,
                          double* gpart, double* work, double* gB_image, void* stream)
{
    if (int rc = gp_ekf_check_sizes("gp_ekf_bwd", L, Dy, N, T)) return rc;
    if (!gp_layout_ok(L, kNeeds)) return fail(-3, "gp_ekf_bwd: the layout has no adjoint (rev_slab, rev_stash, gp_form)");
    if (!pack || !m0 || !y || !var_y || !means || !covs || !pmeans || !pcovs || !cross || !jac || !gm0 || !gy || !gpart || !work)
        return fail(-1, "gp_ekf_bwd: null pointer");
    if (L->D > L->Do && (!a || !ga)) return fail(-1, "gp_ekf_bwd: D=%d > Do=%d needs a and ga", L->D, L->Do);
    if (L->rev_stash && !gB_image) return fail(-1, "gp_ekf_bwd: M=%d (> 112) needs gB_image", L->M);
    if (N == 0 || T == 0) return 0;
    (void)P0; (void)var_x;                              // (they enter through pcovs, cross: their adjoints need no value)
    hipStream_t st = (hipStream_t)stream;
    const int tri = (L->gp_form == CBFSSM_GP_FORM_TRI);
    hipLaunchKernelGGL(gp_lin_alpha_kernel, dim3(16), dim3(256), 0, st, pack + L->Kinv, pack + L->Linvt, pack + L->muB, L->M,
                       L->Do, 16 * L->NBLK, tri, work);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-int(e) - 1000, "gp_ekf_bwd: alpha launch failed");
    const int64_t groups = (N + 15) / 16;
    GpEkfBwdArgs g;
    memset(&g, 0, sizeof(g));
    gp_pack_ptrs(L, pack, g.pk, g.rk);
    g.m0 = m0; g.a = a; g.y = y; g.cond = cond; g.var_y = var_y; g.alpha = work;
    g.means = means; g.pmeans = pmeans; g.pcovs = pcovs; g.cross = cross; g.jac = jac;
    g.gmeans = gmeans; g.gcovs = gcovs; g.gloglik = gloglik;
    g.gm0 = gm0; g.gP0 = gP0; g.ga = ga; g.gy = gy; g.gpart = gpart; g.slab = L->rev_slab;
    g.wP = work + int64_t(16) * 16 * L->NBLK;
    g.wJ = g.wP + groups * 4096;
    g.N = int(N); g.T = int(T); g.M = L->M; g.D = L->D; g.Do = L->Do; g.Dy = Dy;
    const int64_t nslots = groups * (T + 1);
    double* stash = work + ekf_bwd_fixed_elems(L, groups);
    if (L->rev_stash) {
        g.stash_a = stash;
        g.stash_k = stash + nslots * L->NBLK * 256;
        g.fold_slot0 = groups * T;
        e = hipMemsetAsync(gB_image, 0, size_t(L->NBLK) * L->NBLK * 256 * sizeof(double), st);
        if (e != hipSuccess) return fail(-int(e) - 1000, "gp_ekf_bwd: clearing the K^-1 adjoint image failed");
    }
    int rc = dispatch_gp_ekf_bwd(L->NBLK, L->DK, g, st);
    if (rc) return fail(rc, "gp_ekf_bwd launch failed (NBLK=%d DK=%d rc=%d)", L->NBLK, L->DK, rc);
    if (L->rev_stash)
        return cbfssm_stash_contract_f64(L, g.stash_a, g.stash_k, nslots, stash + 2 * nslots * L->NBLK * 256, gB_image, stream);
    return 0;
}

}  // extern "C"
