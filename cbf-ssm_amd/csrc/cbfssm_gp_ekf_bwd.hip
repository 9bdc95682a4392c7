// Host side of the adjoint of GPModel.ekf (cbfssm_gp_ekf_bwd.hpp): argument checks, the alpha pre-kernel, the launch (one
// workgroup per 16 chains) and, at stash heights, the contraction of the K^-1 adjoint's operand images.
#include <hip/hip_runtime.h>
#include <cstring>
#include "../../include/cbfssm_hip.h"
#include "cbfssm_gp_ekf_bwd.hpp"

CBF_FOR_EACH_GPBWD_NBLK(CBF_GPEKFBWD_DECLARE)

namespace cbfssm {

int fail(int rc, const char* fmt, ...);   // cbfssm_api.hip

// cbfssm_gp_lin.hip
__global__ void gp_lin_alpha_kernel(const double* Kinv, const double* G, const double* muB, int M, int Do, int MP, int tri,
                                    double* alpha);
// cbfssm_gp_ekf.hip
bool gp_ekf_layout_ok(const cbfssm_pack_layout* L);
int gp_ekf_check_sizes(const char* who, const cbfssm_pack_layout* L, int Dy, int64_t N, int64_t T);

static int dispatch_gp_ekf_bwd(int NBLK, int DK, const GpEkfBwdArgs& a, hipStream_t st)
{
    switch (NBLK) {
#define X(NB) case NB: return launch_gp_ekf_bwd_nb##NB(DK, a, st);
        CBF_FOR_EACH_GPBWD_NBLK(X)
#undef X
    }
    return -3;
}

// the filter's limits and what the adjoint needs of the layout: a slab, and stash mode exactly above seven row blocks
static bool gp_ekf_bwd_layout_ok(const cbfssm_pack_layout* L)
{
    if (!gp_ekf_layout_ok(L)) return false;
    if (L->rev_slab <= 0 || (L->rev_stash != 0) != (L->NBLK > 7)) return false;
    if (L->gp_form != CBFSSM_GP_FORM_DENSE && L->gp_form != CBFSSM_GP_FORM_TRI) return false;
    return true;
}

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
    if (!gp_ekf_bwd_layout_ok(L) || N < 0 || N > (int64_t(1) << 30)) return -1;
    return (N + 15) / 16;
}

int64_t cbfssm_gp_ekf_bwd_work_elems(const cbfssm_pack_layout* L, int64_t N, int64_t T)
{
    if (!gp_ekf_bwd_layout_ok(L) || N < 0 || N > (int64_t(1) << 30) || T < 0 || T > (int64_t(1) << 24)) return -1;
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
    if (!gp_ekf_bwd_layout_ok(L)) return fail(-3, "gp_ekf_bwd: the layout has no adjoint (rev_slab, rev_stash, gp_form)");
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
    g.pk.Bp = pack + L->Bp; g.pk.Zp = pack + L->Zp; g.pk.cz = pack + L->cz; g.pk.muA = pack + L->muA; g.pk.s2A = pack + L->s2A;
    g.pk.invl = pack + L->invl; g.pk.scal = pack + L->scal; g.pk.KSr = (L->M + 3) / 4;
    g.pk.Wp = pack + L->Wp; g.pk.WTp = pack + L->WTp;
    g.rk.muB = pack + L->muB; g.rk.s2B = pack + L->s2B; g.rk.ZT = pack + L->ZT;
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
