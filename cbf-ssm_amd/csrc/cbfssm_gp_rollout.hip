// Host side of the fused GP rollout and its adjoint (cbfssm_gp_rollout.hpp): argument checks, grids, stash contraction.
#include <hip/hip_runtime.h>
#include <cstring>
#include "../../include/cbfssm_hip.h"
#include "cbfssm_gp_rollout.hpp"
#include "cbfssm_gp_host.hpp"

CBF_FOR_EACH_GPBWD_NBLK(CBF_GPROLL_DECLARE)

namespace cbfssm {

static const int64_t kMaxChains = int64_t(1) << 30;    // as the pass kernels
static const int64_t kMaxSteps = int64_t(1) << 24;
// of the layout: the adjoint's fields (the forward asks for them too), a GP form, Do <= D
static const unsigned kNeeds = GP_NEED_ADJOINT | GP_NEED_FORM | GP_NEED_STATE;

static int dispatch_gp_roll(int NBLK, int DK, const GpRollArgs& a, hipStream_t st)
{
    switch (NBLK) {
#define X(NB) case NB: return launch_gp_roll_nb##NB(DK, a, st);
        CBF_FOR_EACH_GPBWD_NBLK(X)
#undef X
    }
    return -3;
}

static int dispatch_gp_roll_bwd(int NBLK, int DK, const GpRollBwdArgs& a, hipStream_t st)
{
    switch (NBLK) {
#define X(NB) case NB: return launch_gp_roll_bwd_nb##NB(DK, a, st);
        CBF_FOR_EACH_GPBWD_NBLK(X)
#undef X
    }
    return -3;
}


static int check_sizes(const cbfssm_pack_layout* L, int64_t N, int64_t T, const char* who)
{
    if (!L) return fail(-1, "%s: null layout", who);
    if (!gp_layout_ok(L, kNeeds))
        return fail(-3, "%s limits: M <= %d, Do <= D <= 24, Do <= %d, and a layout of cbfssm_gp_pack_layout (M=%d D=%d Do=%d)",
                    who, CBFSSM_MAX_M, CBFSSM_MAX_DOUT, L->M, L->D, L->Do);
    if (N < 0 || T < 1) return fail(-1, "%s: N=%lld must be >= 0 and T=%lld >= 1", who, (long long)N, (long long)T);
    if (N > kMaxChains || T > kMaxSteps) return fail(-3, "%s: N <= 2^30 chains, T <= 2^24 steps", who);
    return 0;
}

}  // namespace cbfssm

using namespace cbfssm;

extern "C" {

int64_t cbfssm_gp_rollout_partials(const cbfssm_pack_layout* L, int64_t N)
{
    if (!gp_layout_ok(L, kNeeds) || N < 0 || N > kMaxChains) return -1;
    return (N + 15) / 16;
}

int64_t cbfssm_gp_rollout_bwd_workgroups(const cbfssm_pack_layout* L, int64_t N)
{
    if (!gp_layout_ok(L, kNeeds) || N < 0 || N > kMaxChains) return -1;
    return (N + 15) / 16;
}

int64_t cbfssm_gp_rollout_bwd_work_elems(const cbfssm_pack_layout* L, int64_t N, int64_t T)
{
    if (!gp_layout_ok(L, kNeeds) || N < 0 || N > kMaxChains || T < 0 || T > kMaxSteps) return -1;
    if (!L->rev_stash) return 0;
    const int64_t nslots = (N + 15) / 16 * T;
    return 2 * nslots * L->NBLK * 256 + cbfssm_stash_contract_work_elems(L, nslots);
}

int cbfssm_gp_rollout_f64(const cbfssm_pack_layout* L, const double* pack, const double* h0, const double* a,
                          const double* eps, const double* var_add, int64_t N, int64_t T, int reverse, double* traj,
                          double* vsave, double* ent_part, void* stream)
{
    int rc = check_sizes(L, N, T, "gp_rollout");
    if (rc) return rc;
    if (!pack || !h0 || !eps || !traj || !ent_part) return fail(-1, "gp_rollout: null pointer");
    if (L->D > L->Do && !a) return fail(-1, "gp_rollout: D=%d > Do=%d needs the auxiliary inputs a", L->D, L->Do);
    if (N == 0) return 0;
    GpRollArgs g;
    memset(&g, 0, sizeof(g));
    gp_pack_ptrs(L, pack, g.pk);
    g.h0 = h0; g.a = a; g.eps = eps; g.var_add = var_add; g.traj = traj; g.vsave = vsave; g.ent_part = ent_part;
    g.N = int(N); g.T = int(T); g.D = L->D; g.Do = L->Do; g.reverse = reverse ? 1 : 0;
    g.tri = (L->gp_form == CBFSSM_GP_FORM_TRI);
    rc = dispatch_gp_roll(L->NBLK, L->DK, g, (hipStream_t)stream);
    if (rc) return fail(rc, "gp_rollout launch failed (NBLK=%d DK=%d rc=%d)", L->NBLK, L->DK, rc);
    return 0;
}

int cbfssm_gp_rollout_bwd_f64(const cbfssm_pack_layout* L, const double* pack, const double* h0, const double* a,
                              const double* eps, const double* traj, const double* vsave, const double* gtraj,
                              const double* g_ent, int64_t N, int64_t T, int reverse, double* gh0, double* ga,
                              double* gpart, double* work, double* gB_image, void* stream)
{
    int rc = check_sizes(L, N, T, "gp_rollout_bwd");
    if (rc) return rc;
    if (!pack || !h0 || !eps || !traj || !vsave || !gtraj || !g_ent || !gh0 || !gpart)
        return fail(-1, "gp_rollout_bwd: null pointer");
    if (L->D > L->Do && (!a || !ga)) return fail(-1, "gp_rollout_bwd: D=%d > Do=%d needs a and ga", L->D, L->Do);
    if (L->rev_stash && (!work || !gB_image)) return fail(-1, "gp_rollout_bwd: M=%d (> 112) needs work and gB_image", L->M);
    if (N == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    GpRollBwdArgs g;
    memset(&g, 0, sizeof(g));
    gp_pack_ptrs(L, pack, g.pk, g.rk);
    g.h0 = h0; g.a = a; g.eps = eps; g.traj = traj; g.vsave = vsave; g.gtraj = gtraj; g.g_ent = g_ent;
    g.gh0 = gh0; g.ga = ga; g.gpart = gpart; g.slab = L->rev_slab;
    g.N = int(N); g.T = int(T); g.M = L->M; g.D = L->D; g.Do = L->Do; g.reverse = reverse ? 1 : 0;
    const int64_t nslots = (N + 15) / 16 * T;
    if (L->rev_stash) {
        g.stash_a = work;
        g.stash_k = work + nslots * L->NBLK * 256;
        hipError_t e = hipMemsetAsync(gB_image, 0, size_t(L->NBLK) * L->NBLK * 256 * sizeof(double), st);
        if (e != hipSuccess) return fail(-int(e) - 1000, "gp_rollout_bwd: clearing the K^-1 adjoint image failed");
    }
    rc = dispatch_gp_roll_bwd(L->NBLK, L->DK, g, st);
    if (rc) return fail(rc, "gp_rollout_bwd launch failed (NBLK=%d DK=%d rc=%d)", L->NBLK, L->DK, rc);
    if (L->rev_stash)
        return cbfssm_stash_contract_f64(L, g.stash_a, g.stash_k, nslots, work + 2 * nslots * L->NBLK * 256, gB_image, stream);
    return 0;
}

}  // extern "C"
