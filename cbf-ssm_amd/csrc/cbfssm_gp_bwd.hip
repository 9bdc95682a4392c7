// Host side of the batch adjoint of GPModel.predict (cbfssm_gp_bwd.hpp): argument checks, grid, stash contraction.
#include <hip/hip_runtime.h>
#include <cstring>
#include "../../include/cbfssm_hip.h"
#include "cbfssm_gp_host.hpp"

CBF_FOR_EACH_GPBWD_NBLK(CBF_GPBWD_DECLARE)

namespace cbfssm {

static int gp_bwd_maxwg(int NBLK)
{
    switch (NBLK) {
#define X(NB) case NB: return GpBwdCfg<NB>::MAXWG;
        CBF_FOR_EACH_GPBWD_NBLK(X)
#undef X
    }
    return 0;
}

static int dispatch_gp_bwd(int NBLK, int DK, const GpBwdArgs& a, unsigned nwg, hipStream_t st)
{
    switch (NBLK) {
#define X(NB) case NB: return launch_gp_bwd_nb##NB(DK, a, nwg, st);
        CBF_FOR_EACH_GPBWD_NBLK(X)
#undef X
    }
    return -3;
}


}  // namespace cbfssm

using namespace cbfssm;

extern "C" {

int64_t cbfssm_gp_predict_bwd_workgroups(const cbfssm_pack_layout* L, int64_t npts)
{
    if (!gp_layout_ok(L, GP_NEED_ADJOINT) || npts < 0 || npts > (int64_t(1) << 34)) return -1;
    const int64_t nblocks = (npts + 15) / 16, cap = gp_bwd_maxwg(L->NBLK);
    return nblocks < cap ? nblocks : cap;
}

int64_t cbfssm_gp_predict_bwd_work_elems(const cbfssm_pack_layout* L, int64_t npts)
{
    if (!gp_layout_ok(L, GP_NEED_ADJOINT) || npts < 0 || npts > (int64_t(1) << 34)) return -1;
    if (!L->rev_stash) return 0;
    const int64_t nblocks = (npts + 15) / 16;
    return 2 * nblocks * L->NBLK * 256 + cbfssm_stash_contract_work_elems(L, nblocks);
}

int cbfssm_gp_predict_bwd_f64(const cbfssm_pack_layout* L, const double* pack, const double* X, int64_t npts,
                              const double* gmean, const double* gvar, double* gX, double* gpart, double* work,
                              double* gB_image, void* stream)
{
    if (!L) return fail(-1, "null layout");
    if (!gp_layout_ok(L, GP_NEED_ADJOINT))
        return fail(-3, "gp_predict_bwd limits: M <= %d, D <= 24, Do <= %d, and a layout of cbfssm_gp_pack_layout (M=%d D=%d Do=%d)",
                    CBFSSM_MAX_M, CBFSSM_MAX_DOUT, L->M, L->D, L->Do);
    if (npts < 0 || npts > (int64_t(1) << 34)) return fail(-1, "bad npts");
    if (!pack || !X || !gmean || !gvar || !gX || !gpart) return fail(-1, "null pointer");
    if (L->rev_stash && (!work || !gB_image)) return fail(-1, "M=%d (> 112) needs work and gB_image", L->M);
    if (npts == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    GpBwdArgs a;
    memset(&a, 0, sizeof(a));
    gp_pack_ptrs(L, pack, a.pk, a.rk);
    a.X = X; a.gmean = gmean; a.gvar = gvar; a.gX = gX; a.gpart = gpart; a.slab = L->rev_slab;
    a.npts = npts; a.nblocks = (npts + 15) / 16;
    a.M = L->M; a.D = L->D; a.Do = L->Do;
    if (L->rev_stash) {
        a.stash_a = work;
        a.stash_k = work + a.nblocks * L->NBLK * 256;
        hipError_t e = hipMemsetAsync(gB_image, 0, size_t(L->NBLK) * L->NBLK * 256 * sizeof(double), st);
        if (e != hipSuccess) return fail(-int(e) - 1000, "gp_predict_bwd: clearing the K^-1 adjoint image failed");
    }
    const unsigned nwg = unsigned(cbfssm_gp_predict_bwd_workgroups(L, npts));
    int rc = dispatch_gp_bwd(L->NBLK, L->DK, a, nwg, st);
    if (rc) return fail(rc, "gp_predict_bwd launch failed (NBLK=%d DK=%d rc=%d)", L->NBLK, L->DK, rc);
    if (L->rev_stash)
        return cbfssm_stash_contract_f64(L, a.stash_a, a.stash_k, a.nblocks, work + 2 * a.nblocks * L->NBLK * 256, gB_image, stream);
    return 0;
}

}  // extern "C"
