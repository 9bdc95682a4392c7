// Host side of the model adjoint of GPModel.moment_match (cbfssm_gp_mm_pbwd.hpp): argument checks, the sections of `work`,
// and the launches -- alpha and W_d, the per-point pass, the tile-outer pass, the fixed-order sums, X_d = K^-1 Wbar_d, the slab.
#include <hip/hip_runtime.h>
#include <cstring>
#include "../../include/cbfssm_hip.h"
#include "cbfssm_gp_mm_pbwd.hpp"
#include "cbfssm_gp_host.hpp"

namespace cbfssm {

struct PbwdPlan {
    int NB, nwg1, nchunk;
    int64_t pc, p1;
    int64_t alpha, Wd, tq, gq, mt, ps, P1, P2e, P2r, P2a, Wbar, abar, Rbar, glx, scal, ehat, X, total;
};

// the launch geometry and the offsets of the sections of `work` (doubles), from the layout and the number of points
static void pbwd_plan(const cbfssm_pack_layout* L, int64_t npts, PbwdPlan& p)
{
    const int64_t M = L->M, D = L->D, Do = L->Do;
    p.NB = int((M + 15) / 16);
    p.nwg1 = int(npts < PBWD_MAXWG ? npts : PBWD_MAXWG);
    int64_t nch = (PBWD_TILE_TARGET + p.NB * p.NB - 1) / (p.NB * p.NB);
    if (nch > PBWD_MAXCHUNK) nch = PBWD_MAXCHUNK;
    const int64_t byeight = (npts + 7) / 8;
    if (nch > byeight) nch = byeight;
    if (nch < 1) nch = 1;
    p.pc = (npts + nch - 1) / nch;
    if (p.pc < 1) p.pc = 1;
    p.nchunk = int((npts + p.pc - 1) / p.pc);
    if (p.nchunk < 1) p.nchunk = 1;
    p.p1 = M * Do + M * D + D + 4;
    int64_t o = 0;
    auto take = [&o](int64_t n) { const int64_t at = o; o += (n + 7) / 8 * 8; return at; };
    p.alpha = take(M * Do);
    p.Wd = take(Do * M * M);
    p.tq = take(npts * M * D);
    p.gq = take(npts * M);
    p.mt = take(npts * D);
    p.ps = take(npts * 2);
    p.P1 = take(int64_t(p.nwg1) * p.p1);
    p.P2e = take(int64_t(p.nchunk) * (Do + 1) * M * M);
    p.P2r = take(int64_t(p.nchunk) * p.NB * M * D);
    p.P2a = take(int64_t(p.nchunk) * p.NB * M * Do);
    p.Wbar = take((Do + 1) * M * M);
    p.abar = take(M * Do);
    p.Rbar = take(M * D);
    p.glx = take(D);
    p.scal = take(4);
    p.ehat = take(M);
    p.X = take(Do * M * M);
    p.total = o;
}

static int64_t pbwd_slab_total(const cbfssm_pack_layout* L)
{
    return int64_t(2) * L->NBLK * 256 + (L->rev_stash ? 0 : int64_t(L->NBLK) * L->NBLK * 256) + int64_t(L->NBLK) * L->JB * 256 + 192;
}

}  // namespace cbfssm

using namespace cbfssm;

extern "C" {

int64_t cbfssm_gp_moment_match_params_bwd_work_elems(const cbfssm_pack_layout* L, int64_t npts)
{
    if (!gp_layout_ok(L, GP_NEED_ADJOINT) || npts < 0 || npts > (int64_t(1) << 34)) return -1;
    if (L->rev_slab != pbwd_slab_total(L)) return -1;
    PbwdPlan p;
    pbwd_plan(L, npts, p);
    return p.total;
}

int cbfssm_gp_moment_match_params_bwd_f64(const cbfssm_pack_layout* L, const double* pack, const double* cflat,
                                          const double* mean, const double* cov, int64_t npts, const double* gfmean,
                                          const double* gfcov, const double* gxcov, const double* gmean, const double* gcov,
                                          const double* xcov, double* red_slab, double* gB_dense, double* work, void* stream)
{
    if (!L) return fail(-1, "null layout");
    if (!gp_layout_ok(L, GP_NEED_ADJOINT) || L->rev_slab != pbwd_slab_total(L))
        return fail(-3, "gp_moment_match_params_bwd limits: M <= %d, D <= 24, Do <= %d, and a layout of cbfssm_gp_pack_layout with "
                        "its adjoint slab (M=%d D=%d Do=%d)", CBFSSM_MAX_M, CBFSSM_MAX_DOUT, L->M, L->D, L->Do);
    if (npts < 0 || npts > (int64_t(1) << 34)) return fail(-1, "bad npts");
    if (!pack || !cflat || !mean || !gmean || !red_slab || !work) return fail(-1, "null pointer");
    if (!gfmean && !gfcov && !gxcov) return fail(-1, "gp_moment_match_params_bwd: no cotangent");
    if ((cov == nullptr) != (gcov == nullptr)) return fail(-1, "gp_moment_match_params_bwd: gcov goes with cov");
    if (gxcov && !xcov) return fail(-1, "gp_moment_match_params_bwd: a cotangent for xcov needs xcov");
    if ((L->rev_stash != 0) != (gB_dense != nullptr))
        return fail(-1, "gp_moment_match_params_bwd: the dense K^-1 adjoint is required exactly in stash layouts");
    if (npts == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    PbwdPlan p;
    pbwd_plan(L, npts, p);
    const int M = L->M, D = L->D, Do = L->Do;
    GpMmPbwdArgs a;
    memset(&a, 0, sizeof(a));
    a.Kinv = pack + L->Kinv; a.Zs = pack + L->Zs;
    // the constrained flat vector: zeta_pos [M][D] | zeta_mean [M][Do] | zeta_var [M][Do] | variance [1] | lengthscales [D]
    const int64_t o1 = int64_t(M) * D, o2 = o1 + int64_t(M) * Do, o3 = o2 + int64_t(M) * Do;
    a.mu = cflat + o1; a.s2 = cflat + o2; a.var = cflat + o3; a.ls = cflat + o3 + 1;
    a.mean = mean; a.cov = cov; a.gf = gfmean; a.gC = gfcov; a.gX = gxcov; a.gmean = gmean; a.gcov = gcov; a.xcov = xcov;
    a.npts = npts; a.M = M; a.D = D; a.Do = Do; a.NB = p.NB;
    a.alpha = work + p.alpha; a.Wd = work + p.Wd; a.tq = work + p.tq; a.gq = work + p.gq; a.mt = work + p.mt; a.ps = work + p.ps;
    a.P1 = work + p.P1; a.p1 = p.p1; a.nwg1 = p.nwg1;
    a.P2e = work + p.P2e; a.P2r = work + p.P2r; a.P2a = work + p.P2a; a.nchunk = p.nchunk; a.pc = p.pc;
    a.Wbar = work + p.Wbar; a.abar = work + p.abar; a.Rbar = work + p.Rbar; a.glx = work + p.glx; a.scal = work + p.scal;
    a.ehat = work + p.ehat; a.X = work + p.X;
    a.slab = red_slab; a.gB_dense = gB_dense; a.NBLK = L->NBLK; a.JB = L->JB; a.stash = L->rev_stash ? 1 : 0;
    a.slab_total = L->rev_slab;
    const unsigned nb = unsigned(p.NB);
    hipLaunchKernelGGL(gp_mm_pbwd_alpha_kernel, dim3(unsigned((M * Do + 255) / 256)), dim3(256), 0, st, a);
    if (gfcov) hipLaunchKernelGGL(gp_mm_pbwd_gemm_kernel<0>, dim3(nb, nb, unsigned(Do)), dim3(16, 16), 0, st, a);
    if (D <= 8) hipLaunchKernelGGL(gp_mm_pbwd_point_kernel<8>, dim3(unsigned(p.nwg1)), dim3(PBWD_ROWS), 0, st, a);
    else if (D <= 16) hipLaunchKernelGGL(gp_mm_pbwd_point_kernel<16>, dim3(unsigned(p.nwg1)), dim3(PBWD_ROWS), 0, st, a);
    else hipLaunchKernelGGL(gp_mm_pbwd_point_kernel<24>, dim3(unsigned(p.nwg1)), dim3(PBWD_ROWS), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-int(e) - 1000, "gp_moment_match_params_bwd: point pass launch failed");
    if (gfcov) hipLaunchKernelGGL(gp_mm_pbwd_tile_kernel, dim3(nb * nb, unsigned(p.nchunk)), dim3(256), 0, st, a);
    const int64_t nred = int64_t(Do + 1) * M * M + int64_t(M) * Do + int64_t(M) * D + D + 4;
    hipLaunchKernelGGL(gp_mm_pbwd_reduce_kernel, dim3(unsigned((nred + 255) / 256)), dim3(256), 0, st, a);
    if (gfcov) {
        hipLaunchKernelGGL(gp_mm_pbwd_gemm_kernel<1>, dim3(nb, nb, unsigned(Do)), dim3(16, 16), 0, st, a);
        hipLaunchKernelGGL(gp_mm_pbwd_rowsum_kernel, dim3(unsigned(M)), dim3(64), 0, st, a);
    }
    const int64_t nslab = L->rev_slab + (gB_dense ? int64_t(M) * M : 0);
    hipLaunchKernelGGL(gp_mm_pbwd_slab_kernel, dim3(unsigned((nslab + 255) / 256)), dim3(256), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(-int(e) - 1000, "gp_moment_match_params_bwd launch failed");
    return 0;
}

}  // extern "C"
