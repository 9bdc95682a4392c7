// What the host files of the GPModel surface (cbfssm_gp_*.hip) share: the layout predicate, the pack pointers of a launch
// and the declarations of the functions and pre-kernels that one of them defines and others use.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/cbfssm_hip.h"
#include "cbfssm_gp_bwd.hpp"

namespace cbfssm {

int fail(int rc, const char* fmt, ...);   // cbfssm_api.hip

// cbfssm_gp_lin.hip: alpha = K^-1 mu as [16][16 NBLK], in the order the GP form asks for
__global__ void gp_lin_alpha_kernel(const double* Kinv, const double* G, const double* muB, int M, int Do, int MP, int tri,
                                    double* alpha);
// cbfssm_gp_mm.hip: the tiles of W_d = K^-1 - K^-1 diag(zeta_var[:, d]) K^-1
__global__ void gp_mm_w_kernel(const double* Kinv, const double* s2B, int M, int NBLK, double* Wimg);
// cbfssm_gp_ekf.hip: the size checks and the launch of cbfssm_gp_ekf_f64 (also behind GPModel.eks and GPModel.adf)
int gp_ekf_check_sizes(const char* who, const cbfssm_pack_layout* L, int Dy, int64_t N, int64_t T);
int gp_ekf_launch(const char* who, const cbfssm_pack_layout* L, const double* pack, const double* m0, const double* P0,
                  const double* a, const double* y, const double* cond, const double* var_x, const double* var_y, int Dy,
                  int64_t N, int64_t T, double* means, double* covs, double* loglik, double* pmeans, double* pcovs,
                  double* cross, double* work, hipStream_t st);
// cbfssm_gp_eks.hip: the two smoother launches behind a forward pass that left means, covs, pmeans, pcovs and cross
int gp_eks_sweep_launch(const char* who, const double* m0, const double* P0, const double* means, const double* covs,
                        const double* pmeans, const double* pcovs, const double* cross, double* smeans, double* scovs,
                        double* sm_init, double* sP_init, double* lag1, double* info, int64_t N, int64_t T, int Do,
                        hipStream_t st);

// what an entry point needs of a layout beyond the geometry
enum : unsigned {
    GP_NEED_ADJOINT = 1,   // the slab and stash fields of the adjoints: rev_slab > 0, rev_stash exactly above seven row blocks
    GP_NEED_FORM = 2,      // gp_form is dense or two-triangular
    GP_NEED_STATE = 4,     // Do <= D: the outputs are the leading inputs (the time loops)
};

// The limits of cbfssm_gp_predict_f64, checked on the layout itself (a layout need not come from cbfssm_gp_pack_layout): the
// geometry every GP surface kernel relies on -- a compiled tile height that covers M, KS = 4 NBLK k-steps per operand
// image, DK and JB as the kernels derive them -- and the parts in `need`.
inline bool gp_layout_ok(const cbfssm_pack_layout* L, unsigned need = 0)
{
    if (!L) return false;
    if (L->M < 1 || L->M > CBFSSM_MAX_M || L->D < 1 || L->D > 24 || L->Do < 1 || L->Do > CBFSSM_MAX_DOUT) return false;
    bool nb = false;
#define X(NB) nb = nb || (L->NBLK == NB);
    CBF_FOR_EACH_GPBWD_NBLK(X)
#undef X
    if (!nb || 16 * L->NBLK < L->M || L->KS != 4 * L->NBLK) return false;
    if ((L->DK != 2 && L->DK != 4 && L->DK != 6) || 4 * L->DK < L->D) return false;
    if (L->JB != (4 * L->DK + 1 + 15) / 16) return false;
    if ((need & GP_NEED_ADJOINT) && (L->rev_slab <= 0 || (L->rev_stash != 0) != (L->NBLK > 7))) return false;
    if ((need & GP_NEED_FORM) && L->gp_form != CBFSSM_GP_FORM_DENSE && L->gp_form != CBFSSM_GP_FORM_TRI) return false;
    if ((need & GP_NEED_STATE) && L->Do > L->D) return false;
    return true;
}

// the sections of a pack as the kernels' operand pointers
inline void gp_pack_ptrs(const cbfssm_pack_layout* L, const double* pack, PackPtrs& pk)
{
    pk.Bp = pack + L->Bp; pk.Zp = pack + L->Zp; pk.cz = pack + L->cz; pk.muA = pack + L->muA; pk.s2A = pack + L->s2A;
    pk.invl = pack + L->invl; pk.scal = pack + L->scal; pk.KSr = (L->M + 3) / 4;
    pk.Wp = pack + L->Wp; pk.WTp = pack + L->WTp;
}
inline void gp_pack_ptrs(const cbfssm_pack_layout* L, const double* pack, PackPtrs& pk, RevPackPtrs& rk)
{
    gp_pack_ptrs(L, pack, pk);
    rk.muB = pack + L->muB; rk.s2B = pack + L->s2B; rk.ZT = pack + L->ZT;
}

}  // namespace cbfssm
