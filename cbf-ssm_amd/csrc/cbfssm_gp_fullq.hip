// Host side of the full-covariance q(z) surface (cbfssm_gp_fullq.hpp): argument checks, the launches of the forward and of
// the adjoint, and the
// small dense steps that run once per call -- S_d = L_d L_d^T with its operand image, W_d = sum_n Fv[n][d] a_n a_n^T from
// the adjoint's A2 images, Lbar_d = tril(2 W_d L_d + klw K^-1 L_d) - klw diag(1 / L_ii), and the KL value.  The dense
// steps are plain library kernels (one output entry per thread, fixed summation order); they are not tuned.
#include <hip/hip_runtime.h>
#include <cstring>
#include "../../include/cbfssm_hip.h"
#include "cbfssm_gp_fullq.hpp"
#include "cbfssm_gp_host.hpp"

CBF_FOR_EACH_GPBWD_NBLK(CBF_GPFQ_DECLARE)

namespace cbfssm {

static int gp_fq_maxwg(int NBLK)
{
    switch (NBLK) {
#define X(NB) case NB: return GpBwdCfg<NB>::MAXWG;
        CBF_FOR_EACH_GPBWD_NBLK(X)
#undef X
    }
    return 0;
}

static int dispatch_gp_fq(int NBLK, int DK, const GpFqArgs& a, unsigned nwg, hipStream_t st)
{
    switch (NBLK) {
#define X(NB) case NB: return launch_gp_fq_nb##NB(DK, a, nwg, st);
        CBF_FOR_EACH_GPBWD_NBLK(X)
#undef X
    }
    return -3;
}

static int dispatch_gp_fq_fwd(int NBLK, int DK, const GpFqFwdArgs& a, unsigned nwg, hipStream_t st)
{
    switch (NBLK) {
#define X(NB) case NB: return launch_gp_fq_fwd_nb##NB(DK, a, nwg, st);
        CBF_FOR_EACH_GPBWD_NBLK(X)
#undef X
    }
    return -3;
}

static bool npts_ok(int64_t npts) { return npts >= 0 && npts <= (int64_t(1) << 34); }

// the q pack: [Do][NBLK][KS][64] operand images of S_d | [Do][M][M] S_d dense | [M][M] sum_d S_d
static int64_t fq_image_elems(const cbfssm_pack_layout* L) { return int64_t(L->Do) * L->NBLK * L->KS * 64; }
static int64_t fq_dense_elems(const cbfssm_pack_layout* L) { return int64_t(L->Do) * L->M * L->M; }

static int fq_slices(int64_t nblocks)
{
    const int64_t s = (nblocks + 15) / 16;
    return int(s < 1 ? 1 : (s > 8 ? 8 : s));
}

// L_d[i][k] of the (Do, M, M) argument: entries above the diagonal are never read
__device__ __forceinline__ double tril_at(const double* q, int M, int i, int k) { return (k <= i) ? q[int64_t(i) * M + k] : 0.0; }

// S_d = L_d L_d^T, dense and as the A-operand image [rb][s][lane]: row 16 rb + (lane & 15), k = 4 s + (lane >> 4)
__global__ __launch_bounds__(256) void fq_s_kernel(const double* q, int M, int NBLK, double* Sp, double* Sd)
{
    __shared__ double As[16][17], Bs[16][17];
    const int tx = threadIdx.x, ty = threadIdx.y, d = blockIdx.z;
    const int i = blockIdx.y * 16 + ty, j = blockIdx.x * 16 + tx;
    const double* qd = q + int64_t(d) * M * M;
    const int kend = 16 * (int(blockIdx.x < blockIdx.y ? blockIdx.x : blockIdx.y) + 1);    // k <= min(i, j)
    double acc = 0.0;
    for (int k0 = 0; k0 < kend && k0 < M; k0 += 16) {
        const int ib = blockIdx.x * 16 + ty;              // rows of L_d behind the columns of this tile
        As[ty][tx] = (i < M && k0 + tx < M) ? tril_at(qd, M, i, k0 + tx) : 0.0;
        Bs[ty][tx] = (ib < M && k0 + tx < M) ? tril_at(qd, M, ib, k0 + tx) : 0.0;
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) acc = fma(As[ty][kk], Bs[tx][kk], acc);
        __syncthreads();
    }
    if (i < M && j < M) {
        Sd[(int64_t(d) * M + i) * M + j] = acc;
        const int KS = 4 * NBLK;
        Sp[((int64_t(d) * NBLK + (i >> 4)) * KS + (j >> 2)) * 64 + 16 * (j & 3) + (i & 15)] = acc;
    }
}

__global__ __launch_bounds__(256) void fq_ssum_kernel(const double* Sd, int M, int Do, double* Ssum)
{
    const int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x, mm = int64_t(M) * M;
    if (idx >= mm) return;
    double s = 0.0;
    for (int d = 0; d < Do; ++d) s += Sd[d * mm + idx];
    Ssum[idx] = s;
}

// One 16 x 16 tile (bi >= bj) of W_d over one slice of the column blocks: sum_n Fv[n][d] A2[i][n] A2[j][n].
// a2img: [column block][NBLK][4][64], C layout: row (lane >> 4) + 4 r, point lane & 15
__global__ __launch_bounds__(256) void fq_wd_kernel(const double* a2img, const double* gvar, int NBLK, int Do, int64_t npts,
                                                    int64_t nblocks, int64_t per, double* part)
{
    __shared__ double Ai[16][17], Aj[16][17];
    const int tid = threadIdx.x, tp = blockIdx.x, d = blockIdx.y, z = blockIdx.z;
    int bi = 0;
    while ((bi + 1) * (bi + 2) / 2 <= tp) ++bi;
    const int bj = tp - bi * (bi + 1) / 2;
    const int r = tid >> 6, l = tid & 63, row = (l >> 4) + 4 * r, n = l & 15;
    const int ty = tid >> 4, tx = tid & 15;
    const int64_t c0 = int64_t(z) * per, c1 = (c0 + per < nblocks) ? c0 + per : nblocks;
    double acc = 0.0;
    for (int64_t cb = c0; cb < c1; ++cb) {
        const int64_t p = cb * 16 + n;
        const double fv = (p < npts) ? gvar[p * Do + d] : 0.0;
        __syncthreads();
        Ai[row][n] = a2img[(cb * NBLK + bi) * 256 + tid] * fv;
        Aj[row][n] = a2img[(cb * NBLK + bj) * 256 + tid];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) acc = fma(Ai[ty][k], Aj[tx][k], acc);
    }
    const int ntp = NBLK * (NBLK + 1) / 2;
    part[((int64_t(z) * Do + d) * ntp + tp) * 256 + tid] = acc;
}

// slices in a fixed order -> dense symmetric W [Do][M][M]; a diagonal tile is taken from its lower half
__global__ __launch_bounds__(256) void fq_wd_reduce_kernel(const double* part, int M, int NBLK, int Do, int ns, double* W)
{
    const int tid = threadIdx.x, tp = blockIdx.x, d = blockIdx.y;
    int bi = 0;
    while ((bi + 1) * (bi + 2) / 2 <= tp) ++bi;
    const int bj = tp - bi * (bi + 1) / 2;
    const int ty = tid >> 4, tx = tid & 15;
    const int ntp = NBLK * (NBLK + 1) / 2;
    double s = 0.0;
    for (int z = 0; z < ns; ++z) s += part[((int64_t(z) * Do + d) * ntp + tp) * 256 + tid];
    const int i = 16 * bi + ty, j = 16 * bj + tx;
    if (i >= M || j >= M) return;
    if (bi == bj && tx > ty) return;
    double* Wd = W + int64_t(d) * M * M;
    Wd[int64_t(i) * M + j] = s;
    if (i != j) Wd[int64_t(j) * M + i] = s;
}

// gq[d] = tril((2 W_d + klw K^-1) L_d) - klw diag(1 / L_d[i][i]); exactly zero above the diagonal.  W or Kinv may be NULL.
__global__ __launch_bounds__(256) void fq_lbar_kernel(const double* q, const double* W, const double* Kinv, double klw, int M,
                                                      double* gq)
{
    __shared__ double As[16][17], Bs[16][17];
    const int tx = threadIdx.x, ty = threadIdx.y, d = blockIdx.z;
    const int i = blockIdx.y * 16 + ty, j = blockIdx.x * 16 + tx;
    const int64_t mm = int64_t(M) * M;
    const double* qd = q + d * mm;
    double acc = 0.0;
    if (blockIdx.x <= blockIdx.y) {
        for (int k0 = 16 * blockIdx.x; k0 < M; k0 += 16) {     // L_d[k][j] = 0 for k < j
            double av = 0.0;
            if (i < M && k0 + tx < M) {
                if (W) av = 2.0 * W[d * mm + int64_t(i) * M + k0 + tx];
                if (Kinv) av = fma(klw, Kinv[int64_t(i) * M + k0 + tx], av);
            }
            As[ty][tx] = av;
            Bs[ty][tx] = (k0 + ty < M && j < M) ? tril_at(qd, M, k0 + ty, j) : 0.0;
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) acc = fma(As[ty][kk], Bs[kk][tx], acc);
            __syncthreads();
        }
    }
    if (i < M && j < M) {
        double v = (j <= i) ? acc : 0.0;
        if (i == j && Kinv) v -= klw / qd[int64_t(i) * M + i];
        gq[d * mm + int64_t(i) * M + j] = v;
    }
}

// KL(q || p) = 0.5 [ sum_ij K^-1_ij (sum_d S_d + sum_d f_d f_d^T)_ij + Do (log det K - M) - sum_d sum_i log L_d[i][i]^2 ]
__global__ __launch_bounds__(256) void fq_kl_kernel(const double* q, const double* Ssum, const double* Kinv, const double* zmean,
                                                    const double* scal, int M, int Do, double* out)
{
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int64_t mm = int64_t(M) * M;
    double acc = 0.0;
    for (int64_t idx = tid; idx < mm; idx += 256) {
        const int i = int(idx / M), j = int(idx - int64_t(i) * M);
        double ff = 0.0;
        for (int d = 0; d < Do; ++d) ff = fma(zmean[i * Do + d], zmean[j * Do + d], ff);
        acc = fma(Kinv[idx], Ssum[idx] + ff, acc);
    }
    for (int idx = tid; idx < M * Do; idx += 256) {
        const int d = idx / M, i = idx - d * M;
        const double lii = q[d * mm + int64_t(i) * M + i];
        acc -= log(lii * lii);
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        const double tot = red[0] + red[1] + red[2] + red[3];
        out[0] = 0.5 * (tot + double(Do) * (scal[CBFSSM_SCAL_LOGDET] - double(M)));
    }
}

static int launched(const char* what)
{
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail(-int(e) - 1000, "%s launch failed", what);
}

}  // namespace cbfssm

using namespace cbfssm;

extern "C" {

int64_t cbfssm_gp_fullq_pack_elems(const cbfssm_pack_layout* L)
{
    if (!gp_layout_ok(L, GP_NEED_ADJOINT)) return -1;
    return fq_image_elems(L) + fq_dense_elems(L) + int64_t(L->M) * L->M;
}

int cbfssm_gp_fullq_prepare_f64(const cbfssm_pack_layout* L, const double* q_sqrt, double* qpack, void* stream)
{
    if (!L) return fail(-1, "null layout");
    if (!gp_layout_ok(L, GP_NEED_ADJOINT))
        return fail(-3, "gp_fullq limits: M <= %d, D <= 24, Do <= %d, and a layout of cbfssm_gp_pack_layout (M=%d D=%d Do=%d)",
                    CBFSSM_MAX_M, CBFSSM_MAX_DOUT, L->M, L->D, L->Do);
    if (!q_sqrt || !qpack) return fail(-1, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    double* Sp = qpack;
    double* Sd = qpack + fq_image_elems(L);
    double* Ssum = Sd + fq_dense_elems(L);
    hipError_t e = hipMemsetAsync(Sp, 0, size_t(fq_image_elems(L)) * sizeof(double), st);     // the zero padding
    if (e != hipSuccess) return fail(-int(e) - 1000, "gp_fullq_prepare: clearing the operand images failed");
    const unsigned nb = unsigned((L->M + 15) / 16);
    hipLaunchKernelGGL(fq_s_kernel, dim3(nb, nb, unsigned(L->Do)), dim3(16, 16), 0, st, q_sqrt, L->M, L->NBLK, Sp, Sd);
    hipLaunchKernelGGL(fq_ssum_kernel, dim3(unsigned((int64_t(L->M) * L->M + 255) / 256)), dim3(256), 0, st, (const double*)Sd,
                       L->M, L->Do, Ssum);
    return launched("gp_fullq_prepare");
}

int cbfssm_gp_fullq_predict_f64(const cbfssm_pack_layout* L, const double* pack, const double* qpack, const double* X,
                                int64_t npts, double* fmean, double* fvar, void* stream)
{
    if (!L) return fail(-1, "null layout");
    if (!gp_layout_ok(L, GP_NEED_ADJOINT))
        return fail(-3, "gp_fullq_predict limits: M <= %d, D <= 24, Do <= %d, and a layout of cbfssm_gp_pack_layout (M=%d D=%d Do=%d)",
                    CBFSSM_MAX_M, CBFSSM_MAX_DOUT, L->M, L->D, L->Do);
    if (!npts_ok(npts)) return fail(-1, "bad npts");
    if (!pack || !qpack || !X || !fmean || !fvar) return fail(-1, "null pointer");
    if (npts == 0) return 0;
    GpFqFwdArgs a;
    memset(&a, 0, sizeof(a));
    gp_pack_ptrs(L, pack, a.pk);
    a.X = X; a.Sp = qpack; a.fmean = fmean; a.fvar = fvar;
    a.npts = npts; a.nblocks = (npts + 15) / 16;
    a.M = L->M; a.D = L->D; a.Do = L->Do; a.tri = (L->gp_form == CBFSSM_GP_FORM_TRI);
    const int64_t cap = 4 * int64_t(gp_fq_maxwg(L->NBLK));       // persistent over the column blocks beyond that
    const unsigned nwg = unsigned(a.nblocks < cap ? a.nblocks : cap);
    int rc = dispatch_gp_fq_fwd(L->NBLK, L->DK, a, nwg, (hipStream_t)stream);
    if (rc) return fail(rc, "gp_fullq_predict launch failed (NBLK=%d DK=%d rc=%d)", L->NBLK, L->DK, rc);
    return 0;
}

int cbfssm_gp_fullq_kl_f64(const cbfssm_pack_layout* L, const double* pack, const double* q_sqrt, const double* qpack,
                           const double* zeta_mean, double* kl, void* stream)
{
    if (!L) return fail(-1, "null layout");
    if (!gp_layout_ok(L, GP_NEED_ADJOINT)) return fail(-3, "gp_fullq limits: M <= %d, D <= 24, Do <= %d", CBFSSM_MAX_M, CBFSSM_MAX_DOUT);
    if (!pack || !q_sqrt || !qpack || !zeta_mean || !kl) return fail(-1, "null pointer");
    const double* Ssum = qpack + fq_image_elems(L) + fq_dense_elems(L);
    hipLaunchKernelGGL(fq_kl_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, q_sqrt, Ssum, pack + L->Kinv, zeta_mean,
                       pack + L->scal, L->M, L->Do, kl);
    return launched("gp_fullq_kl");
}

int64_t cbfssm_gp_fullq_bwd_workgroups(const cbfssm_pack_layout* L, int64_t npts)
{
    if (!gp_layout_ok(L, GP_NEED_ADJOINT) || !npts_ok(npts)) return -1;
    const int64_t nblocks = (npts + 15) / 16, cap = gp_fq_maxwg(L->NBLK);
    return nblocks < cap ? nblocks : cap;
}

int64_t cbfssm_gp_fullq_a2_elems(const cbfssm_pack_layout* L, int64_t npts)
{
    if (!gp_layout_ok(L, GP_NEED_ADJOINT) || !npts_ok(npts)) return -1;
    return (npts + 15) / 16 * L->NBLK * 256;
}

int64_t cbfssm_gp_fullq_bwd_work_elems(const cbfssm_pack_layout* L, int64_t npts)
{
    if (!gp_layout_ok(L, GP_NEED_ADJOINT) || !npts_ok(npts)) return -1;
    if (!L->rev_stash) return 0;
    const int64_t nblocks = (npts + 15) / 16;
    return 2 * nblocks * L->NBLK * 256 + cbfssm_stash_contract_work_elems(L, nblocks);
}

int cbfssm_gp_fullq_bwd_f64(const cbfssm_pack_layout* L, const double* pack, const double* qpack, const double* X, int64_t npts,
                            const double* gmean, const double* gvar, double* gX, double* gpart, double* a2_image, double* work,
                            double* gB_image, void* stream)
{
    if (!L) return fail(-1, "null layout");
    if (!gp_layout_ok(L, GP_NEED_ADJOINT))
        return fail(-3, "gp_fullq_bwd limits: M <= %d, D <= 24, Do <= %d, and a layout of cbfssm_gp_pack_layout (M=%d D=%d Do=%d)",
                    CBFSSM_MAX_M, CBFSSM_MAX_DOUT, L->M, L->D, L->Do);
    if (!npts_ok(npts)) return fail(-1, "bad npts");
    if (!pack || !qpack || !X || !gmean || !gvar || !gX || !gpart || !a2_image) return fail(-1, "null pointer");
    if (L->rev_stash && (!work || !gB_image)) return fail(-1, "M=%d (> 112) needs work and gB_image", L->M);
    if (npts == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    GpFqArgs a;
    memset(&a, 0, sizeof(a));
    gp_pack_ptrs(L, pack, a.pk, a.rk);                              // (the full form reads no sigma_z^2 image)
    a.X = X; a.gmean = gmean; a.gvar = gvar; a.gX = gX; a.gpart = gpart; a.slab = L->rev_slab;
    a.npts = npts; a.nblocks = (npts + 15) / 16;
    a.Sp = qpack; a.a2img = a2_image;
    a.M = L->M; a.D = L->D; a.Do = L->Do;
    if (L->rev_stash) {
        a.stash_a = work;
        a.stash_k = work + a.nblocks * L->NBLK * 256;
        hipError_t e = hipMemsetAsync(gB_image, 0, size_t(L->NBLK) * L->NBLK * 256 * sizeof(double), st);
        if (e != hipSuccess) return fail(-int(e) - 1000, "gp_fullq_bwd: clearing the K^-1 adjoint image failed");
    }
    const unsigned nwg = unsigned(cbfssm_gp_fullq_bwd_workgroups(L, npts));
    int rc = dispatch_gp_fq(L->NBLK, L->DK, a, nwg, st);
    if (rc) return fail(rc, "gp_fullq_bwd launch failed (NBLK=%d DK=%d rc=%d)", L->NBLK, L->DK, rc);
    if (L->rev_stash)
        return cbfssm_stash_contract_f64(L, a.stash_a, a.stash_k, a.nblocks, work + 2 * a.nblocks * L->NBLK * 256, gB_image, stream);
    return 0;
}

int64_t cbfssm_gp_fullq_wd_work_elems(const cbfssm_pack_layout* L, int64_t npts)
{
    if (!gp_layout_ok(L, GP_NEED_ADJOINT) || !npts_ok(npts)) return -1;
    const int64_t ntp = int64_t(L->NBLK) * (L->NBLK + 1) / 2;
    return int64_t(fq_slices((npts + 15) / 16)) * L->Do * ntp * 256;
}

int cbfssm_gp_fullq_wd_f64(const cbfssm_pack_layout* L, const double* a2_image, const double* gvar, int64_t npts, double* work,
                           double* W, void* stream)
{
    if (!L) return fail(-1, "null layout");
    if (!gp_layout_ok(L, GP_NEED_ADJOINT)) return fail(-3, "gp_fullq limits: M <= %d, D <= 24, Do <= %d", CBFSSM_MAX_M, CBFSSM_MAX_DOUT);
    if (!npts_ok(npts)) return fail(-1, "bad npts");
    if (!a2_image || !gvar || !work || !W) return fail(-1, "null pointer");
    if (npts == 0) return 0;
    const int64_t nblocks = (npts + 15) / 16;
    const int ns = fq_slices(nblocks);
    const int64_t per = (nblocks + ns - 1) / ns;
    const unsigned ntp = unsigned(L->NBLK * (L->NBLK + 1) / 2);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(fq_wd_kernel, dim3(ntp, unsigned(L->Do), unsigned(ns)), dim3(256), 0, st, a2_image, gvar, L->NBLK, L->Do,
                       npts, nblocks, per, work);
    hipLaunchKernelGGL(fq_wd_reduce_kernel, dim3(ntp, unsigned(L->Do)), dim3(256), 0, st, (const double*)work, L->M, L->NBLK, L->Do,
                       ns, W);
    return launched("gp_fullq_wd");
}

int cbfssm_gp_fullq_lbar_f64(const cbfssm_pack_layout* L, const double* pack, const double* q_sqrt, const double* W,
                             double kl_weight, double* gq, void* stream)
{
    if (!L) return fail(-1, "null layout");
    if (!gp_layout_ok(L, GP_NEED_ADJOINT)) return fail(-3, "gp_fullq limits: M <= %d, D <= 24, Do <= %d", CBFSSM_MAX_M, CBFSSM_MAX_DOUT);
    if (!q_sqrt || !gq || (!W && !pack)) return fail(-1, "null pointer");
    const unsigned nb = unsigned((L->M + 15) / 16);
    hipLaunchKernelGGL(fq_lbar_kernel, dim3(nb, nb, unsigned(L->Do)), dim3(16, 16), 0, (hipStream_t)stream, q_sqrt, W,
                       pack ? pack + L->Kinv : (const double*)nullptr, kl_weight, L->M, gq);
    return launched("gp_fullq_lbar");
}

}  // extern "C"
