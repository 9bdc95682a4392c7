// Voliro's forward filter run (cbfssm/model/voliro.py:188-242,314-338) and its adjoint, one launch each.
//
//   q = var_x, r = var_y,  k = q / (q + r),  sig = (1-k)^2 q + k^2 r                     (loop invariant)
//   for t = 0 .. S-1:   f = symplectic_euler(x, u[t]);  mu = f + k (y[t] - f);  x = mu + eps[t] sqrt(sig);  traj[t] = x
//                       kl += 0.5 sum_d (log q - log sig + (sig + (mu - f)^2) / q - 1)
//
// The work is serial in t and tiny per chain (13 doubles of state), so the shape is one lane per chain with the state --
// and, in the reverse sweep, the adjoint carry and the per-chain sums of the variance adjoints -- in registers, 64 chains
// (one wave) per workgroup, no LDS and no barrier.  The rows of the next step are loaded before the arithmetic of the
// current one.  Rows are read and written in place, 13 (or 6) consecutive doubles per lane: a wave covers one contiguous
// 6.6 KB (3 KB) stretch per tensor and step and uses every byte of every cache line it touches, so staging through LDS
// would save address cycles only, at the price of a wait per step on the serial path.
// The reverse sweep recomputes f of every step from traj[t-1] (x0 at t = 0) and u[t]; nothing else is kept.
// No atomics: every output has one writer, the partial sums leave through a fixed-order wave reduction, one slab per
// workgroup, and cbfssm_reduce_partials_f64 adds the slabs in a fixed order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cbfssm_rigid_filter.hpp"

namespace cbfssm {

int fail(int rc, const char* fmt, ...);   // cbfssm_api.hip

static const int64_t kRfMaxChains = int64_t(1) << 30;    // as the rollout
static const int64_t kRfMaxSteps = int64_t(1) << 24;

// sum over the 64 lanes in a fixed order; every lane must call it; lane 0 holds the result
__device__ __forceinline__ double rf_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

template <int W>
__device__ __forceinline__ void rf_load(double* dst, const double* src)
{
#pragma unroll
    for (int i = 0; i < W; ++i) dst[i] = src[i];
}

__global__ __launch_bounds__(RF_WG) void rigid_filter_kernel(cbfssm_rigid_body rb, const double* __restrict__ x0,
                                                             const double* __restrict__ u, const double* __restrict__ y,
                                                             const double* __restrict__ eps,
                                                             const double* __restrict__ var_x,
                                                             const double* __restrict__ var_y, int64_t N, int64_t S,
                                                             double* __restrict__ traj, double* __restrict__ kl_part)
{
    const int64_t n = int64_t(blockIdx.x) * RF_WG + threadIdx.x;
    double kl = 0.0;
    if (n < N) {
        double gk[RF_DX], gs[RF_DX], gc[RF_DX];
        double kl0 = 0.0;
#pragma unroll
        for (int d = 0; d < RF_DX; ++d) {
            const RfGain g = rf_gain(var_x[d], var_y[d]);
            gk[d] = g.k; gs[d] = g.s; gc[d] = g.c;
            kl0 += g.kl0;
        }
        double x[RF_DX], uc[RF_DU], yc[RF_DX], un[RF_DU] = {}, yn[RF_DX] = {}, f[RF_DX];
        double ec, en = 0.0;
        rf_load<RF_DX>(x, x0 + n * RF_DX);
        rf_load<RF_DU>(uc, u + n * RF_DU);
        rf_load<RF_DX>(yc, y + n * RF_DX);
        ec = eps[n];
        double acc = 0.0;
        for (int64_t t = 0; t < S; ++t) {
            if (t + 1 < S) {                                  // the next step's rows, ahead of this step's arithmetic
                const int64_t row = (t + 1) * N + n;
                rf_load<RF_DU>(un, u + row * RF_DU);
                rf_load<RF_DX>(yn, y + row * RF_DX);
                en = eps[row];
            }
            rf_step(rb, x, uc, f, nullptr);
            double* out = traj + (t * N + n) * RF_DX;
#pragma unroll
            for (int d = 0; d < RF_DX; ++d) {
                const double df = yc[d] - f[d];
                x[d] = f[d] + gk[d] * df + ec * gs[d];
                out[d] = x[d];
                acc += gc[d] * (df * df);
            }
#pragma unroll
            for (int d = 0; d < RF_DU; ++d) uc[d] = un[d];
#pragma unroll
            for (int d = 0; d < RF_DX; ++d) yc[d] = yn[d];
            ec = en;
        }
        kl = 0.5 * acc + double(S) * kl0;
    }
    kl = rf_wave_sum(kl);                                     // lanes beyond N add exactly zero
    if (threadIdx.x == 0) kl_part[blockIdx.x] = kl;
}

__global__ __launch_bounds__(RF_WG) void rigid_filter_bwd_kernel(cbfssm_rigid_body rb, const double* __restrict__ x0,
                                                                 const double* __restrict__ u,
                                                                 const double* __restrict__ y,
                                                                 const double* __restrict__ eps,
                                                                 const double* __restrict__ var_x,
                                                                 const double* __restrict__ var_y,
                                                                 const double* __restrict__ traj,
                                                                 const double* __restrict__ gtraj,
                                                                 const double* __restrict__ g_kl, int64_t N, int64_t S,
                                                                 double* __restrict__ gx0, double* __restrict__ gu,
                                                                 double* __restrict__ gy, double* __restrict__ gpart)
{
    const int64_t n = int64_t(blockIdx.x) * RF_WG + threadIdx.x;
    double gq[RF_DX], gr[RF_DX];
#pragma unroll
    for (int d = 0; d < RF_DX; ++d) gq[d] = gr[d] = 0.0;
    if (n < N) {
        const double gkl = g_kl[0];
        double kk[RF_DX], kc[RF_DX];
#pragma unroll
        for (int d = 0; d < RF_DX; ++d) {
            const RfGain g = rf_gain(var_x[d], var_y[d]);
            kk[d] = g.k; kc[d] = g.c * gkl;
        }
        double A[RF_DX], Bn[RF_DX], Cn[RF_DX], carry[RF_DX];
#pragma unroll
        for (int d = 0; d < RF_DX; ++d) A[d] = Bn[d] = Cn[d] = carry[d] = 0.0;
        double xp[RF_DX], uc[RF_DU], yc[RF_DX], gt[RF_DX], ec;
        double xpn[RF_DX] = {}, un[RF_DU] = {}, yn[RF_DX] = {}, gtn[RF_DX] = {}, en = 0.0;
        {
            const int64_t row = (S - 1) * N + n;
            rf_load<RF_DX>(xp, S > 1 ? traj + (row - N) * RF_DX : x0 + n * RF_DX);
            rf_load<RF_DU>(uc, u + row * RF_DU);
            rf_load<RF_DX>(yc, y + row * RF_DX);
            rf_load<RF_DX>(gt, gtraj + row * RF_DX);
            ec = eps[row];
        }
        for (int64_t t = S - 1; t >= 0; --t) {
            if (t > 0) {                                      // the rows of step t-1, ahead of this step's arithmetic
                const int64_t row = (t - 1) * N + n;
                rf_load<RF_DX>(xpn, t > 1 ? traj + (row - N) * RF_DX : x0 + n * RF_DX);
                rf_load<RF_DU>(un, u + row * RF_DU);
                rf_load<RF_DX>(yn, y + row * RF_DX);
                rf_load<RF_DX>(gtn, gtraj + row * RF_DX);
                en = eps[row];
            }
            double f[RF_DX], gf[RF_DX], inv_n;
            rf_step(rb, xp, uc, f, &inv_n);
            double* gyo = gy + (t * N + n) * RF_DX;
#pragma unroll
            for (int d = 0; d < RF_DX; ++d) {
                const double gx = gt[d] + carry[d];
                const double df = yc[d] - f[d];
                const double gdf = kk[d] * gx + kc[d] * df;   // d loss / d (y - f)
                gyo[d] = gdf;
                gf[d] = gx - gdf;
                A[d] += gx * df;
                Bn[d] += gx * ec;
                Cn[d] += df * df;
            }
            double guo[RF_DU];
            rf_step_bwd(rb, xp, uc, f, inv_n, gf, carry, guo);
            double* gup = gu + (t * N + n) * RF_DU;
#pragma unroll
            for (int d = 0; d < RF_DU; ++d) gup[d] = guo[d];
#pragma unroll
            for (int d = 0; d < RF_DX; ++d) { xp[d] = xpn[d]; yc[d] = yn[d]; gt[d] = gtn[d]; }
#pragma unroll
            for (int d = 0; d < RF_DU; ++d) uc[d] = un[d];
            ec = en;
        }
        double* g0 = gx0 + n * RF_DX;
#pragma unroll
        for (int d = 0; d < RF_DX; ++d) g0[d] = carry[d];
#pragma unroll
        for (int d = 0; d < RF_DX; ++d)
            rf_gain_bwd(var_x[d], var_y[d], A[d], Bn[d], gkl * Cn[d], gkl * double(S), &gq[d], &gr[d]);
    }
    double* slab = gpart + int64_t(blockIdx.x) * RF_SLAB;     // lanes beyond N add exactly zero
#pragma unroll
    for (int d = 0; d < RF_DX; ++d) {
        const double a = rf_wave_sum(gq[d]);
        const double b = rf_wave_sum(gr[d]);
        if (threadIdx.x == 0) { slab[d] = a; slab[RF_DX + d] = b; }
    }
    if (threadIdx.x < RF_SLAB - 2 * RF_DX) slab[2 * RF_DX + threadIdx.x] = 0.0;
}

static int rf_check(int64_t N, int64_t S, const char* who)
{
    if (N < 0 || S < 1) return fail(-1, "%s: N=%lld must be >= 0 and S=%lld >= 1", who, (long long)N, (long long)S);
    if (N > kRfMaxChains || S > kRfMaxSteps) return fail(-3, "%s: N <= 2^30 chains, S <= 2^24 steps", who);
    return 0;
}

static int rf_launched(const char* who)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-int(e) - 1000, "%s launch failed: %s", who, hipGetErrorString(e));
    return 0;
}

}  // namespace cbfssm

using namespace cbfssm;

extern "C" {

int64_t cbfssm_rigid_filter_partials(int64_t N)
{
    if (N < 0 || N > kRfMaxChains) return -1;
    return (N + RF_WG - 1) / RF_WG;
}

int cbfssm_rigid_filter_f64(const cbfssm_rigid_body* body, const double* x0, const double* u, const double* y,
                            const double* eps, const double* var_x, const double* var_y, int64_t N, int64_t S,
                            double* traj, double* kl_part, void* stream)
{
    int rc = rf_check(N, S, "rigid_filter");
    if (rc) return rc;
    if (!body || !x0 || !u || !y || !eps || !var_x || !var_y || !traj || !kl_part)
        return fail(-1, "rigid_filter: null pointer");
    if (N == 0) return 0;
    const unsigned nwg = unsigned((N + RF_WG - 1) / RF_WG);
    hipLaunchKernelGGL(rigid_filter_kernel, dim3(nwg), dim3(RF_WG), 0, (hipStream_t)stream, *body, x0, u, y, eps, var_x,
                       var_y, N, S, traj, kl_part);
    return rf_launched("rigid_filter");
}

int cbfssm_rigid_filter_bwd_f64(const cbfssm_rigid_body* body, const double* x0, const double* u, const double* y,
                                const double* eps, const double* var_x, const double* var_y, const double* traj,
                                const double* gtraj, const double* g_kl, int64_t N, int64_t S, double* gx0, double* gu,
                                double* gy, double* gpart, void* stream)
{
    int rc = rf_check(N, S, "rigid_filter_bwd");
    if (rc) return rc;
    if (!body || !x0 || !u || !y || !eps || !var_x || !var_y || !traj || !gtraj || !g_kl || !gx0 || !gu || !gy || !gpart)
        return fail(-1, "rigid_filter_bwd: null pointer");
    if (N == 0) return 0;
    const unsigned nwg = unsigned((N + RF_WG - 1) / RF_WG);
    hipLaunchKernelGGL(rigid_filter_bwd_kernel, dim3(nwg), dim3(RF_WG), 0, (hipStream_t)stream, *body, x0, u, y, eps,
                       var_x, var_y, traj, gtraj, g_kl, N, S, gx0, gu, gy, gpart);
    return rf_launched("rigid_filter_bwd");
}

}  // extern "C"
