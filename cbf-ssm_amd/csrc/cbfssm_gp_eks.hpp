// Rauch-Tung-Striebel smoother behind the extended Kalman filter of cbfssm_gp_ekf.hpp (GPModel.eks).  gp_ekf_kernel, in its
// EMIT form, leaves per step t and chain n
//
//   pmeans[t] = m-_t,   pcovs[t] = P-_t = A_t P_{t-1} A_t^T + diag(fv + var_x),   cross[t] = A_t P_{t-1}   (P_{-1} = P0)
//
// and the smoother is, for t = T-1 .. 0 from (ms_{T-1}, Ps_{T-1}) = (means[T-1], covs[T-1]),
//
//   G_t      = cross[t]^T (P-_t)^-1                 Cholesky factor of P-_t, two triangular solves per column of cross[t]
//   ms_{t-1} = m_{t-1} + G_t (ms_t - m-_t)
//   Ps_{t-1} = P_{t-1} + G_t (Ps_t - P-_t) G_t^T    lower triangle computed, mirrored: bitwise symmetric
//   lag1[t]  = G_t Ps_t                             Cov(x_{t-1}, x_t | all y), when asked for
//
// with (m_{t-1}, P_{t-1}) the filtered moments, (m0, P0) at t = 0: the last iteration gives the smoothed initial belief.
//
// Two kernels.  The gains do not depend on the recursion, and a factorisation is a chain of 16 dependent pivots (a square
// root, a reciprocal and an LDS round trip each): inside the time loop it set the pace (DESIGN.md 3.2i has both forms
// measured).  So gp_eks_gain_kernel forms every G_t in parallel over (t, n), and gp_eks_sweep_kernel, serial in time and
// parallel over chains, is left with three small products per step.  G_t and the flag of its factorisation travel in the
// output slots of time t - 1 -- scovs[t-1] and smeans[t-1][0]; sP_init and sm_init[0] at t = 0 -- which the sweep reads
// before it writes Ps_{t-1} and ms_{t-1} there: no buffer beyond the outputs, and every output entry is still written.
//
// Lanes as in the covariance part of gp_ekf_kernel, in both kernels: one lane per (chain, row i), 16 lanes side by side are
// one chain, so a chain never leaves its wave and wave barriers are all that is needed.  One wave per workgroup, four
// chains per wave.  [16][17] tiles in LDS per chain: the factor of P-_t in the gain kernel (strictly lower part; the
// reciprocal roots of the pivots are in registers); G_t, Ps_t - P-_t and Ps_t (bitwise symmetric) in the sweep.  Row i of
// G_t is the solution of P-_t g = cross[t][:, i]: every lane solves its own right-hand side in registers against the
// factor in LDS, with no exchange between lanes.  The sweep issues the stores of step t+1 and the loads of step t-1 before
// the work of step t.
//
// A pivot <= 0 or not finite at step t sets info[n] = t + 1 (the first one met going backward, i.e. the largest t) and turns
// the chain's later results -- times < t, the initial belief, lag1[<= t] -- into NaN; nothing traps.  No atomics, no spin
// wait: every output entry has one last writer and two calls are bitwise identical.  VALU, not MFMA: DESIGN.md 3.2i.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace cbfssm {

struct GpEksArgs {
    const double* m0;      // (N, Do)
    const double* P0;      // (N, Do, Do), lower triangle read, or null: zero
    const double* means;   // (T, N, Do)       filtered
    const double* covs;    // (T, N, Do, Do)
    const double* pmeans;  // (T, N, Do)       predicted
    const double* pcovs;   // (T, N, Do, Do)
    const double* cross;   // (T, N, Do, Do)   A_t P_{t-1}
    double* smeans;        // (T, N, Do)
    double* scovs;         // (T, N, Do, Do)
    double* sm_init;       // (N, Do)
    double* sP_init;       // (N, Do, Do)
    double* lag1;          // (T, N, Do, Do) or null
    double* info;          // (N)  0, or t + 1 of the failed factorisation
    int N, T, Do;
};

constexpr int EKS_CHAINS = 4;                           // per wave = per workgroup
constexpr int EKS_PD = 17;
constexpr int EKS_TILE = 16 * EKS_PD;

// the 16 lanes of a chain exchange data through LDS: in program order within the wave
__device__ __forceinline__ void eks_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// row i of a (Do, Do) matrix into 16 registers, zero padded; upto: entries q <= upto only (the lower triangle of P0)
__device__ __forceinline__ void eks_load_row(const double* src, bool on, int Do, int upto, double (&v)[16])
{
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = (on && q < Do && q <= upto) ? src[q] : 0.0;
}

// where G_t and the flag of its factorisation wait for the sweep: the output slots of time t - 1
__device__ __forceinline__ double* eks_gain_slot(const GpEksArgs& a, int t, int nc)
{
    const int64_t DD = int64_t(a.Do) * a.Do;
    return t > 0 ? a.scovs + (int64_t(t - 1) * a.N + nc) * DD : a.sP_init + int64_t(nc) * DD;
}
__device__ __forceinline__ double* eks_flag_slot(const GpEksArgs& a, int t, int nc)
{
    return t > 0 ? a.smeans + (int64_t(t - 1) * a.N + nc) * a.Do : a.sm_init + int64_t(nc) * a.Do;
}

// ---- G_t for every (t, n): grid (ceil(N / 4), min(T, 65535))
__global__ __launch_bounds__(64) void gp_eks_gain_kernel(GpEksArgs a)
{
    constexpr int PD = EKS_PD;
    __shared__ double lds[EKS_CHAINS * EKS_TILE];
    const int l = threadIdx.x, cl = l >> 4, i = l & 15;
    const int N = a.N, T = a.T, Do = a.Do;
    const int n = blockIdx.x * EKS_CHAINS + cl;
    const int nc = min(n, N - 1);                       // chains >= N repeat chain N - 1 and store nothing
    const bool act = i < Do, st = act && (n < N);
    const int ic = act ? i : 0;
    double* Lt = lds + cl * EKS_TILE;

#pragma unroll 1
    for (int t = blockIdx.y; t < T; t += gridDim.y) {
        const int64_t ot = (int64_t(t) * N + nc) * Do;
        double r[16], x[16];                            // row i of P-_t; column i of cross[t], the right-hand side of row i of G_t
        eks_load_row(a.pcovs + (ot + ic) * Do, act, Do, 16, r);
#pragma unroll
        for (int q = 0; q < 16; ++q) x[q] = (act && q < Do) ? a.cross[(ot + q) * Do + ic] : 0.0;
        eks_wave_sync();                                // the previous t's readers of Lt are done

        // P-_t = L L^T, right looking: at step j lane i holds what is left of row i; column j of L goes through Lt
        double rd[16];                                  // 1 / L[j][j]
        bool bad = false;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            rd[j] = 1.0;
            if (j < Do) {
                const double piv = __shfl(r[j], j, 16);
                bad = bad || !(piv > 0.0) || !(piv < __builtin_inf());
                rd[j] = 1.0 / sqrt(piv);
                const double lij = r[j] * rd[j];
                Lt[i * PD + j] = lij;
                eks_wave_sync();
#pragma unroll
                for (int k = j + 1; k < 16; ++k) r[k] = fma(-lij, Lt[k * PD + j], r[k]);
            }
        }
        // L z = x, then L^T g = z, in registers: x becomes row i of G_t
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (j < Do) {
                x[j] *= rd[j];
#pragma unroll
                for (int k = j + 1; k < 16; ++k) x[k] = fma(-x[j], Lt[k * PD + j], x[k]);
            }
        }
#pragma unroll
        for (int j = 15; j >= 0; --j) {
            if (j < Do) {
                x[j] *= rd[j];
#pragma unroll
                for (int k = 0; k < j; ++k) x[k] = fma(-x[j], Lt[j * PD + k], x[k]);
            }
        }
        if (st) {
            double* g = eks_gain_slot(a, t, nc) + int64_t(i) * Do;
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if (q < Do) g[q] = x[q];
            if (i == 0) eks_flag_slot(a, t, nc)[0] = bad ? 1.0 : 0.0;
        }
    }
}

// ---- the sweep: grid ceil(N / 4)
__global__ __launch_bounds__(64) void gp_eks_sweep_kernel(GpEksArgs a)
{
    constexpr int PD = EKS_PD;
    __shared__ double lds[EKS_CHAINS * (3 * EKS_TILE + 16)];
    const int l = threadIdx.x, cl = l >> 4, i = l & 15;
    const int N = a.N, T = a.T, Do = a.Do;
    const int n = blockIdx.x * EKS_CHAINS + cl;
    const int nc = min(n, N - 1);                       // chains >= N repeat chain N - 1 and store nothing
    const bool act = i < Do, st = act && (n < N);
    const int ic = act ? i : 0;
    double* Dt = lds + cl * (3 * EKS_TILE + 16);        // Ps_t - P-_t
    double* Gt = Dt + EKS_TILE;                         // G_t
    double* Pst = Gt + EKS_TILE;                        // Ps_t
    double* dv = Pst + EKS_TILE;                        // [16]  ms_t - m-_t
    const double nan = __builtin_nan("");
    const int64_t DD = int64_t(Do) * Do;

    // the operands of a step: G_t and its flag, P-_t by rows, m-_t, the filtered moments of t - 1
    double x[16], r[16], pf[16], pm, mf, fl;
    auto fetch = [&](int t, double (&x_)[16], double (&r_)[16], double (&pf_)[16], double& pm_, double& mf_, double& fl_) {
        const int64_t ot = (int64_t(t) * N + nc) * Do + ic;
        eks_load_row(eks_gain_slot(a, t, nc) + int64_t(ic) * Do, act, Do, 16, x_);
        fl_ = eks_flag_slot(a, t, nc)[0];
        eks_load_row(a.pcovs + ot * Do, act, Do, 16, r_);
        pm_ = act ? a.pmeans[ot] : 0.0;
        if (t > 0) {
            const int64_t op = ot - int64_t(N) * Do;
            eks_load_row(a.covs + op * Do, act, Do, 16, pf_);
            mf_ = act ? a.means[op] : 0.0;
        } else {
            const int64_t op = int64_t(nc) * Do + ic;
            eks_load_row(a.P0 ? a.P0 + op * Do : a.m0, act && a.P0, Do, ic, pf_);
            mf_ = act ? a.m0[op] : 0.0;
        }
    };
    fetch(T - 1, x, r, pf, pm, mf, fl);
    double ms;
    // (ms_{t-1}, Ps_{t-1}) of step t into the slots of time t - 1, or the initial belief; Pst is whole (a wave sync precedes)
    auto store = [&](int t) {
        if (st) {
            double* sm = eks_flag_slot(a, t, nc);
            double* sc = eks_gain_slot(a, t, nc);
            sm[i] = ms;
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if (q < Do) sc[int64_t(i) * Do + q] = Pst[i * PD + q];
        }
    };

    // ---- the last filtered belief is the last smoothed one, bitwise
    const int64_t o = (int64_t(T - 1) * N + nc) * Do + ic;
    ms = act ? a.means[o] : 0.0;
    {
        double ps[16];
        eks_load_row(a.covs + o * Do, act, Do, 16, ps);
#pragma unroll
        for (int q = 0; q < 16; ++q) Pst[i * PD + q] = ps[q];
        if (st) {
            a.smeans[o] = ms;
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if (q < Do) a.scovs[o * Do + q] = ps[q];
        }
    }
    int failed = 0;                                     // t + 1 of the first failed factorisation met (chain uniform)

#pragma unroll 1
    for (int t = T - 1; t >= 0; --t) {
        // the previous step's results (time t, over G_{t+1} and its flag, which every lane has read) and the next step's
        // operands (their slots are written two steps from here): stores and loads in flight under this step's work, so
        // that the wait at the end of the step is for traffic that has had the whole step
        if (t < T - 1) store(t + 1);
        double xn[16], rn[16], pfn[16], pmn = 0.0, mfn = 0.0, fln = 0.0;
        if (t > 0) fetch(t - 1, xn, rn, pfn, pmn, mfn, fln);
        if (fl != 0.0 && !failed) failed = t + 1;

        eks_wave_sync();                                // the previous step's readers of Gt and Dt are done; Pst is whole
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            Gt[i * PD + q] = x[q];
            Dt[i * PD + q] = Pst[i * PD + q] - r[q];    // bitwise symmetric, as both are
        }
        dv[i] = ms - pm;
        eks_wave_sync();

        // ---- ms_{t-1}, row i of E = G (Ps_t - P-_t) and of lag1[t] = G Ps_t
        double msn = 0.0, e[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) e[q] = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (k < Do) {
                msn = fma(x[k], dv[k], msn);
                const double* dk = Dt + k * PD;
#pragma unroll
                for (int q = 0; q < 16; ++q) e[q] = fma(x[k], dk[q], e[q]);
            }
        }
        msn = mf + msn;
        if (a.lag1) {
            double g1[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) g1[q] = 0.0;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                if (k < Do) {
                    const double* pk = Pst + k * PD;
#pragma unroll
                    for (int q = 0; q < 16; ++q) g1[q] = fma(x[k], pk[q], g1[q]);
                }
            }
            if (st) {
                double* lg = a.lag1 + (int64_t(t) * N + nc) * DD + int64_t(i) * Do;
#pragma unroll
                for (int q = 0; q < 16; ++q)
                    if (q < Do) lg[q] = failed ? nan : g1[q];
            }
        }
        eks_wave_sync();                                // the chain has read Ps_t before one of its lanes writes Ps_{t-1}

        // ---- Ps_{t-1} = P_{t-1} + E G^T: the lower triangle, mirrored
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (j <= i && act) {
                const double* gj = Gt + j * PD;
                double p = 0.0;
#pragma unroll
                for (int q = 0; q < 16; ++q) p = fma(e[q], gj[q], p);
                p = failed ? nan : pf[j] + p;
                Pst[i * PD + j] = p;
                Pst[j * PD + i] = p;
            }
        }
        ms = failed ? nan : msn;
        eks_wave_sync();

        if (t > 0) {
            // the wait for this step's loads belongs HERE, where they and the stores ahead of them have had the whole
            // step, not behind the next step's stores (an empty statement that takes the values pins it)
#pragma unroll
            for (int q = 0; q < 16; ++q) asm volatile("" : "+v"(xn[q]), "+v"(rn[q]), "+v"(pfn[q]));
            asm volatile("" : "+v"(pmn), "+v"(mfn), "+v"(fln));
#pragma unroll
            for (int q = 0; q < 16; ++q) { x[q] = xn[q]; r[q] = rn[q]; pf[q] = pfn[q]; }
            pm = pmn;
            mf = mfn;
            fl = fln;
        }
    }
    store(0);
    if (i == 0 && n < N) a.info[nc] = double(failed);
}

}  // namespace cbfssm
