// The adjoint of GPModel.moment_match with respect to the MODEL: what the five leaves receive through
// alpha = K^-1 mu, W_d = K^-1 - K^-1 diag(s2_d) K^-1, Z~, the lengthscales and the variance, delivered as ONE reduced slab in
// the Slab<NBLK,JB,STASH> layout of cbfssm_adjoint.hpp (sections gMu, gS2, gB, gZ; small: glx, gsig, glogsig) plus, above
// seven row blocks, the dense row-major K^-1 adjoint -- cbfssm_gp_tail_f64 (kl_weight 0) does the rest, unchanged.
//
// Notation of 3.2k / 3.2m.  Per point n (A = I + S~ = L1 L1^T, B = I/2 + S~ = L2 L2^T, r_i = z~_i - m~):
//
//     a1_i = A^-1 r_i,  t_i = B^-1 r_i,  g_i = r_i . t_i,  q_i = v det(A)^-1/2 exp(-r_i . a1_i / 2)
//     Q_ij = c2 exp(-|z~_i - z~_j|^2 / 4 - (g_i + g_j + 2 r_i . t_j) / 8)        (u_i . u_j = r_i . t_j: no u is kept)
//     Gs = (gC + gC^T) / 2,  fbar = gf - 2 Gs fmean,  Hbar = A^-1 S~ diag(l) gX^T
//     Qbar_ij = alpha_i . (Gs alpha_j) - sum_d gC_dd W_d,ij,   E = Qbar o Q
//     qbar_i = alpha_i . fbar + r_i^T Hbar alpha_i,  ebar_i = qbar_i q_i
//
// and summed over the points
//
//     abar_i  = sum_n [ q_i (fbar + Hbar^T r_i) + 2 sum_j Q_ij Gs alpha_j ]
//     Wbar_d  = - sum_n gC_dd Q,     Ehat = sum_n E
//     Rbar_i  = sum_n [ q_i Hbar alpha_i - ebar_i a1_i - sum_j E_ij (t_i + t_j) / 2 ]
//     glogsig = sum_n [ sum_i ebar_i + 2 sum_ij E_ij ],   gsig = sum_n tr gC
//     glx_k   = sum_n [ gmean_k mean_k + sum_l (gcov + gcov^T)_kl S_kl - sum_d gX_dk xcov_dk ]
//
// glx is the belief's side of the lengthscale adjoint: the lengthscales reach the belief only through m~ = m / l,
// S~ = S / (l l^T) and the scaling of xcov, so that side is the contraction of the INPUT adjoint's results (gmean, gcov of
// cbfssm_gp_moment_match_bwd_f64, in the lower-triangle convention) with the inputs themselves -- no second S~ adjoint.
//
// Two passes.  gp_mm_pbwd_point_kernel walks the points (one workgroup, one thread per inducing row): the two D x D
// factorisations by one lane each, the four substitutions per row, the mean-side terms into the workgroup's partial, and
// t_i, g_i, m~, log c2 and the flag per point into `work`.  gp_mm_pbwd_tile_kernel is TILE-OUTER: a workgroup owns one
// 16 x 16 tile (ib, jb) of the M x M images and a chunk of the points (grid.y); a thread owns one entry and keeps its Do + 1
// accumulators (Wbar_d, Ehat) and its W_d entries in registers over the point loop, so no image is read-modify-written;
// the per-row sums over j go through two 16 x 16 LDS tiles (Q, E).  Every (tile, chunk) writes its own partial; the
// partials are summed in a fixed order (gp_mm_pbwd_reduce_kernel).  Once per call: X_d = K^-1 Wbar_d, then every entry of the
// slab by one thread (gp_mm_pbwd_slab_kernel):
//
//     gMu = K^-1 abar,   gS2_id = -(X_d K^-1)_ii,   gZ_ik = Rbar_ik - ehat_i z~_ik + (Ehat Z~)_ik   (column D: zero)
//     gB  = sym( sum_d [ abar_d mu_d^T + Wbar_d - 2 diag(s2_d) X_d ] )
//
// Workgroup barriers only; no atomics, no inline assembly; one writer per entry; two calls are bitwise identical.  Rows and
// columns >= M of every image are exactly zero.  A point whose factorisation meets a non-positive pivot runs on the
// stand-in pivot 1, contributes exact zeros by select, and makes every data entry of the slab NaN by select at the end.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cbfssm {

constexpr int PBWD_ROWS = 320;            // threads of the point pass: one per inducing row (CBFSSM_MAX_M)
constexpr int PBWD_MAXWG = 512;           // workgroups of the point pass (persistent over the points beyond that)
constexpr int PBWD_MAXCHUNK = 64;         // point chunks of the tile pass
constexpr int PBWD_TILE_TARGET = 2048;    // workgroups the tile pass aims for

struct GpMmPbwdArgs {
    // the model: dense sections of the pack and the constrained flat vector
    const double* Kinv;    // [M][M]
    const double* Zs;      // [M][D]
    const double* mu;      // [M][Do]
    const double* s2;      // [M][Do]
    const double* ls;      // [D]
    const double* var;     // [1]
    // the call
    const double* mean;    // (npts, D)
    const double* cov;     // (npts, D, D) lower triangle, or NULL
    const double* gf;      // (npts, Do) or NULL
    const double* gC;      // (npts, Do, Do) or NULL
    const double* gX;      // (npts, Do, D) or NULL
    const double* gmean;   // (npts, D): the input adjoint's result
    const double* gcov;    // (npts, D, D) or NULL with cov
    const double* xcov;    // (npts, Do, D): the forward's result (read only with gX)
    int64_t npts;
    int M, D, Do, NB;      // NB = ceil(M / 16)
    // sections of `work`
    double* alpha;         // [M][Do]
    double* Wd;            // [Do][M][M]
    double* tq;            // [npts][M][D]   t_i = B^-1 r_i
    double* gq;            // [npts][M]      g_i
    double* mt;            // [npts][D]      m~
    double* ps;            // [npts][2]      log c2, 1 (0: flagged)
    double* P1;            // [nwg1][p1]     partials of the point pass: abar [M][Do] | Rbar [M][D] | glx [D] | 4 scalars
    int64_t p1;
    int nwg1;
    double* P2e;           // [nchunk][Do + 1][M][M]
    double* P2r;           // [nchunk][NB][M][D]
    double* P2a;           // [nchunk][NB][M][Do]
    int nchunk;
    int64_t pc;            // points per chunk
    double* Wbar;          // [Do + 1][M][M]: Wbar_d, then Ehat
    double* abar;          // [M][Do]
    double* Rbar;          // [M][D]
    double* glx;           // [D]
    double* scal;          // [4]: sum ebar, sum tr gC, flagged points, 0
    double* ehat;          // [M]
    double* X;             // [Do][M][M]
    // the results
    double* slab;
    double* gB_dense;      // [M][M] (stash layouts) or NULL
    int NBLK, JB, stash;
    int64_t slab_total;
};

__device__ __forceinline__ double pbwd_block_sum(double v, double* red, int tid, int nwaves)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < nwaves; ++i) s += red[i];          // fixed order
    return s;
}

// alpha = K^-1 mu, one thread per entry
__global__ __launch_bounds__(256) void gp_mm_pbwd_alpha_kernel(GpMmPbwdArgs a)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.M * a.Do) return;
    const int i = idx / a.Do, d = idx - i * a.Do;
    double s = 0.0;
    for (int k = 0; k < a.M; ++k) s = fma(a.Kinv[int64_t(i) * a.M + k], a.mu[k * a.Do + d], s);
    a.alpha[idx] = s;
}

// MODE 0: W_d = K^-1 - K^-1 diag(s2_d) K^-1.   MODE 1: X_d = K^-1 Wbar_d.   grid (NB, NB, Do), 16 x 16 threads
template <int MODE>
__global__ __launch_bounds__(256) void gp_mm_pbwd_gemm_kernel(GpMmPbwdArgs a)
{
    __shared__ double As[16][17], Bs[16][17];
    const int M = a.M, d = blockIdx.z, tx = threadIdx.x, ty = threadIdx.y;
    const int i = blockIdx.y * 16 + ty, j = blockIdx.x * 16 + tx;
    const double* Bm = (MODE == 0) ? a.Kinv : a.Wbar + int64_t(d) * M * M;
    double acc = 0.0;
    for (int k0 = 0; k0 < M; k0 += 16) {
        double av = 0.0, bv = 0.0;
        if (i < M && k0 + tx < M) {
            av = a.Kinv[int64_t(i) * M + k0 + tx];
            if (MODE == 0) av *= a.s2[(k0 + tx) * a.Do + d];
        }
        if (k0 + ty < M && j < M) bv = Bm[int64_t(k0 + ty) * M + j];
        As[ty][tx] = av;
        Bs[ty][tx] = bv;
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) acc = fma(As[ty][kk], Bs[kk][tx], acc);
        __syncthreads();
    }
    if (i < M && j < M) {
        const int64_t o = (int64_t(d) * M + i) * M + j;
        if (MODE == 0) a.Wd[o] = a.Kinv[int64_t(i) * M + j] - acc;
        else a.X[o] = acc;
    }
}

// The per-point pass.  DP: the input width padded to 8, 16 or 24 (the padding dimensions carry the identity factor and
// r = 0); the substitutions are unrolled over DP with the rows' vectors in registers, the factors are broadcast LDS reads.
template <int DP>
__global__ __launch_bounds__(PBWD_ROWS) void gp_mm_pbwd_point_kernel(GpMmPbwdArgs a)
{
    constexpr int DS = DP + 1;
    __shared__ double L1[DP * DS], L2[DP * DS], St[DP * DS];
    __shared__ double inv1[DP], inv2[DP], mts[DP], lsv[DP];
    __shared__ double Gs[16 * 17], gfv[16], fb[16], fm[16];
    __shared__ double Hb[DP * 17];                        // Hbar [k][d]
    __shared__ double qs[PBWD_ROWS];
    __shared__ double red[8];
    __shared__ double sc[4];                              // c1, log c2, flag of either factor
    const int tid = threadIdx.x, M = a.M, D = a.D, Do = a.Do;
    const int i = tid;
    const bool row = i < M;
    double* Pa = a.P1 + int64_t(blockIdx.x) * a.p1;
    double* Pr = Pa + M * Do;
    double* Pl = Pr + M * D;
    double* Psc = Pl + D;
    if (row) {
        for (int d = 0; d < Do; ++d) Pa[i * Do + d] = 0.0;
        for (int k = 0; k < D; ++k) Pr[i * D + k] = 0.0;
    }
    if (tid < DP) lsv[tid] = tid < D ? a.ls[tid] : 1.0;
    const double v = a.var[0];
    double glx_acc = 0.0, se_acc = 0.0, sg_acc = 0.0, nflag = 0.0;
    __syncthreads();
    for (int64_t n = blockIdx.x; n < a.npts; n += gridDim.x) {
        __syncthreads();
        // 1. the belief in lengthscale units, the cotangents
        for (int e = tid; e < DP * DP; e += PBWD_ROWS) {
            const int k = e / DP, l = e - k * DP;
            double s = 0.0;
            if (a.cov && k < D && l < D) {
                const int hi = k > l ? k : l, lo = k > l ? l : k;
                s = a.cov[(n * D + hi) * D + lo] / (lsv[k] * lsv[l]);
            }
            St[k * DS + l] = s;
            L1[k * DS + l] = s + (k == l ? 1.0 : 0.0);
            L2[k * DS + l] = s + (k == l ? 0.5 : 0.0);
        }
        if (tid < DP) mts[tid] = tid < D ? a.mean[n * D + tid] / lsv[tid] : 0.0;
        if (tid < 256) {
            const int d = tid >> 4, e = tid & 15;
            double g = 0.0;
            if (a.gC && d < Do && e < Do) g = 0.5 * (a.gC[(n * Do + d) * Do + e] + a.gC[(n * Do + e) * Do + d]);
            Gs[d * 17 + e] = g;
        }
        if (tid < 16) gfv[tid] = (a.gf && tid < Do) ? a.gf[n * Do + tid] : 0.0;
        __syncthreads();
        // 2. the two factorisations, one lane each (row by row, in place)
        if (tid == 0 || tid == 64) {
            double* L = tid ? L2 : L1;
            double* inv = tid ? inv2 : inv1;
            double ld = 0.0, bad = 0.0;
            for (int k = 0; k < D; ++k) {
                for (int c = 0; c < k; ++c) {
                    double s = L[k * DS + c];
                    for (int jj = 0; jj < c; ++jj) s = fma(-L[k * DS + jj], L[c * DS + jj], s);
                    L[k * DS + c] = s * inv[c];
                }
                double p = L[k * DS + k];
                for (int jj = 0; jj < k; ++jj) p = fma(-L[k * DS + jj], L[k * DS + jj], p);
                if (!(p > 0.0)) { bad = 1.0; p = 1.0; }      // finite stand-in; the point is flagged
                const double lkk = sqrt(p);
                L[k * DS + k] = lkk;
                inv[k] = 1.0 / lkk;
                ld += log(lkk);
            }
            for (int k = D; k < DP; ++k) { L[k * DS + k] = 1.0; inv[k] = 1.0; }
            if (tid == 0) { sc[0] = v * exp(-ld); sc[2] = bad; }
            else { sc[1] = 2.0 * log(v) - 0.5 * D * 0.69314718055994530942 - ld; sc[3] = bad; }
        }
        __syncthreads();
        const bool valid = (sc[2] == 0.0) && (sc[3] == 0.0);
        // 3. per row: a1 = A^-1 r, t = B^-1 r, q, g
        double r[DP], a1[DP];
        double q = 0.0;
        if (row) {
            double x[DP];
#pragma unroll
            for (int k = 0; k < DP; ++k) r[k] = k < D ? a.Zs[i * D + k] - mts[k] : 0.0;
            double ww = 0.0;
#pragma unroll
            for (int k = 0; k < DP; ++k) {
                double s = r[k];
#pragma unroll
                for (int jj = 0; jj < k; ++jj) s = fma(-L1[k * DS + jj], x[jj], s);
                x[k] = s * inv1[k];
                ww = fma(x[k], x[k], ww);
            }
            q = sc[0] * exp(-0.5 * ww);
#pragma unroll
            for (int k = DP - 1; k >= 0; --k) {
                double s = x[k];
#pragma unroll
                for (int jj = k + 1; jj < DP; ++jj) s = fma(-L1[jj * DS + k], a1[jj], s);
                a1[k] = s * inv1[k];
            }
            double g = 0.0;
#pragma unroll
            for (int k = 0; k < DP; ++k) {
                double s = r[k];
#pragma unroll
                for (int jj = 0; jj < k; ++jj) s = fma(-L2[k * DS + jj], x[jj], s);
                x[k] = s * inv2[k];
                g = fma(x[k], x[k], g);
            }
#pragma unroll
            for (int k = DP - 1; k >= 0; --k) {
                double s = x[k];
#pragma unroll
                for (int jj = k + 1; jj < DP; ++jj) s = fma(-L2[jj * DS + k], x[jj], s);
                x[k] = s * inv2[k];
            }
            double* tq = a.tq + (n * M + i) * D;
#pragma unroll
            for (int k = 0; k < DP; ++k)
                if (k < D) tq[k] = x[k];
            a.gq[n * M + i] = g;
            qs[i] = q;
        }
        __syncthreads();
        // fmean (threads 0 .. Do-1) and Hbar = A^-1 S~ diag(l) gX^T (threads 64 .. 64+Do-1)
        if (tid < Do) {
            double s = 0.0;
            for (int m = 0; m < M; ++m) s = fma(a.alpha[m * Do + tid], qs[m], s);
            fm[tid] = s;
        }
        if (tid >= 64 && tid < 64 + 16) {
            const int d = tid - 64;
            double x[DP];
            if (a.gX && d < Do) {
#pragma unroll
                for (int k = 0; k < DP; ++k) {
                    double s = 0.0;
                    for (int l = 0; l < D; ++l) s = fma(St[k * DS + l], lsv[l] * a.gX[(n * Do + d) * D + l], s);
                    x[k] = s;
                }
#pragma unroll
                for (int k = 0; k < DP; ++k) {
                    double s = x[k];
#pragma unroll
                    for (int jj = 0; jj < k; ++jj) s = fma(-L1[k * DS + jj], x[jj], s);
                    x[k] = s * inv1[k];
                }
#pragma unroll
                for (int k = DP - 1; k >= 0; --k) {
                    double s = x[k];
#pragma unroll
                    for (int jj = k + 1; jj < DP; ++jj) s = fma(-L1[jj * DS + k], x[jj], s);
                    x[k] = s * inv1[k];
                }
            } else {
#pragma unroll
                for (int k = 0; k < DP; ++k) x[k] = 0.0;
            }
#pragma unroll
            for (int k = 0; k < DP; ++k) Hb[k * 17 + d] = x[k];
        }
        __syncthreads();
        if (tid < 16) {
            double s = gfv[tid];
            for (int e = 0; e < Do; ++e) s = fma(-2.0 * Gs[tid * 17 + e], fm[e], s);
            fb[tid] = tid < Do ? s : 0.0;
        }
        __syncthreads();
        // 5. per row: qbar, ebar, the mean-side terms of abar and Rbar
        double eb = 0.0;
        if (row) {
            double al[16];
#pragma unroll
            for (int d = 0; d < 16; ++d) al[d] = d < Do ? a.alpha[i * Do + d] : 0.0;
            double qb = 0.0;
#pragma unroll
            for (int d = 0; d < 16; ++d) qb = fma(al[d], fb[d], qb);
            double ha[DP];
#pragma unroll
            for (int k = 0; k < DP; ++k) {
                double s = 0.0;
#pragma unroll
                for (int d = 0; d < 16; ++d) s = fma(Hb[k * 17 + d], al[d], s);
                ha[k] = s;
                qb = fma(r[k], s, qb);
            }
            eb = qb * q;
            if (valid) {
#pragma unroll
                for (int k = 0; k < DP; ++k)
                    if (k < D) Pr[i * D + k] += q * ha[k] - eb * a1[k];
#pragma unroll
                for (int d = 0; d < 16; ++d)
                    if (d < Do) {
                        double s = fb[d];
#pragma unroll
                        for (int k = 0; k < DP; ++k) s = fma(Hb[k * 17 + d], r[k], s);
                        Pa[i * Do + d] += q * s;
                    }
            }
        }
        const double se = pbwd_block_sum((row && valid) ? eb : 0.0, red, tid, PBWD_ROWS / 64);
        if (tid == 0) {
            double tr = 0.0;
            for (int d = 0; d < Do; ++d) tr += Gs[d * 17 + d];
            if (valid) { se_acc += se; sg_acc += tr; }
            else nflag += 1.0;
            a.ps[2 * n] = sc[1];
            a.ps[2 * n + 1] = valid ? 1.0 : 0.0;
        }
        // the belief's side of the lengthscale adjoint, and m~ for the tile pass
        if (tid < D) {
            const int k = tid;
            double term = a.gmean[n * D + k] * a.mean[n * D + k];
            if (a.cov) {
                for (int l = 0; l < D; ++l) {
                    const int hi = k > l ? k : l, lo = k > l ? l : k;
                    const double gv = a.gcov[(n * D + hi) * D + lo];
                    term = fma(k == l ? 2.0 * gv : gv, a.cov[(n * D + hi) * D + lo], term);
                }
            }
            if (a.gX)
                for (int d = 0; d < Do; ++d) term = fma(-a.gX[(n * Do + d) * D + k], a.xcov[(n * Do + d) * D + k], term);
            glx_acc += valid ? term : 0.0;
            a.mt[n * D + k] = mts[k];
        }
    }
    if (tid < D) Pl[tid] = glx_acc;
    if (tid == 0) { Psc[0] = se_acc; Psc[1] = sg_acc; Psc[2] = nflag; Psc[3] = 0.0; }
}

// The tile-outer pass: grid (NB * NB, nchunk), 256 threads, thread (il, jl) owns entry (16 ib + il, 16 jb + jl).
__global__ __launch_bounds__(256) void gp_mm_pbwd_tile_kernel(GpMmPbwdArgs a)
{
    constexpr int DS = 25;
    __shared__ double zI[16 * DS], tI[16 * DS], tJ[16 * DS], rI[16 * DS];
    __shared__ double aI[16 * 17], aJ[16 * 17], Gs[16 * 17], beta[16 * 17], Qt[16 * 17], Et[16 * 17];
    __shared__ double gI[16], gJ[16], gcd[16], psc[2];
    const int tid = threadIdx.x, il = tid >> 4, jl = tid & 15;
    const int M = a.M, D = a.D, Do = a.Do, NB = a.NB;
    const int ib = blockIdx.x / NB, jb = blockIdx.x - ib * NB, chunk = blockIdx.y;
    const int i = 16 * ib + il, j = 16 * jb + jl;
    const bool in = i < M && j < M;
    for (int e = tid; e < 16 * DS; e += 256) {
        const int rw = e / DS, k = e - rw * DS, gi = 16 * ib + rw;
        zI[e] = (gi < M && k < D) ? a.Zs[gi * D + k] : 0.0;
    }
    aI[il * 17 + jl] = (i < M && jl < Do) ? a.alpha[i * Do + jl] : 0.0;
    aJ[il * 17 + jl] = (16 * jb + il < M && jl < Do) ? a.alpha[(16 * jb + il) * Do + jl] : 0.0;
    double mq = 0.0;
    if (in) {
        double d2 = 0.0;
        for (int k = 0; k < D; ++k) {
            const double df = a.Zs[i * D + k] - a.Zs[j * D + k];
            d2 = fma(df, df, d2);
        }
        mq = -0.25 * d2;
    }
    double wd[16], accW[16];
#pragma unroll
    for (int d = 0; d < 16; ++d) {
        wd[d] = (in && d < Do) ? a.Wd[(int64_t(d) * M + i) * M + j] : 0.0;
        accW[d] = 0.0;
    }
    double accE = 0.0, accR0 = 0.0, accR1 = 0.0, accA = 0.0;
    const int64_t n0 = int64_t(chunk) * a.pc;
    const int64_t n1 = n0 + a.pc < a.npts ? n0 + a.pc : a.npts;
    for (int64_t n = n0; n < n1; ++n) {
        __syncthreads();
        for (int e = tid; e < 16 * DS; e += 256) {
            const int rw = e / DS, k = e - rw * DS, gi = 16 * ib + rw, gj = 16 * jb + rw;
            const bool ki = gi < M && k < D, kj = gj < M && k < D;
            tI[e] = ki ? a.tq[(n * M + gi) * D + k] : 0.0;
            tJ[e] = kj ? a.tq[(n * M + gj) * D + k] : 0.0;
            rI[e] = ki ? zI[e] - a.mt[n * D + k] : 0.0;
        }
        if (tid < 16) {
            gI[tid] = (16 * ib + tid < M) ? a.gq[n * M + 16 * ib + tid] : 0.0;
            gJ[tid] = (16 * jb + tid < M) ? a.gq[n * M + 16 * jb + tid] : 0.0;
            gcd[tid] = tid < Do ? a.gC[(n * Do + tid) * Do + tid] : 0.0;
        }
        Gs[il * 17 + jl] = (il < Do && jl < Do) ? 0.5 * (a.gC[(n * Do + il) * Do + jl] + a.gC[(n * Do + jl) * Do + il]) : 0.0;
        if (tid == 0) { psc[0] = a.ps[2 * n]; psc[1] = a.ps[2 * n + 1]; }
        __syncthreads();
        {   // beta[jj = il][d = jl] = (Gs alpha_jj)_d
            double b = 0.0;
            for (int e = 0; e < Do; ++e) b = fma(Gs[jl * 17 + e], aJ[il * 17 + e], b);
            beta[il * 17 + jl] = b;
        }
        __syncthreads();
        double uu = 0.0;
        for (int k = 0; k < D; ++k) uu = fma(rI[il * DS + k], tJ[jl * DS + k], uu);
        const double Q = (in && psc[1] != 0.0) ? exp(psc[0] + mq - 0.125 * (gI[il] + gJ[jl] + 2.0 * uu)) : 0.0;
        double qb = 0.0;
#pragma unroll
        for (int d = 0; d < 16; ++d) {
            qb = fma(aI[il * 17 + d], beta[jl * 17 + d], qb);
            qb = fma(-gcd[d], wd[d], qb);
            accW[d] = fma(-gcd[d], Q, accW[d]);
        }
        const double E = qb * Q;
        accE += E;
        Qt[il * 17 + jl] = Q;
        Et[il * 17 + jl] = E;
        __syncthreads();
        {   // row il, column jl (and jl + 16) of sum_j E_ij (t_i + t_j); column jl of sum_j Q_ij beta_j
            double s0 = 0.0, s1 = 0.0, sa = 0.0;
            const bool c0 = jl < D, c1 = jl + 16 < D;
            const double ti0 = c0 ? tI[il * DS + jl] : 0.0, ti1 = c1 ? tI[il * DS + jl + 16] : 0.0;
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) {
                const double e = Et[il * 17 + jj];
                if (c0) s0 = fma(e, tJ[jj * DS + jl] + ti0, s0);
                if (c1) s1 = fma(e, tJ[jj * DS + jl + 16] + ti1, s1);
                sa = fma(Qt[il * 17 + jj], beta[jj * 17 + jl], sa);
            }
            accR0 += s0;
            accR1 += s1;
            accA += sa;
        }
    }
    if (in) {
        double* Pe = a.P2e + int64_t(chunk) * (Do + 1) * M * M + int64_t(i) * M + j;
#pragma unroll
        for (int d = 0; d < 16; ++d)
            if (d < Do) Pe[int64_t(d) * M * M] = accW[d];
        Pe[int64_t(Do) * M * M] = accE;
    }
    if (i < M) {
        double* Prr = a.P2r + ((int64_t(chunk) * NB + jb) * M + i) * D;
        if (jl < D) Prr[jl] = accR0;
        if (jl + 16 < D) Prr[jl + 16] = accR1;
        if (jl < Do) a.P2a[((int64_t(chunk) * NB + jb) * M + i) * Do + jl] = accA;
    }
}

// the partials summed in a fixed order: Wbar / Ehat, abar, Rbar, glx, the scalars; one thread per entry
__global__ __launch_bounds__(256) void gp_mm_pbwd_reduce_kernel(GpMmPbwdArgs a)
{
    const int M = a.M, D = a.D, Do = a.Do, NB = a.NB;
    const bool hasC = a.gC != nullptr;
    const int64_t nE = int64_t(Do + 1) * M * M, nA = int64_t(M) * Do, nR = int64_t(M) * D;
    int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (idx < nE) {
        double s = 0.0;
        if (hasC)
            for (int c = 0; c < a.nchunk; ++c) s += a.P2e[int64_t(c) * nE + idx];
        a.Wbar[idx] = s;
        return;
    }
    idx -= nE;
    if (idx < nA) {
        double s = 0.0, s2 = 0.0;
        for (int w = 0; w < a.nwg1; ++w) s += a.P1[int64_t(w) * a.p1 + idx];
        if (hasC)
            for (int c = 0; c < a.nchunk * NB; ++c) s2 += a.P2a[int64_t(c) * nA + idx];
        a.abar[idx] = s + 2.0 * s2;
        return;
    }
    idx -= nA;
    if (idx < nR) {
        double s = 0.0, s2 = 0.0;
        for (int w = 0; w < a.nwg1; ++w) s += a.P1[int64_t(w) * a.p1 + nA + idx];
        if (hasC)
            for (int c = 0; c < a.nchunk * NB; ++c) s2 += a.P2r[int64_t(c) * nR + idx];
        a.Rbar[idx] = s - 0.5 * s2;
        return;
    }
    idx -= nR;
    if (idx < D + 4) {
        double s = 0.0;
        for (int w = 0; w < a.nwg1; ++w) s += a.P1[int64_t(w) * a.p1 + nA + nR + idx];
        if (idx < D) a.glx[idx] = s;
        else a.scal[idx - D] = s;
    }
}

// ehat_i = sum_j Ehat_ij: one wave per row
__global__ __launch_bounds__(64) void gp_mm_pbwd_rowsum_kernel(GpMmPbwdArgs a)
{
    const int i = blockIdx.x, l = threadIdx.x, M = a.M;
    const double* Eh = a.Wbar + int64_t(a.Do) * M * M;
    double s = 0.0;
    for (int j = l; j < M; j += 64) s += Eh[int64_t(i) * M + j];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (l == 0) a.ehat[i] = s;
}

__device__ __forceinline__ double pbwd_kib_half(const GpMmPbwdArgs& a, int i, int j, bool hasC)
{
    const int M = a.M, Do = a.Do;
    double s = 0.0;
    for (int d = 0; d < Do; ++d) {
        s = fma(a.abar[i * Do + d], a.mu[j * Do + d], s);
        if (hasC) {
            const int64_t o = (int64_t(d) * M + i) * M + j;
            s += a.Wbar[o] - 2.0 * a.s2[i * Do + d] * a.X[o];
        }
    }
    return s;
}

// every entry of the slab (and of the dense K^-1 adjoint) by one thread
__global__ __launch_bounds__(256) void gp_mm_pbwd_slab_kernel(GpMmPbwdArgs a)
{
    const int M = a.M, D = a.D, Do = a.Do, NBLK = a.NBLK, JB = a.JB;
    const bool hasC = a.gC != nullptr;
    const bool flagged = a.scal[2] > 0.0;
    const double nan = __builtin_nan("");
    int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (idx >= a.slab_total) {                            // the dense image, row-major [M][M]
        idx -= a.slab_total;
        if (!a.gB_dense || idx >= int64_t(M) * M) return;
        const int i = int(idx / M), j = int(idx - int64_t(i) * M);
        const double vv = 0.5 * (pbwd_kib_half(a, i, j, hasC) + pbwd_kib_half(a, j, i, hasC));
        a.gB_dense[idx] = flagged ? nan : vv;
        return;
    }
    const int64_t oS2 = int64_t(NBLK) * 256, oB = 2 * oS2, oZ = oB + (a.stash ? 0 : int64_t(NBLK) * NBLK * 256),
                  oSm = oZ + int64_t(NBLK) * JB * 256;
    double val = 0.0;
    bool data = false;
    if (idx >= oSm) {
        const int s = int(idx - oSm);
        if (s >= 32 && s < 32 + D) { val = a.glx[s - 32]; data = true; }
        else if (s == 96) { val = a.scal[1]; data = true; }
        else if (s == 97) {
            double t = 0.0;
            if (hasC)
                for (int m = 0; m < M; ++m) t += a.ehat[m];
            val = a.scal[0] + 2.0 * t;
            data = true;
        }
    } else {
        // an MFMA C-layout image [rb][cb][4][64]: row = 16 rb + (lane >> 4) + 4 r, col = 16 cb + (lane & 15)
        const int64_t base = idx < oS2 ? 0 : (idx < oB ? oS2 : (idx < oZ ? oB : oZ));
        const int ncb = idx < oB ? 1 : (idx < oZ ? NBLK : JB);
        const int64_t rel = idx - base;
        const int blk = int(rel >> 8), rr = int(rel >> 6) & 3, lane = int(rel & 63);
        const int rb = blk / ncb, cb = blk - rb * ncb;
        const int rowi = 16 * rb + (lane >> 4) + 4 * rr, col = 16 * cb + (lane & 15);
        if (idx < oS2) {                                  // gMu = K^-1 abar
            if (rowi < M && col < Do) {
                double s = 0.0;
                for (int k = 0; k < M; ++k) s = fma(a.Kinv[int64_t(rowi) * M + k], a.abar[k * Do + col], s);
                val = s; data = true;
            }
        } else if (idx < oB) {                            // gS2_id = -(X_d K^-1)_ii
            if (rowi < M && col < Do) {
                double s = 0.0;
                if (hasC)
                    for (int k = 0; k < M; ++k) s = fma(a.X[(int64_t(col) * M + rowi) * M + k], a.Kinv[int64_t(k) * M + rowi], s);
                val = -s; data = true;
            }
        } else if (idx < oZ) {                            // gB (not in stash layouts)
            if (rowi < M && col < M) {
                val = 0.5 * (pbwd_kib_half(a, rowi, col, hasC) + pbwd_kib_half(a, col, rowi, hasC));
                data = true;
            }
        } else {                                          // gZ: the Z~ adjoint itself in columns < D, column D (ones row) zero
            if (rowi < M && col < D) {
                double s = a.Rbar[rowi * D + col];
                if (hasC) {
                    const double* Eh = a.Wbar + int64_t(Do) * M * M + int64_t(rowi) * M;
                    double t = 0.0;
                    for (int m = 0; m < M; ++m) t = fma(Eh[m], a.Zs[m * D + col], t);
                    s += t - a.ehat[rowi] * a.Zs[rowi * D + col];
                }
                val = s; data = true;
            }
        }
    }
    a.slab[idx] = (data && flagged) ? nan : val;
}

}  // namespace cbfssm
