// Fused time loop of ONE sparse GP with a per-step, per-chain Gaussian filter update, and its adjoint: the conditioned
// forward step of CBF-SSM (cbfssm/model/cbfssm.py:185-237) for N independent chains with PER-CHAIN auxiliary inputs
// a (T, N, Da), per-chain pseudo-observations ytilde (T, N, Do) and a mask cond (T, N):
//     m = h + fmean(h, a_t),  v = fvar(h, a_t) + var_x                                               (:199-206)
//     cond[t, n]:  r = var_y + (k_factor - 1) v,  s = r + v,  k = v / s,  delta = ytilde_t - m         (:212-217)
//                  mu = m + k delta,  sig = (1 - k)^2 v + k^2 r,  h <- mu + eps_t sqrt(sig)            (:218-221)
//                  kl += 0.5 (log v - log sig + (sig + (mu - m)^2) / v - 1)                            (:232-234)
//     otherwise:   h <- m + eps_t sqrt(v)                                                              (:224)
// gp_rollout (cbfssm_gp_rollout.hpp) is the case cond = 0; the pass kernels (cbfssm_kernels.hpp) condition, but on
// inputs shared by the particles of a sequence, on pseudo-observations that are no differentiable input and behind one
// global switch.
//
// gp_filter_kernel: the structure of gp_rollout_kernel (one workgroup per 16 chains, Tile::phase1, phase2 / phase2_tri,
// gather, three barriers per step); only the epilogue per (chain, state dim) lane differs.  The two branches are chosen
// by SELECT: a ytilde entry at cond = 0 may be NaN (missing data) and reaches no output.  With 1 - k = r / s the update
// is evaluated as the pass kernel does: sig = k r, sig / v = r / s, (mu - m)^2 / v = k delta^2 / s, so
//     kl = 0.5 sum [ k (delta^2 / s - 1) - log(r / s) ]
// with the logarithm through LogProd (one log per lane and pass) and the rational part as a plain sum; one partial per
// workgroup.  m and v of every step are kept for the adjoint (msave, vsave).
//
// gp_filter_bwd_kernel: gp_rollout_bwd_kernel with another formation of Fm / Fv at the top of a step and another carry
// at its bottom.  With g = gtraj[t] + carry, g_kl = d loss / d kl and delta, k, sig recomputed from the saved m, v:
//     cond = 0:  Fm = g,  Fv = g eps / (2 sqrt v),  gytilde[t] = 0
//     cond = 1:  sigb = g eps / (2 sqrt sig) + g_kl (1 / v - 1 / sig) / 2
//                kb   = g delta + g_kl k delta^2 / v            (+ sigb (2 k r - 2 (1 - k) v), which is 0 at k = v / s)
//                db   = g k + g_kl k^2 delta / v                                     -> gytilde[t] = db
//                rb   = sigb k^2 - kb v / s^2                                        -> d / d var_y += rb
//                Fv   = sigb (1 - k)^2 + g_kl (1 / v - sig / v^2 - k^2 delta^2 / v^2) / 2 + kb r / s^2 + (k_factor - 1) rb
//                Fm   = g - db
// After phase G the state rows of gX plus Fm are the next carry (h enters m directly and through the GP).  sum Fv per
// state dim goes to the slab's d/d var_x entries, sum rb to its d/d var_y entries.
// Phases B to F, the row-block setup and the slab write are the shared body of cbfssm_gp_tile.hpp (GpWave), as in the
// rollout adjoint and the batch kernel; gp_ekf_bwd_kernel (cbfssm_gp_ekf_bwd.hpp) builds on the same pieces.
// No atomics, one writer per output: two calls are bitwise identical.  Padded chains carry zero adjoints
// and the rows m >= M of the tiles are zero, so both contribute exactly zero.
#pragma once
#include "cbfssm_gp_bwd.hpp"

namespace cbfssm {

struct GpFiltArgs {
    PackPtrs pk;
    const double* h0;        // (N, Do)
    const double* a;         // (T, N, Da), Da = D - Do (unused when Da = 0)
    const double* ytilde;    // (T, N, Do): entries at cond = 0 are never used (they may be NaN)
    const double* cond;      // (T, N) 0 / 1, or null: condition everywhere
    const double* eps;       // (T, N)
    const double* var_x;     // (Do) or null
    const double* var_y;     // (Do)
    double k_factor;
    double* traj;            // (T, N, Do)
    double* msave;           // (T, N, Do) or null (with vsave): m = h + fmean and v = fvar + var_x of every step
    double* vsave;
    double* kl_part;         // one partial per workgroup
    int N, T, D, Do, reverse;
    int tri;
};

struct GpFiltBwdArgs {
    PackPtrs pk;
    RevPackPtrs rk;
    const double* h0;
    const double* a;
    const double* ytilde;
    const double* cond;
    const double* eps;
    const double* var_y;
    double k_factor;
    const double* traj;
    const double* msave;
    const double* vsave;
    const double* gtraj;     // (T, N, Do): d loss / d traj
    const double* g_kl;      // one double on the device: d loss / d kl
    double* gh0;             // (N, Do)
    double* ga;              // (T, N, Da)
    double* gytilde;         // (T, N, Do)
    double* gpart;           // [workgroup][slab]
    int64_t slab;
    double* stash_a;         // stash tile heights: [workgroup * T + step][NBLK][4][64] operand images (A2bar^T, K^T)
    double* stash_k;
    int N, T, M, D, Do, reverse;
};

template <int NBLK, int RB, int DK, bool BREG, bool TRI, int KT>
__global__ __launch_bounds__(64 * ((NBLK + RB - 1) / RB)) void gp_filter_kernel(GpFiltArgs a)
{
    typedef Tile<NBLK, RB, DK, BREG, TRI, KT> TT;
    constexpr int W = TT::W, NT = TT::NT, QPW = TT::QPW;
    constexpr int AUXR = (DK * 64 + NT - 1) / NT;
    extern __shared__ double lds[];
    double* xq = lds;                                // [DK*64]   scaled GP input, row j = index >> 4, chain = index & 15
    double* Kt = xq + DK * 64;                       // [MP*16]
    double* part = Kt + TT::MP * 16;                 // [W][512]
    double* red = part + W * 512;                    // 64
    double* At = red + 64;                           // TRI: A = L^-1 k tile, then the waves' flags
    int* flag = reinterpret_cast<int*>(At + TT::MP * 16);

    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, g = l >> 4, nl = l & 15;
    const int N = a.N, T = a.T, Do = a.Do;
    const int naux = a.D - Do;
    const int c0 = blockIdx.x * 16;
    const int dir = a.reverse ? -1 : 1;
    const int t_first = a.reverse ? T - 1 : 0;
    const double kf1 = a.k_factor - 1.0;

    TT tile;
    tile.load_operands(a.pk, w, l);

    // per-lane constants of the epilogue tasks of this wave: state-row group q = w + qi W < 4, row d = 4 q + g, chain nl
    double vx[QPW], vy[QPW], il[QPW], hcur[QPW], lin[QPW];
    LogProd lp[QPW];
    bool act[QPW];
    int dcl[QPW];
    const int c = min(c0 + nl, N - 1);
    const bool cval = (c0 + nl) < N;
#pragma unroll
    for (int qi = 0; qi < QPW; ++qi) {
        const int q = w + qi * W;
        const int d = 4 * q + g;
        act[qi] = (q < 4) && (d < Do);
        const int dc = act[qi] ? d : 0;
        dcl[qi] = dc;
        vx[qi] = a.var_x ? a.var_x[dc] : 0.0;
        vy[qi] = a.var_y[dc];
        il[qi] = a.pk.invl[dc];
        hcur[qi] = a.h0[int64_t(c) * Do + dc];
        lin[qi] = 0.0;
        lp[qi].init();
    }

    // auxiliary input rows of this thread: base pointer and 1 / lengthscale are fixed for the whole pass
    const double* auxp[AUXR];
    double auxl[AUXR];
    const int64_t auxs = int64_t(N) * naux;          // time stride of a
#pragma unroll
    for (int k2 = 0; k2 < AUXR; ++k2) {
        const int i = tid + k2 * NT, ja = i >> 4, n = i & 15;
        auxp[k2] = a.pk.invl; auxl[k2] = 0.0;        // (no row: a valid dummy address, factor 0)
        if (i < 16 * naux) {
            auxp[k2] = a.a + int64_t(min(c0 + n, N - 1)) * naux + ja;
            auxl[k2] = a.pk.invl[Do + ja];
        }
    }

    // xq rows [0, Do) carry the chain state, rows [Do, D) the auxiliary inputs, rows [D, 4 DK) stay zero
    for (int i = tid; i < DK * 64; i += NT) xq[i] = 0.0;
    if constexpr (TRI) {
        if (tid < 64) { flag[tid] = 0; flag[tid + 64] = 0; }
    }
    __syncthreads();
    if (T > 0) {
#pragma unroll
        for (int qi = 0; qi < QPW; ++qi)
            if (act[qi]) xq[64 * (w + qi * W) + l] = hcur[qi] * il[qi];
#pragma unroll
        for (int k2 = 0; k2 < AUXR; ++k2) {
            const int i = tid + k2 * NT;
            if (i < 16 * naux) xq[16 * Do + i] = auxp[k2][int64_t(t_first) * auxs] * auxl[k2];
        }
    }

    for (int step = 0; step < T; ++step) {
        const int t = t_first + dir * step;
        const int tn = t + dir;
        const bool has_next = (step + 1 < T);
        __syncthreads();                             // xq complete

        // this step's noise, pseudo-observation and mask and the next step's auxiliary rows, issued ahead of the tile work
        double eps_t, cnd, ytil[QPW], auxr[AUXR];
        eps_t = a.eps[int64_t(t) * N + c];
        cnd = a.cond ? a.cond[int64_t(t) * N + c] : 1.0;
#pragma unroll
        for (int qi = 0; qi < QPW; ++qi) ytil[qi] = a.ytilde[(int64_t(t) * N + c) * Do + dcl[qi]];
#pragma unroll
        for (int k2 = 0; k2 < AUXR; ++k2) {
            const int i = tid + k2 * NT;
            auxr[k2] = (has_next && i < 16 * naux) ? auxp[k2][int64_t(tn) * auxs] : 0.0;
        }

        double kr[RB][4];
        tile.phase1(xq, Kt, kr, w, l);
        // (the loads above land here, a phase after they were issued: see pass_kernel)
        asm volatile("" : "+v"(eps_t), "+v"(cnd));
#pragma unroll
        for (int qi = 0; qi < QPW; ++qi) asm volatile("" : "+v"(ytil[qi]));
#pragma unroll
        for (int k2 = 0; k2 < AUXR; ++k2) asm volatile("" : "+v"(auxr[k2]));
        __syncthreads();
        if constexpr (TRI) tile.phase2_tri(Kt, At, flag, step + 1, part, w, l, nullptr);
        else tile.phase2(Kt, part, kr, w, l, nullptr);
        __syncthreads();                             // part complete; xq and Kt free

        // ---- step epilogue
        const bool do_cond = (cnd != 0.0);
#pragma unroll
        for (int qi = 0; qi < QPW; ++qi) {
            const int q = w + qi * W;
            if (q < 4) {
                double fm, fv;
                tile.gather(part, q, l, fm, fv);
                if (act[qi]) {
                    const int d = 4 * q + g;
                    const double m = hcur[qi] + fm;                                    // cbfssm.py:205
                    const double v = fv + vx[qi];                                      // :206
                    const double r = vy[qi] + kf1 * v;                                 // :212-214
                    const double s = r + v;                                            // :216
                    const double rs = fast_rcp(s);
                    const double kk = v * rs;                                          // :217
                    const double dl = ytil[qi] - m;                                    // :215 (NaN where data is missing)
                    const double mu = m + kk * dl;                                     // :218
                    const double sig = kk * r;                                         // :219-220 with 1 - k = r / s
                    // a select between the two branches: nothing of the conditioned one survives at cond = 0
                    const double hn = do_cond ? (mu + eps_t * (sig * fast_rsqrt(sig)))          // :221
                                              : (m + eps_t * (v * fast_rsqrt(v)));              // :224
                    hcur[qi] = hn;
                    if (cval) {
                        const int64_t o = (int64_t(t) * N + c) * Do + d;
                        a.traj[o] = hn;
                        if (a.msave) { a.msave[o] = m; a.vsave[o] = v; }
                        if (do_cond) {
                            lin[qi] += kk * (dl * dl * rs - 1.0);                      // :232
                            lp[qi].mul(r * rs);
                        }
                    }
                    if (has_next) xq[64 * q + l] = hn * il[qi];
                }
            }
        }
        if (has_next) {
#pragma unroll
            for (int k2 = 0; k2 < AUXR; ++k2) {
                const int i = tid + k2 * NT;
                if (i < 16 * naux) xq[16 * Do + i] = auxr[k2] * auxl[k2];
            }
        }
    }

    // ---- KL partial of this workgroup: 0.5 sum (k (delta^2 / s - 1) - log(r / s)) over the conditioned steps
    double v = 0.0;
#pragma unroll
    for (int qi = 0; qi < QPW; ++qi)
        if (act[qi] && cval) v += 0.5 * (lin[qi] - lp[qi].log());
    double tot = block_sum(v, red, tid, NT);
    if constexpr (TRI) {
        if (tid == 0 && flag[CBF_FLAG_TIMEOUT_SLOT] != 0) tot = __builtin_nan("");   // a hand-off poll ran out (see flag_wait)
    }
    if (tid == 0) a.kl_part[blockIdx.x] = tot;
}

// LDS of the adjoint: the tiles of gp_predict_bwd_kernel plus the carry tile
template <int NBLK, int DK>
struct GpFiltBwdGeom {
    static constexpr int PD = 17;
    static constexpr int LDS_DOUBLES = GpBwdGeom<NBLK, DK>::LDS_DOUBLES + 16 * PD;
    static_assert(LDS_DOUBLES <= 163840 / 8, "LDS budget");
};

template <int NBLK, int RB, int DK, bool STASH>
__global__ __launch_bounds__(64 * ((NBLK + RB - 1) / RB)) void gp_filter_bwd_kernel(GpFiltBwdArgs a)
{
    typedef GpWave<NBLK, RB, DK> WV;
    constexpr int W = WV::W, NT = WV::NT, MP = WV::MP;
    constexpr int JB = WV::JB;
    constexpr int NG = 4 * JB;                          // 4-row groups of the input-adjoint tile
    constexpr int GPW = (NG + W - 1) / W;               // groups per wave in phase G
    constexpr int PD = 17;
    constexpr int PSL = JB * 256;

    extern __shared__ double lds[];
    double* xq = lds;                                   // [4 DK][17] scaled inputs x~[j][n]
    double* Kt = xq + 4 * DK * PD;                      // [MP][17]  kernel tile, then Ebar transposes
    double* A2t = Kt + MP * PD;                         // [MP][17]  A2 transposes, then the A2bar tile
    double* Fm = A2t + MP * PD;                         // [16][17]  d loss / d fmean [d][n]
    double* Fv = Fm + 16 * PD;                          // [16][17]
    double* part = Fv + 16 * PD;                        // [W][PSL]  per-wave partial tiles of (Z~)^T Ebar
    double* red = part + W * PSL;                       // 64
    double* carry = red + 64;                           // [16][17]  adjoint of the state handed to the earlier step [d][n]

    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, g = l >> 4, nl = l & 15;
    const int M = a.M, D = a.D, Do = a.Do, N = a.N, T = a.T;
    const int Da = D - Do;
    const int dir = a.reverse ? -1 : 1;
    const int64_t p0 = int64_t(blockIdx.x) * 16;
    const double gkl = a.g_kl[0];
    const double kf1 = a.k_factor - 1.0;

    WV wv;
    wv.setup(a.pk, tid);

    // ---- accumulators of the parameter adjoints (all steps of this workgroup)
    GpAdjAcc<NBLK, RB, JB, STASH> acc;
    acc.zero();
    double glx[GPW];
#pragma unroll
    for (int k2 = 0; k2 < GPW; ++k2) glx[k2] = 0.0;
    double gsig = 0.0, glogsig = 0.0;
    double gvx = 0.0, gvy = 0.0;                        // sums of Fv and of rb over this thread's (chain, dim = tid & 15) entries
    double ilg[GPW];
#pragma unroll
    for (int k2 = 0; k2 < GPW; ++k2) {
        const int j = 4 * (w + k2 * W) + g;
        ilg[k2] = (j < D) ? a.pk.invl[j] : 0.0;
    }
    const double vyd = ((tid & 15) < Do) ? a.var_y[tid & 15] : 1.0;     // (NT is a multiple of 16: d = tid & 15 below)
    for (int i = tid; i < 16 * PD; i += NT) carry[i] = 0.0;

    for (int sp = T - 1; sp >= 0; --sp) {               // forward step index, last first
        const int t = a.reverse ? T - 1 - sp : sp;
        const int tp = t - dir;                         // time index of the forward step before this one
        __syncthreads();                                // the previous step's readers of xq / part / Fm / Fv are done; carry complete
        for (int i = tid; i < 4 * DK * 16; i += NT) {
            const int j = i >> 4, n = i & 15;
            const int64_t p = p0 + n;
            double v = 0.0;
            if (j < D && p < N) {
                if (j < Do) v = (sp == 0) ? a.h0[p * Do + j] : a.traj[(int64_t(tp) * N + p) * Do + j];
                else v = a.a[(int64_t(t) * N + p) * Da + (j - Do)];
                v *= a.pk.invl[j];
            }
            xq[j * PD + n] = v;
        }
        for (int i = tid; i < 256; i += NT) {
            const int n = i >> 4, d = i & 15;           // (d fastest: the trajectories are (T, N, Do))
            const int64_t p = p0 + n;
            double vm = 0.0, vv = 0.0;
            if (d < Do && p < N) {
                const int64_t o = (int64_t(t) * N + p) * Do + d;
                const double gb = a.gtraj[o] + carry[d * PD + n];
                const double ge = gb * a.eps[int64_t(t) * N + p];
                const double v = a.vsave[o];
                const bool do_cond = a.cond ? (a.cond[int64_t(t) * N + p] != 0.0) : true;
                if (do_cond) {
                    // delta, k, sig of the forward step again (cbfssm.py:212-220), then the adjoint in the header's order
                    const double r = vyd + kf1 * v;
                    const double s = r + v;
                    const double rs = fast_rcp(s), rv = fast_rcp(v);
                    const double k = v * rs, omk = r * rs;
                    const double dl = a.ytilde[o] - a.msave[o];
                    const double sig = k * r;
                    const double rsg = fast_rsqrt(sig);
                    const double kd = k * dl;
                    const double sigb = 0.5 * (ge * rsg + gkl * (rv - rsg * rsg));
                    const double kb = gb * dl + gkl * kd * dl * rv;                    // (d sig / d k = 0 at k = v / s)
                    const double db = gb * k + gkl * k * kd * rv;
                    const double rb = sigb * k * k - kb * k * rs;                      // v / s^2 = k / s
                    vv = sigb * omk * omk + 0.5 * gkl * rv * (1.0 - (sig + kd * kd) * rv) + kb * omk * rs + kf1 * rb;
                    vm = gb - db;
                    gvy += rb;
                    a.gytilde[o] = db;
                } else {
                    vm = gb;
                    vv = 0.5 * ge * fast_rsqrt(v);      // d sqrt(v) = 1 / (2 sqrt v)
                    a.gytilde[o] = 0.0;
                }
            }
            Fm[d * PD + n] = vm;
            Fv[d * PD + n] = vv;
            gvx += vv;
        }
        __syncthreads();

        // ---- B: kernel tile (rows of this wave)
        d4 kreg[RB];
        wv.kernel_tile(xq, Kt, M, kreg);
        __syncthreads();

        // ---- C: A2 rows of this wave (K^-1 streams from L2 as the A-operand image of the pack)
        d4 a2[RB];
        wv.image_times_tile(wv.bop, Kt, a2);

        // ---- E: A2bar, and the parameter adjoints that contract over the 16 chains; stash slot = workgroup * T + step
        GpUpstream up;
        wv.load_upstream(Fm, Fv, up, gsig);
        wv.template phase_E<STASH>(a.rk, up, Kt, A2t, a2, kreg, int64_t(blockIdx.x) * T + sp, a.stash_a, a.stash_k, acc);
        __syncthreads();

        // ---- F: Kbar, Ebar, input adjoint partials, Zbar~
        d4 ebar[RB];
        wv.kbar(A2t, a2, up.fvsum, ebar);
        wv.ebar_of(ebar, kreg, M, ebar);
        wv.phase_F_tail(a.rk.ZT, Kt, xq, part, ebar, D, acc.gZ);
        __syncthreads();

        // ---- G: input adjoint of this step: state rows + Fm -> carry (gh0 at the first forward step), the others -> ga[t]
        {
            const int64_t p = p0 + nl;
            const bool pvalid = p < N;
            double esum = 0.0;                          // colsum of Ebar for this lane's chain = row D of the xbar tile
            const int jbD = D >> 4, qD = (D >> 2) & 3, gD = D & 3;
#pragma unroll
            for (int ww = 0; ww < W; ++ww) esum += part[ww * PSL + (jbD * 4 + qD) * 64 + gD * 16 + nl];
#pragma unroll
            for (int k2 = 0; k2 < GPW; ++k2) {
                const int gi = w + k2 * W;
                if (gi < NG) {
                    const int j = 4 * gi + g;
                    double xb = 0.0;
#pragma unroll
                    for (int ww = 0; ww < W; ++ww) xb += part[ww * PSL + gi * 64 + l];
                    if (j < D && pvalid) {
                        const double xt = xq[j * PD + nl];
                        xb -= xt * esum;
                        glx[k2] += xb * xt;                                        // lengthscale adjoint (inputs)
                        const double gx = xb * ilg[k2];
                        if (j < Do) {
                            const double cv = gx + Fm[j * PD + nl];                // h enters m directly and through the GP
                            if (sp == 0) a.gh0[p * Do + j] = cv;
                            else carry[j * PD + nl] = cv;
                        } else {
                            a.ga[(int64_t(t) * N + p) * Da + (j - Do)] = gx;
                        }
                    }
                    if (j == D && pvalid) glogsig += xb;
                }
            }
        }
    }

    // ---- write this workgroup's slab
    __syncthreads();
    double* slab = a.gpart + int64_t(blockIdx.x) * a.slab;
    wv.template write_slab<STASH>(slab, acc);
    const double gv[2] = {gvx, gvy};                    // d loss / d var_x [0, 16) and d loss / d var_y [16, 32) by state dim
    wv.template write_state_sums<STASH>(slab, part, gv);
    wv.template write_sums<STASH>(slab, glx, gsig, glogsig, red);
}

// ---- launchers: K^-1 placement (registers up to seven row blocks, streamed above), two row blocks per wave from 13 row
// blocks and the compile-time trim of the seven-block tile follow the predict dispatcher (cbfssm_inst.hpp)
template <int NBLK, int DK, int KT>
int launch_gp_filt_k(const GpFiltArgs& a, hipStream_t st)
{
    typedef Cfg<NBLK> C;
    const unsigned groups = unsigned((a.N + 15) / 16);
    if (a.tri) {
        typedef Tile<NBLK, C::RB, DK, C::BREG, true, KT> TT;
        const size_t lds = TT::LDS_DOUBLES * sizeof(double);
        auto k = gp_filter_kernel<NBLK, C::RB, DK, C::BREG, true, KT>;
        int rc = set_lds(k, lds);
        if (rc) return rc;
        hipLaunchKernelGGL(k, dim3(groups), dim3(TT::NT), lds, st, a);
    } else {
        typedef Tile<NBLK, C::RB, DK, C::BREG, false, KT> TT;
        const size_t lds = TT::LDS_DOUBLES * sizeof(double);
        auto k = gp_filter_kernel<NBLK, C::RB, DK, C::BREG, false, KT>;
        int rc = set_lds(k, lds);
        if (rc) return rc;
        hipLaunchKernelGGL(k, dim3(groups), dim3(TT::NT), lds, st, a);
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -int(e) - 1000;
}

template <int NBLK, int DK>
int launch_gp_filt_t(const GpFiltArgs& a, hipStream_t st)
{
    if constexpr (trim_tiles<NBLK>()) {
        switch (4 * NBLK - a.pk.KSr) {
            case 0: return launch_gp_filt_k<NBLK, DK, 0>(a, st);
            case 1: return launch_gp_filt_k<NBLK, DK, 1>(a, st);
            case 2: return launch_gp_filt_k<NBLK, DK, 2>(a, st);
            case 3: return launch_gp_filt_k<NBLK, DK, 3>(a, st);
        }
    }
    return launch_gp_filt_k<NBLK, DK, -1>(a, st);
}

template <int NBLK>
int launch_gp_filt_n(int DK, const GpFiltArgs& a, hipStream_t st)
{
    switch (DK) {
        case 2: return launch_gp_filt_t<NBLK, 2>(a, st);
        case 4: return launch_gp_filt_t<NBLK, 4>(a, st);
        case 6: return launch_gp_filt_t<NBLK, 6>(a, st);
    }
    return -2;
}

template <int NBLK, int DK>
int launch_gp_filt_bwd_k(const GpFiltBwdArgs& a, hipStream_t st)
{
    typedef GpBwdCfg<NBLK> C;
    const size_t lds = size_t(GpFiltBwdGeom<NBLK, DK>::LDS_DOUBLES) * sizeof(double);
    auto k = gp_filter_bwd_kernel<NBLK, C::RB, DK, C::STASH>;
    int rc = set_lds(k, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k, dim3(unsigned((a.N + 15) / 16)), dim3(64 * C::W), lds, st, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -int(e) - 1000;
}

template <int NBLK>
int launch_gp_filt_bwd_n(int DK, const GpFiltBwdArgs& a, hipStream_t st)
{
    switch (DK) {
        case 2: return launch_gp_filt_bwd_k<NBLK, 2>(a, st);
        case 4: return launch_gp_filt_bwd_k<NBLK, 4>(a, st);
        case 6: return launch_gp_filt_bwd_k<NBLK, 6>(a, st);
    }
    return -2;
}

}  // namespace cbfssm

#define CBF_GPFILT_DECLARE(NB)                                                                   \
    namespace cbfssm {                                                                           \
    int launch_gp_filt_nb##NB(int DK, const GpFiltArgs& a, hipStream_t st);                      \
    int launch_gp_filt_bwd_nb##NB(int DK, const GpFiltBwdArgs& a, hipStream_t st);               \
    }

#define CBF_GPFILT_INSTANTIATE(NB)                                                               \
    namespace cbfssm {                                                                           \
    int launch_gp_filt_nb##NB(int DK, const GpFiltArgs& a, hipStream_t st)                       \
    {                                                                                            \
        return launch_gp_filt_n<NB>(DK, a, st);                                            \
    }                                                                                            \
    int launch_gp_filt_bwd_nb##NB(int DK, const GpFiltBwdArgs& a, hipStream_t st)                \
    {                                                                                            \
        return launch_gp_filt_bwd_n<NB>(DK, a, st);                                              \
    }                                                                                            \
    }
