// Fused time loop of ONE sparse GP and its adjoint: the recurrence
//     h <- h + fmean(h, a_t) + eps_t sqrt(fvar(h, a_t) + var_add)
// over T steps for N independent chains with PER-CHAIN auxiliary inputs a (T, N, Da), from a per-chain h0.  Two things
// in the reference have this shape: Voliro's recognition run (cbfssm/model/voliro.py:139-186: one run from h = 0,
// backwards in time, GP input (h, u_t, y_t) with a per-particle u_t) and the free-running transition of a trained
// CBF-SSM (cbfssm/model/cbfssm.py:199-206,224).  The pass kernels (cbfssm_kernels.hpp) cannot take per-chain inputs:
// their u / y are shared by the particles of a sequence.
//
// gp_rollout_kernel: one workgroup per 16 chains, the time loop inside.  A step is the body of predict_kernel
// (Tile::phase1, phase2 / phase2_tri, gather) and an epilogue per (chain, state dim) lane that writes the next GP input
// straight into the LDS operand tile.  entropy = 0.5 sum log(2 pi e v) leaves as one partial per workgroup (LogProd: one
// log per lane and pass).
//
// gp_rollout_bwd_kernel: the algebra of gp_predict_bwd_kernel (cbfssm_gp_bwd.hpp, phases B to G) with the column block
// fixed per workgroup and the loop running over the steps in reverse order of the forward.  Per step the GP input is
// rebuilt from the saved trajectory (the previous row of traj, h0 at the first step), the upstream adjoints are formed in
// the kernel from g = gtraj[t] + carry:
//     Fm = g,   Fv = g eps / (2 sqrt v) + g_ent / (2 v)
// and after phase G the state rows of gX plus g become the next carry (h enters the step directly and through the GP);
// the rows j >= Do leave as ga[t].  The parameter adjoints stay in VGPRs for the whole pass and leave once per
// workgroup in the Slab<> layout; sum Fv per state dim goes to the slab's d/d var_x entries (d loss / d var_add).
// Tile heights above seven row blocks write the stash operand images per (workgroup, step) slot.
// Phases B to F, the row-block setup and the slab write are the shared body of cbfssm_gp_tile.hpp (GpWave), the same calls
// as in the batch kernel; what loads the tiles, the stash slot index, phase G and the carry are this kernel's own.
// No atomics, one writer per output: two calls are bitwise identical.  Padded chains carry zero adjoints and the rows
// m >= M of the tiles are zero, so both contribute exactly zero.
#pragma once
#include "cbfssm_gp_bwd.hpp"

namespace cbfssm {

struct GpRollArgs {
    PackPtrs pk;
    const double* h0;        // (N, Do)
    const double* a;         // (T, N, Da), Da = D - Do (unused when Da = 0)
    const double* eps;       // (T, N)
    const double* var_add;   // (Do) or null
    double* traj;            // (T, N, Do)
    double* vsave;           // (T, N, Do) or null: v = fvar + var_add of every step, kept for the adjoint
    double* ent_part;        // one partial per workgroup
    int N, T, D, Do, reverse;
    int tri;
};

struct GpRollBwdArgs {
    PackPtrs pk;
    RevPackPtrs rk;
    const double* h0;
    const double* a;
    const double* eps;
    const double* traj;
    const double* vsave;
    const double* gtraj;     // (T, N, Do): d loss / d traj
    const double* g_ent;     // one double on the device: d loss / d entropy
    double* gh0;             // (N, Do)
    double* ga;              // (T, N, Da)
    double* gpart;           // [workgroup][slab]
    int64_t slab;
    double* stash_a;         // stash tile heights: [workgroup * T + step][NBLK][4][64] operand images (A2bar^T, K^T)
    double* stash_k;
    int N, T, M, D, Do, reverse;
};

template <int NBLK, int RB, int DK, bool BREG, bool TRI, int KT>
__global__ __launch_bounds__(64 * ((NBLK + RB - 1) / RB)) void gp_rollout_kernel(GpRollArgs a)
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

    TT tile;
    tile.load_operands(a.pk, w, l);

    // per-lane constants of the epilogue tasks of this wave: state-row group q = w + qi W < 4, row d = 4 q + g, chain nl
    double va[QPW], il[QPW], hcur[QPW];
    LogProd lp[QPW];
    bool act[QPW];
    const int c = min(c0 + nl, N - 1);
    const bool cval = (c0 + nl) < N;
#pragma unroll
    for (int qi = 0; qi < QPW; ++qi) {
        const int q = w + qi * W;
        const int d = 4 * q + g;
        act[qi] = (q < 4) && (d < Do);
        const int dc = act[qi] ? d : 0;
        va[qi] = a.var_add ? a.var_add[dc] : 0.0;
        il[qi] = a.pk.invl[dc];
        hcur[qi] = a.h0[int64_t(c) * Do + dc];
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

        // this step's noise and the next step's auxiliary rows, issued ahead of the tile work
        double eps_t[QPW], auxr[AUXR];
#pragma unroll
        for (int qi = 0; qi < QPW; ++qi) eps_t[qi] = a.eps[int64_t(t) * N + c];
#pragma unroll
        for (int k2 = 0; k2 < AUXR; ++k2) {
            const int i = tid + k2 * NT;
            auxr[k2] = (has_next && i < 16 * naux) ? auxp[k2][int64_t(tn) * auxs] : 0.0;
        }

        double kr[RB][4];
        tile.phase1(xq, Kt, kr, w, l);
        // (the loads above land here, a phase after they were issued: see pass_kernel)
#pragma unroll
        for (int qi = 0; qi < QPW; ++qi) asm volatile("" : "+v"(eps_t[qi]));
#pragma unroll
        for (int k2 = 0; k2 < AUXR; ++k2) asm volatile("" : "+v"(auxr[k2]));
        __syncthreads();
        if constexpr (TRI) tile.phase2_tri(Kt, At, flag, step + 1, part, w, l, nullptr);
        else tile.phase2(Kt, part, kr, w, l, nullptr);
        __syncthreads();                             // part complete; xq and Kt free

        // ---- step epilogue
#pragma unroll
        for (int qi = 0; qi < QPW; ++qi) {
            const int q = w + qi * W;
            if (q < 4) {
                double fm, fv;
                tile.gather(part, q, l, fm, fv);
                if (act[qi]) {
                    const int d = 4 * q + g;
                    const double v = fv + va[qi];
                    const double hn = hcur[qi] + fm + eps_t[qi] * (v * fast_rsqrt(v));
                    hcur[qi] = hn;
                    if (cval) {
                        const int64_t o = (int64_t(t) * N + c) * Do + d;
                        a.traj[o] = hn;
                        if (a.vsave) a.vsave[o] = v;
                        lp[qi].mul(v);
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

    // ---- entropy partial of this workgroup: 0.5 sum (log(2 pi e) + log v)
    double v = 0.0;
#pragma unroll
    for (int qi = 0; qi < QPW; ++qi)
        if (act[qi] && cval) v += 0.5 * (double(T) * 2.8378770664093453391 + lp[qi].log());
    double tot = block_sum(v, red, tid, NT);
    if constexpr (TRI) {
        if (tid == 0 && flag[CBF_FLAG_TIMEOUT_SLOT] != 0) tot = __builtin_nan("");   // a hand-off poll ran out (see flag_wait)
    }
    if (tid == 0) a.ent_part[blockIdx.x] = tot;
}

// LDS of the adjoint: the tiles of gp_predict_bwd_kernel plus the carry tile
template <int NBLK, int DK>
struct GpRollBwdGeom {
    static constexpr int PD = 17;
    static constexpr int LDS_DOUBLES = GpBwdGeom<NBLK, DK>::LDS_DOUBLES + 16 * PD;
    static_assert(LDS_DOUBLES <= 163840 / 8, "LDS budget");
};

template <int NBLK, int RB, int DK, bool STASH>
__global__ __launch_bounds__(64 * ((NBLK + RB - 1) / RB)) void gp_rollout_bwd_kernel(GpRollBwdArgs a)
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
    const double gent = a.g_ent[0];

    WV wv;
    wv.setup(a.pk, tid);

    // ---- accumulators of the parameter adjoints (all steps of this workgroup)
    GpAdjAcc<NBLK, RB, JB, STASH> acc;
    acc.zero();
    double glx[GPW];
#pragma unroll
    for (int k2 = 0; k2 < GPW; ++k2) glx[k2] = 0.0;
    double gsig = 0.0, glogsig = 0.0;
    double gva = 0.0;                                   // sum of Fv over this thread's (chain, dim = tid & 15) entries
    double ilg[GPW];
#pragma unroll
    for (int k2 = 0; k2 < GPW; ++k2) {
        const int j = 4 * (w + k2 * W) + g;
        ilg[k2] = (j < D) ? a.pk.invl[j] : 0.0;
    }
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
                const double rs = fast_rsqrt(a.vsave[o]);
                vm = gb;
                vv = 0.5 * rs * (gb * a.eps[int64_t(t) * N + p] + gent * rs);   // d sqrt(v) = 1 / (2 sqrt v), d log v = 1 / v
            }
            Fm[d * PD + n] = vm;
            Fv[d * PD + n] = vv;
            gva += vv;
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

        // ---- G: input adjoint of this step: state rows -> carry (gh0 at the first forward step), the others -> ga[t]
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
                            const double cv = gx + Fm[j * PD + nl];                // h enters h' directly and through the GP
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
    const double gv[1] = {gva};                         // d loss / d var_add by state dim
    wv.template write_state_sums<STASH>(slab, part, gv);
    wv.template write_sums<STASH>(slab, glx, gsig, glogsig, red);
}

// ---- launchers: K^-1 placement (registers up to seven row blocks, streamed above), two row blocks per wave from 13 row
// blocks and the compile-time trim of the seven-block tile follow the predict dispatcher (cbfssm_inst.hpp)
template <int NBLK, int DK, int KT>
int launch_gp_roll_k(const GpRollArgs& a, hipStream_t st)
{
    typedef Cfg<NBLK> C;
    const unsigned groups = unsigned((a.N + 15) / 16);
    if (a.tri) {
        typedef Tile<NBLK, C::RB, DK, C::BREG, true, KT> TT;
        const size_t lds = TT::LDS_DOUBLES * sizeof(double);
        auto k = gp_rollout_kernel<NBLK, C::RB, DK, C::BREG, true, KT>;
        int rc = set_lds(k, lds);
        if (rc) return rc;
        hipLaunchKernelGGL(k, dim3(groups), dim3(TT::NT), lds, st, a);
    } else {
        typedef Tile<NBLK, C::RB, DK, C::BREG, false, KT> TT;
        const size_t lds = TT::LDS_DOUBLES * sizeof(double);
        auto k = gp_rollout_kernel<NBLK, C::RB, DK, C::BREG, false, KT>;
        int rc = set_lds(k, lds);
        if (rc) return rc;
        hipLaunchKernelGGL(k, dim3(groups), dim3(TT::NT), lds, st, a);
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -int(e) - 1000;
}

template <int NBLK, int DK>
int launch_gp_roll_t(const GpRollArgs& a, hipStream_t st)
{
    if constexpr (trim_tiles<NBLK>()) {
        switch (4 * NBLK - a.pk.KSr) {
            case 0: return launch_gp_roll_k<NBLK, DK, 0>(a, st);
            case 1: return launch_gp_roll_k<NBLK, DK, 1>(a, st);
            case 2: return launch_gp_roll_k<NBLK, DK, 2>(a, st);
            case 3: return launch_gp_roll_k<NBLK, DK, 3>(a, st);
        }
    }
    return launch_gp_roll_k<NBLK, DK, -1>(a, st);
}

template <int NBLK>
int launch_gp_roll_n(int DK, const GpRollArgs& a, hipStream_t st)
{
    switch (DK) {
        case 2: return launch_gp_roll_t<NBLK, 2>(a, st);
        case 4: return launch_gp_roll_t<NBLK, 4>(a, st);
        case 6: return launch_gp_roll_t<NBLK, 6>(a, st);
    }
    return -2;
}

template <int NBLK, int DK>
int launch_gp_roll_bwd_k(const GpRollBwdArgs& a, hipStream_t st)
{
    typedef GpBwdCfg<NBLK> C;
    const size_t lds = size_t(GpRollBwdGeom<NBLK, DK>::LDS_DOUBLES) * sizeof(double);
    auto k = gp_rollout_bwd_kernel<NBLK, C::RB, DK, C::STASH>;
    int rc = set_lds(k, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k, dim3(unsigned((a.N + 15) / 16)), dim3(64 * C::W), lds, st, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -int(e) - 1000;
}

template <int NBLK>
int launch_gp_roll_bwd_n(int DK, const GpRollBwdArgs& a, hipStream_t st)
{
    switch (DK) {
        case 2: return launch_gp_roll_bwd_k<NBLK, 2>(a, st);
        case 4: return launch_gp_roll_bwd_k<NBLK, 4>(a, st);
        case 6: return launch_gp_roll_bwd_k<NBLK, 6>(a, st);
    }
    return -2;
}

}  // namespace cbfssm

#define CBF_GPROLL_DECLARE(NB)                                                                   \
    namespace cbfssm {                                                                           \
    int launch_gp_roll_nb##NB(int DK, const GpRollArgs& a, hipStream_t st);                      \
    int launch_gp_roll_bwd_nb##NB(int DK, const GpRollBwdArgs& a, hipStream_t st);               \
    }

#define CBF_GPROLL_INSTANTIATE(NB)                                                               \
    namespace cbfssm {                                                                           \
    int launch_gp_roll_nb##NB(int DK, const GpRollArgs& a, hipStream_t st)                       \
    {                                                                                            \
        return launch_gp_roll_n<NB>(DK, a, st);                                                  \
    }                                                                                            \
    int launch_gp_roll_bwd_nb##NB(int DK, const GpRollBwdArgs& a, hipStream_t st)                \
    {                                                                                            \
        return launch_gp_roll_bwd_n<NB>(DK, a, st);                                              \
    }                                                                                            \
    }
