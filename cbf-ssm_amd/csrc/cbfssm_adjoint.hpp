// Reverse-mode (adjoint) time-loop kernels of the CBF-SSM ELBO: what tf.train.AdamOptimizer.minimize differentiates
// through the two tf.while_loops (cbfssm/model/cbfssm.py:107-111,176-179,273-275), re-derived by hand.
//
// One workgroup owns 16 chains and walks the recurrence backwards from the saved trajectory (x_t or h_t).  Of the
// forward evaluation it reads the per-step (fmean, fvar) and, when they were kept, the A2 = K^-1 K tiles; the kernel
// tile K = k(Z, x_t) is recomputed (and A2 too when no tiles were kept: phase C).  Per step, between four workgroup
// barriers:
//
//   B   K tile of this wave's rows (MFMA + exp) -> LDS;           (the next step's inputs are loaded meanwhile)
//   E   A2bar = mu Fm + 2 A2 o (s2 Fv) - K o colsum(Fv)                                                  MFMA
//       mubar += A2 Fm^T,  s2bar += (A2 o A2) Fv^T,  Kinvbar += A2bar K^T      (k-dim = the 16 chains)    MFMA
//   F   Kbar = Kinv A2bar - A2 o colsum(Fv);  Ebar = Kbar o K                                            MFMA
//       xbar~ = Z~^T Ebar - x~ o colsum(Ebar),  Zbar~ += Ebar x~^T                                       MFMA
//       (two 16-row input blocks, D = 9 .. 24: only block 0 -- it holds every state row -- goes through the MFMAs; colsum(Ebar)
//        is summed in the lanes, the lengthscale adjoint of the rows j >= 16 follows from Zbar~ after the time loop)
//   G   carry d loss/d x_t (or d loss/d h_t) to the next reverse step, then in the same lanes
//   D   per-(chain, dim) adjoint of the NEXT step's epilogue -> Fm = d loss/d fmean, Fv = d loss/d fvar  (16 x 16 each)
//
// The eight-wave tile (seven row blocks, K^-1 adjoint in registers: M = 65 .. 112) lays the end of the step out differently.
// Nothing in the recurrence reads Zbar~, and phases G / D are vector latency on the waves 0 .. 3 with the matrix units of the
// other SIMDs idle.  So phase F ends with xbar~ -> the partial tiles and Ebar -> the wave's own rows of the K tile (dead
// since phase E), and Zbar~ += Ebar x~^T runs BEHIND the barrier that releases phase G, in the waves 4 .. 6 and the eighth
// wave, for all seven row blocks by a compile-time deal (rev_zdeal); the body is instantiated per wave role (rev_body).
//
// Parameter adjoints accumulate in VGPRs over the whole pass and leave the kernel once, as one partial slab per
// workgroup (summed in a fixed order by reduce_partials_kernel: bitwise reproducible, no atomics).
#pragma once
#include "cbfssm_kernels.hpp"

namespace cbfssm {

struct RevPackPtrs {
    const double* muB;   // [NBLK][4][64]   A[row m][k = d]
    const double* s2B;
    const double* ZT;    // [NBLK][JB][4][64]  A[row j][k = m], row D is all ones (for m < M)
};

// Backward-run adjoint: the chunk table of one launch.  Entry e (grid.y, in launch order) is nsteps[e] consecutive steps
// from t_begin[e] upwards of run[e]: whole resample-to-resample segments, so every entry is an independent workgroup set
// with its own slab.  Filled on the host (cbfssm_bwd_schedule, or the explicit segment ranges of stash mode).
constexpr int BWD_SCHED_CAP = 32;
struct BwdSched {
    int run[BWD_SCHED_CAP];
    int t_begin[BWD_SCHED_CAP];
    int nsteps[BWD_SCHED_CAP];
};

struct RevArgs {
    PackPtrs pk;
    RevPackPtrs rk;
    int N, S, T, B;
    int dim_x, dim_u, dim_y;
    int Do, D;
    int recog_len, condition;
    double k_factor;
    double cL;             // lambda0 / S : weight of (kl_x - loglik) in the loss      (cbfssm.py:257-262)
    double cE;             // lambda1 / S : weight of -entropy
    const double* var_x;
    const double* var_y;
    const double* u;
    const double* y;
    const double* eps;     // fwd: (T-1,N); bwd: (2,T,N)
    const double* hid;     // bwd: (2,T,N)
    const double* x;       // fwd: (T,N,dim_x) saved trajectory
    const double* y2;      // fwd: (T,N,dob)
    const double* h_all;   // bwd: (2,T,N,dob) saved outputs of both runs
    double* gy2;           // (T,N,dob): written by the fwd reverse, read by the bwd reverse
    double* gpart;         // [workgroup][slab]
    int64_t slab;          // doubles per workgroup
    int KSr;               // ceil(M / 4)
    // time range of this launch
    int t_hi, t_lo;        // fwd: steps t = t_hi .. t_lo (descending), t_hi <= T-2
    BwdSched sched;        // bwd: the chunk of every grid.y index
    double* gx_carry;      // fwd: (N, dim_x) adjoint of x_{t_lo} handed to the next launch (null: single launch)
    // stash mode (tile heights whose K^-1-adjoint does not fit the VGPR file): the A2bar^T and K^T operand images of
    // every step go to HBM, [slot = workgroup * chunk_steps + step][NBLK][4][64] doubles each (stash_ld = 16 x slots);
    // cbfssm_stash_contract_f64 contracts them after the launch
    double* stash_a;
    double* stash_k;
    int64_t stash_ld;
    int chunk_steps;
    int half;              // CBFSSMHALF forward pass
    double* gx0;           // half: (N, dim_x) d loss / d x_0 per chain (summed over the particles by the caller)
    int group0, gtotal;    // this launch covers chain groups [group0, group0 + gridDim.x) of gtotal
    const double* a2s;     // optional: A2 = K^-1 k tiles of every step as saved by the forward evaluation
                           // (PassArgs::a2s layout); NULL -> phase C recomputes them
    const double* fmv;     // (fmean, fvar) of every step as saved by the forward evaluation (PassArgs::fmv layout)
    int ksave;             // 1: every saved record is [A2 tile][kernel tile] (PassArgs::ksave)
    int M;                 // inducing points (rows m >= M of the tiles are padding)
    // input gradients (the IG instantiations only): per step and chain, written once by the workgroup that owns them
    double* gin;           // fwd: (T-1, dim_u, N), bwd: (2, T, dim_u+dim_y, N): adjoint of the scaled data rows x~[j] of the GP input
    double* gyo;           // fwd: (T, dim_y, N): adjoint of the observed dimensions of y_tilde (row 0: of x_0)
};

// slab layout (doubles), all in MFMA C-layout [r][lane] blocks of 256
template <int NBLK, int JB, bool STASH>
struct Slab {
    static constexpr int gMu = 0;                                         // [NBLK][256]
    static constexpr int gS2 = gMu + NBLK * 256;                          // [NBLK][256]
    static constexpr int gB = gS2 + NBLK * 256;                           // [NBLK][NBLK][256]  (absent in stash mode)
    static constexpr int gZ = gB + (STASH ? 0 : NBLK * NBLK * 256);       // [NBLK][JB][256]
    static constexpr int small = gZ + NBLK * JB * 256;   // [0,16) gvx, [16,32) gvy, [32,32+16*JB) glx, 96 gsig, 97 glogsig
    static constexpr int total = small + 192;            // [100,192): diagnostic stamps (CBF_REV_STAMPS builds only)
};


// Input-adjoint geometry.  The D inputs plus the ones row fill JB 16-row blocks.  With two blocks (four or six k-steps of
// the input dimension: D = 9 .. 24, the state dimension is at most 16) every state row sits in block 0 and the recurrence needs nothing else from the product xbar~ = (Z~)^T Ebar, so only JX = 1
// block of it is computed per step:
//   - colsum(Ebar) (the ones row, wherever it sits) is summed in the lanes: 16 doubles per wave in an LDS area of their own;
//   - the lengthscale adjoint of the rows j >= 16, sum_{t,n} xbar~[j,n] x~[j,n], is
//         sum_m z~[m,j] Zbar~[m][j]  -  sum_{t,n} colsum(Ebar)[n] x~[j,n]^2
//     with Zbar~ the accumulator the kernel keeps anyway; the second sum is one fused multiply-add per step and lane.
// A wave's slot of the partial tiles: JX blocks of 256, and at least the 16 x 17 transpose scratch the eight-wave tiles
// put there (272 doubles).
// IG (input gradients: d loss / d u and d loss / d y are wanted): the data rows j >= 16 are an output of every step, so both
// blocks go through the MFMAs again -- the general JX = JB path, on the chain.
template <int DK, bool IG = false>
struct RevInGeom {
    static constexpr int JB = (4 * DK + 1 + 15) / 16;
    static constexpr bool SPLITJ = (JB == 2) && !IG;
    static constexpr int JX = SPLITJ ? 1 : JB;
    static constexpr int PSL = SPLITJ ? 272 : (JB > 2 ? JB : 2) * 256;
    static constexpr int ECS = SPLITJ ? 16 : 0;                         // column sums of Ebar: doubles per wave
};

// Sum of a double over the four 16-lane groups of a wave (lanes nl, nl + 16, nl + 32, nl + 48), in every lane.  The gfx950
// lane swaps exchange the odd 16-lane rows of the first operand with the even rows of the second (permlane16) and the upper
// half of the first with the lower half of the second (permlane32): with both operands the same value, the two results
// are the two addends.  Vector ALU only -- an LDS permute would be two round trips here.
__device__ __forceinline__ double rowgroup_sum(double x)
{
    typedef unsigned int u2 __attribute__((ext_vector_type(2)));
    unsigned lo = __double2loint(x), hi = __double2hiint(x);
    u2 pl = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    u2 ph = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    const double y = __hiloint2double(ph[0], pl[0]) + __hiloint2double(ph[1], pl[1]);
    lo = __double2loint(y); hi = __double2hiint(y);
    pl = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    ph = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    return __hiloint2double(ph[0], pl[0]) + __hiloint2double(ph[1], pl[1]);
}

// LDS budget of one adjoint workgroup (doubles).  Stash-mode tiles re-read the Z~ operand images every step instead of
// holding them in registers; when the K^-1 image does not fit anyway, the LDS left over holds those images (a read
// that misses L1 costs an L2 round trip right in front of the MFMAs that need it).
template <int NBLK, int RB, int DK, bool STASH, bool IG = false>
struct RevLds {
    static constexpr int W = (NBLK + RB - 1) / RB;
    static constexpr int JB = (4 * DK + 1 + 15) / 16;
    static constexpr int JX = RevInGeom<DK, IG>::JX;
    static constexpr int PSL = RevInGeom<DK, IG>::PSL;
    static constexpr int ECS = W * RevInGeom<DK, IG>::ECS;
    static constexpr int BASE_PLAIN = 2 * 4 * DK * 17 + 2 * (16 * NBLK) * 17 + 2 * 16 * 17 + W * PSL + 64 + ECS;
    // Stash-mode tiles that stream K^-1: the per-wave partial tiles of the input adjoint (`part`, written at the end of
    // phase F, read in phase G) live in the K tile's LDS, which is dead by then -- one more workgroup barrier per step
    // buys W x PSL doubles (28 KB at NBLK = 13) for the operand images below.
    static constexpr bool PALIAS = STASH;
    static constexpr int KTR = PALIAS ? ((16 * NBLK) * 17 > W * PSL ? (16 * NBLK) * 17 : W * PSL) : (16 * NBLK) * 17;
    static constexpr int BASE = PALIAS ? 2 * 4 * DK * 17 + KTR + (16 * NBLK) * 17 + 2 * 16 * 17 + 64 + ECS : BASE_PLAIN;
    static constexpr int LIMIT = 163840 / 8;
    static constexpr int ZP = NBLK * DK * 64 + 16 * NBLK;          // Z~ A-operand image + row constants
    static constexpr int ZT = NBLK * JX * 256;                     // (Z~)^T A-operand image (the blocks phase F multiplies)
    static constexpr int MU = NBLK * 256;                          // mu_z B-operand image (phase E)
    // filled in this order (measured at NBLK = 13 / D = 21, where only part fits: {(Z~)^T} and {Z~, mu} are within 1 %)
    static constexpr bool ZTLDS = STASH && (BASE + ZT <= LIMIT);
    static constexpr bool ZLDS = STASH && (BASE + ZP + (ZTLDS ? ZT : 0) <= LIMIT);
    static constexpr bool MULDS = ZLDS && (BASE + ZP + (ZTLDS ? ZT : 0) + MU <= LIMIT);
    static constexpr int EXTRA = (ZLDS ? ZP : 0) + (ZTLDS ? ZT : 0) + (MULDS ? MU : 0);   // variants without the K^-1 image
};

// BLDS: the K^-1 A-operand image lives in LDS for the whole pass (one copy per workgroup, trimmed to the ceil(M/4)
// k-steps that carry data); otherwise it streams from L2.  RB: 16-row blocks of inducing points per wave.
// Seven row-block waves load the four SIMDs 2-2-2-1.  The in-register tiles of that height get an EIGHTH wave, which
// lands next to wave 3 and takes the last REV_XCB column blocks of the Kinvbar accumulation for ALL row blocks (its
// operands, A2bar and K, are complete in the LDS tiles between the barriers that end phases E and F); it has no other
// role and leaves before the epilogue (a wave that has ended no longer counts at s_barrier).
// Measured on the C3 kernels (ms, forward-pass / backward-run adjoint; without the wave 5.12 / 5.83):
//   1 block 5.14 / 5.59, 2 blocks 4.89 / 5.60, 3 blocks 4.81 / 5.72, 4 blocks 5.11 / 6.01 (the extra wave's 112 MFMAs
//   no longer fit into phase F next to wave 3's own); with the operand loads of phases E and F issued early (below):
//   2 blocks 4.68 / 5.54, 3 blocks 4.30 / 5.40, 4 blocks 4.66 / -.
#ifndef CBF_REV_XCB
#define CBF_REV_XCB 3
#endif
constexpr int REV_XCB = CBF_REV_XCB;
// ... and it STARTS EARLY.  Its operands of row block rb exist as soon as that row block's wave has written its A2bar rows,
// a quarter into phase E -- not only after the barrier that ends E.  Measured per wave (profiles/r02/
// adjoint_phase_shares_per_wave.log): with the whole of its 84 MFMAs between the barriers of phase F, wave 3's SIMD carries
// 41 + 84 MFMAs there against 82 on the others (phase F 41 % of a step on wave 3, 33-35 % elsewhere, everybody waiting
// for it) and idles half of phase E (wave 3 waits 9-11 % there).  So the row-block waves raise an LDS flag per row block
// (flag_release / flag_wait, cbfssm_kernels.hpp) and the extra wave takes the first REV_XEARLY row blocks before that
// barrier, the rest after it.
#ifndef CBF_REV_XEARLY
#define CBF_REV_XEARLY 3
#endif
constexpr int REV_XEARLY = CBF_REV_XEARLY;
// Two of them behind barrier 5 since the row-block waves have no Zbar~ in phase F (below): their phase F is eight MFMAs
// shorter, and with one late block this wave's share of it was what everybody waited for at barrier 5.  C3 train step (ms) with
// 0 / 1 / 2 / 3 / 4 late blocks: 10.22 / 10.02 / 9.79 / 9.88 / 10.44 (profiles/zbar_window/deal_variants.txt).
#ifndef CBF_REV_XLATE
#define CBF_REV_XLATE 2
#endif
constexpr int REV_XLATE = CBF_REV_XLATE;      // row blocks the extra wave takes behind barrier 5 (see the kernel)
// THE Zbar~ DEAL of the eight-wave tiles.  Nothing in the recurrence reads Zbar~ += Ebar x~^T, so it does not run in phase F,
// in front of the barrier the carry chain (phases G / D, vector latency on waves 0-3) waits at: every row-block wave
// leaves its rows of Ebar in its own rows of the K tile, and behind barrier 5 the waves that have nothing to carry
// accumulate Zbar~ for everybody.  rev_zdeal(rb): the wave that owns the Zbar~ accumulator of row block rb (7: the eighth
// wave); a wave's blocks are taken in ascending order.  CBF_REV_ZDEAL picks the table (1: measured, not kept -- DESIGN 6.ZW).
#ifndef CBF_REV_ZDEAL
#define CBF_REV_ZDEAL 0
#endif
constexpr int REV_ZW0 = 4;                    // first row-block wave that takes part in the deal (waves 0-3 carry phase D)
constexpr int ROLE_ALL = 0, ROLE_CARRY = 1, ROLE_DEAL = 2, ROLE_XTRA = 3;   // wave roles of the kernel body (see rev_body)
constexpr int rev_zdeal(int rb)
{
#if CBF_REV_ZDEAL == 1
    constexpr int owner[7] = {4, 5, 6, 7, 4, 5, 7};      // the eighth wave takes two, wave 6 (two row groups in phase G) one
#else
    constexpr int owner[7] = {4, 5, 6, 7, 4, 5, 6};
#endif
    return owner[rb];
}
constexpr int rev_zcount(int wv)              // row blocks dealt to wave wv
{
    int n = 0;
    for (int rb = 0; rb < 7; ++rb) n += (rev_zdeal(rb) == wv) ? 1 : 0;
    return n;
}
constexpr int rev_zblock(int wv, int k)       // the k-th of them (7: none)
{
    for (int rb = 0; rb < 7; ++rb)
        if (rev_zdeal(rb) == wv && k-- == 0) return rb;
    return 7;
}
constexpr int rev_zmax(int w0, int w1)        // most row blocks of any wave w0 <= wv <= w1
{
    int n = 0;
    for (int wv = w0; wv <= w1; ++wv) n = rev_zcount(wv) > n ? rev_zcount(wv) : n;
    return n;
}
#ifdef CBF_NO_XW          // diagnostic builds: the seven-wave form
constexpr bool rev_extra_wave(int, bool) { return false; }
#else
// Stash-mode tiles get an extra wave too, with another job: it is the STASH WRITER.  It copies the two operand images of every
// step (K^T right after barrier 1, A2bar^T after barrier 4) from the LDS tiles to HBM, so that the row-block waves issue
// no global stores inside the time loop: vmcnt retires in order and counts stores, and at 256 VGPRs with two row blocks per
// wave these kernels reload spilled registers all through a step -- every such reload was an `s_waitcnt vmcnt(0)` that also
// waited for the step's stash stores to reach HBM (isa_wait_audit.py: `vmcnt(1): waits for 9 [WWWWWWWWS]`).  It lands on
// the SIMD that carries the fewest row blocks.  C4 adjoints 9.80 / 13.78 -> 9.58 / 13.34 ms, train step 38.9 -> 38.0 ms.
// Not at 16 row blocks: eight waves would become nine and the three-wave SIMD would cap everybody at 168 VGPRs.
// (Measured and NOT kept, round 3: the same wave also taking over Zbar~ += Ebar x~^T for all row blocks through an Ebar
// tile in LDS -- the row-block waves shed 32 accumulator VGPRs (spill slots 64 -> 48 / 34 -> 12) and 16 MFMAs per step, the
// kernels did not move: 9.68 / 13.35 ms.  And kernel tiles kept by the forward evaluation for these tile heights, read back
// instead of rebuilt: 10.9 / 15.9 ms loaded at the step top, 11.1 / 15.9 ms prefetched a step ahead -- slower both ways.)
#ifdef CBF_REV_RB13
constexpr bool rev_extra_wave(int nblk, bool stash) { return stash ? (nblk != 16 && nblk != 13) : (nblk == 7); }
#else
constexpr bool rev_extra_wave(int nblk, bool stash) { return stash ? (nblk != 16) : (nblk == 7); }
#endif
#endif

// KD: k-steps of the products whose k index is the GP output dimension (mu Fm, s2 Fv): 4 in general, 2 when the launcher
// knows Do <= 8 (the backward runs of the Sarcos class: dim_x - dim_y = 7) -- the other two would multiply zeros.
// KSV: the forward evaluation kept the kernel tile of every step next to its A2 tile (RevArgs::ksave, non-stash tiles):
// phase B is a copy -- registers that were loaded a step ahead go to the LDS tile -- instead of 6 MFMAs and four
// exponentials per lane, and the Z~ rows / row constants of the wave are not held at all.
// IG: the launch also writes, per step and chain, the adjoint of the data rows of the GP input (RevArgs::gin) and, in the
// forward-pass adjoint, of the observed dimensions of y_tilde (RevArgs::gyo): what tf.gradients(loss, sample_in / sample_out)
// needs of the time loops.  Off: the code below is the code without the switch.
// ROLE: the kernel body, once per WAVE ROLE (rev_kernel below picks it, wave-uniformly).  The eight-wave tiles run at the
// register cap: the waves 0 .. 3 (ROLE_CARRY) hold the phase D / G lane state and no Zbar~ accumulator, the waves 4 .. 6
// (ROLE_DEAL) two row blocks of Zbar~ accumulators and no lane state, the eighth wave (ROLE_XTRA) its own loop.  One body
// for all would hold the union in every wave (measured on the two C3 kernels: 80 and 28 B of scratch per lane against the
// 44 and 0 of the form without the deal), so it is instantiated per role, as sym_run<WV> in cbfssm_contract.hip.
// ROLE_ALL: every other tile -- the one body it always was, and still INSIDE the kernel: the body is text
// (cbfssm_adjoint_body.inc) that the role function and the kernel both include, because the same text called as an
// inlined function is allocated and scheduled differently by the compiler (measured: C4 train step +1.7 %).
template <int NBLK, int RB, int DK, bool BLDS, bool STASH, int MODE, int KD, bool KSV, bool IG, int ROLE>
__device__ __forceinline__ void rev_body(const RevArgs& a)
{
#include "cbfssm_adjoint_body.inc"
}

template <int NBLK, int RB, int DK, bool BLDS, bool STASH, int MODE, int KD = 4, bool KSV = false, bool IG = false>
__global__ __launch_bounds__(64 * ((NBLK + RB - 1) / RB + (rev_extra_wave(NBLK, STASH) ? 1 : 0))) void rev_kernel(RevArgs a)
{
    if constexpr (rev_extra_wave(NBLK, STASH) && !STASH) {
        // (every role runs the same sequence of workgroup barriers)
        const int wu = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
        if (wu == (NBLK + RB - 1) / RB) rev_body<NBLK, RB, DK, BLDS, STASH, MODE, KD, KSV, IG, ROLE_XTRA>(a);
        else if (wu < REV_ZW0) rev_body<NBLK, RB, DK, BLDS, STASH, MODE, KD, KSV, IG, ROLE_CARRY>(a);
        else rev_body<NBLK, RB, DK, BLDS, STASH, MODE, KD, KSV, IG, ROLE_DEAL>(a);
    } else {
        constexpr int ROLE = ROLE_ALL;
#include "cbfssm_adjoint_body.inc"
    }
}

}  // namespace cbfssm
