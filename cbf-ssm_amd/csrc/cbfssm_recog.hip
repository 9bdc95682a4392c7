// Recognition model of the forward-only variants: x_0 = dense(GRU(16)(reversed first recog_len steps of [u, y]))
// (cbfssm/model/cbfssmhalf.py:82-93, cbfssm/model/prssm.py:132-141: tf.contrib.rnn.GRUCell(16) + tf.layers.dense, TF 1.8
// gate layout: [r | u] = sigmoid([x, h] W_g + b_g), c = tanh([x, r o h] W_c + b_c), h' = u o h + (1 - u) o c).
//
// A few hundred FLOPs per sequence and step -- but written with a tensor library it is ~15 launches per GRU step forwards
// and ~35 backwards: 800 launches for recog_len = 16, most of a CBFSSMHALF train step at the small-scale shapes (3.5 ms
// of a 4.1 ms step at the Actuator shape even inside a HIP graph).  Here: ONE wave per sequence walks the recog_len steps,
// forwards (keeping h, r, u, c of every step: 64 doubles) and backwards; the weight gradients leave as one slab per
// sequence and are summed in a fixed order by cbfssm_reduce_partials_f64 (no atomics: reproducible).
//
// Behind the GRU: PR-SSM's other recogniser, conv1d -> max_pool -> dense in float32 (prssm.py:146-157), in the same shape.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cbfssm_hip.h"

namespace cbfssm {

int fail(int rc, const char* fmt, ...);   // cbfssm_api.hip

constexpr int GRU_H = 16;                 // cbfssmhalf.py:84
constexpr int GRU_MAXIN = 32;             // dim_u + dim_y

struct GruArgs {
    int B, T, dim_u, dim_y, dim_x, R;
    const double* u;
    const double* y;
    const double* Wg;     // [n_in + 16][32]
    const double* bg;     // [32]
    const double* Wc;     // [n_in + 16][16]
    const double* bc;     // [16]
    const double* Wd;     // [16][dim_x]
    const double* bd;     // [dim_x]
    double* x0;           // [B][dim_x]
    double* act;          // [B][R][64]: h (before the step), r, u, c     (+ [B][16]: h after the last step, behind it)
    const double* gx0;    // [B][dim_x]   d loss / d x_0
    double* gpart;        // [B][P]       per-sequence gradient slabs, the six tensors behind each other
    int64_t P;
    double* gwin;         // [B][R][n_in] d loss / d window [u, y][:, :R] in sequence time order, or null (weights only)
};

__device__ __forceinline__ double sigm(double x) { return 1.0 / (1.0 + exp(-x)); }

__device__ __forceinline__ double gru_input(const GruArgs& a, int b, int step, int i)
{
    const int t = a.R - 1 - step;                                           // the reversed window (cbfssmhalf.py:86)
    return (i < a.dim_u) ? a.u[(int64_t(b) * a.T + t) * a.dim_u + i] : a.y[(int64_t(b) * a.T + t) * a.dim_y + (i - a.dim_u)];
}

__global__ __launch_bounds__(64) void gru_forward_kernel(GruArgs a)
{
    __shared__ double xs[GRU_MAXIN], hs[GRU_H], rh[GRU_H];
    const int l = threadIdx.x, b = blockIdx.x;
    const int n_in = a.dim_u + a.dim_y;
    double h = 0.0;                                                          // lane j < 16 carries h_j
    if (l < GRU_H) hs[l] = 0.0;
    for (int step = 0; step < a.R; ++step) {
        if (l < n_in) xs[l] = gru_input(a, b, step, l);
        __syncthreads();
        double r = 0.0, z = 0.0;
        if (l < 2 * GRU_H) {                                                 // gate column l: r (l < 16) or u (l >= 16)
            double s = a.bg[l];
            for (int i = 0; i < n_in; ++i) s = fma(xs[i], a.Wg[i * 32 + l], s);
            for (int k = 0; k < GRU_H; ++k) s = fma(hs[k], a.Wg[(n_in + k) * 32 + l], s);
            s = sigm(s);
            if (l < GRU_H) r = s; else z = s;
        }
        z = __shfl(z, (l & 15) + 16);                                        // lane j < 16: r_j and u_j
        if (l < GRU_H) rh[l] = r * h;
        __syncthreads();
        if (l < GRU_H) {
            double s = a.bc[l];
            for (int i = 0; i < n_in; ++i) s = fma(xs[i], a.Wc[i * 16 + l], s);
            for (int k = 0; k < GRU_H; ++k) s = fma(rh[k], a.Wc[(n_in + k) * 16 + l], s);
            const double c = tanh(s);
            if (a.act) {
                double* o = a.act + (int64_t(b) * a.R + step) * 64;
                o[l] = h; o[16 + l] = r; o[32 + l] = z; o[48 + l] = c;
            }
            h = z * h + (1.0 - z) * c;
        }
        __syncthreads();                                                     // xs, hs, rh are rewritten below
        if (l < GRU_H) hs[l] = h;
    }
    __syncthreads();
    if (a.act && l < GRU_H) a.act[int64_t(a.B) * a.R * 64 + int64_t(b) * GRU_H + l] = h;
    if (l < a.dim_x) {
        double s = a.bd[l];
        for (int k = 0; k < GRU_H; ++k) s = fma(hs[k], a.Wd[k * a.dim_x + l], s);
        a.x0[int64_t(b) * a.dim_x + l] = s;
    }
}

// reverse mode through the dense layer and the recog_len GRU steps of one sequence.  IN: also the adjoint of the window
// (GruArgs::gwin) -- a template flag, not a test of the pointer: with the test in the one kernel the default CBFSSMHALF train
// step measured 6 us slower than its parent (profiles/half_input_gradients/), so the weights-only kernel stays the code it was
template <bool IN>
__global__ __launch_bounds__(64) void gru_backward_kernel(GruArgs a)
{
    __shared__ double xs[GRU_MAXIN], hp[GRU_H], rs[GRU_H], dcp[GRU_H], dgp[2 * GRU_H], dhs[GRU_H], gxs[GRU_H];
    const int l = threadIdx.x, b = blockIdx.x;
    const int n_in = a.dim_u + a.dim_y, nrow = n_in + GRU_H;
    double* slab = a.gpart + int64_t(b) * a.P;
    double* gWg = slab;
    double* gbg = gWg + int64_t(nrow) * 32;
    double* gWc = gbg + 32;
    double* gbc = gWc + int64_t(nrow) * 16;
    double* gWd = gbc + 16;
    double* gbd = gWd + int64_t(GRU_H) * a.dim_x;
    // dense layer: x_0 = h_R W_d + b_d
    if (l < GRU_H) gxs[l] = (l < a.dim_x) ? a.gx0[int64_t(b) * a.dim_x + l] : 0.0;
    const double hR = (l < GRU_H) ? a.act[int64_t(a.B) * a.R * 64 + int64_t(b) * GRU_H + l] : 0.0;
    __syncthreads();
    double dh = 0.0;
    if (l < GRU_H) {
        for (int d = 0; d < a.dim_x; ++d) {
            gWd[l * a.dim_x + d] = hR * gxs[d];
            dh = fma(a.Wd[l * a.dim_x + d], gxs[d], dh);
        }
    }
    if (l < a.dim_x) gbd[l] = gxs[l];
    // accumulators of this lane: W_g column l & 31, rows (l >> 5) + 2 k;  W_c column l & 15, rows (l >> 4) + 4 k
    constexpr int NG = (GRU_MAXIN + GRU_H + 1) / 2, NC = (GRU_MAXIN + GRU_H + 3) / 4;
    double accg[NG], accc[NC], accbg = 0.0, accbc = 0.0;
#pragma unroll
    for (int k = 0; k < NG; ++k) accg[k] = 0.0;
#pragma unroll
    for (int k = 0; k < NC; ++k) accc[k] = 0.0;
    for (int step = a.R - 1; step >= 0; --step) {
        const double* o = a.act + (int64_t(b) * a.R + step) * 64;
        double h = 0.0, r = 0.0, z = 0.0, c = 0.0;
        if (l < GRU_H) { h = o[l]; r = o[16 + l]; z = o[32 + l]; c = o[48 + l]; hp[l] = h; rs[l] = r; }
        if (l < n_in) xs[l] = gru_input(a, b, step, l);
        // h' = u h + (1 - u) c
        double dz = 0.0, dhn = 0.0;
        if (l < GRU_H) {
            dz = dh * (h - c);
            dcp[l] = dh * (1.0 - z) * (1.0 - c * c);                          // through tanh
            dhn = dh * z;
        }
        __syncthreads();
        // candidate: c = tanh([x, r o h] W_c + b_c)
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const int i = (l >> 4) + 4 * k;
            if (i < nrow) accc[k] = fma((i < n_in) ? xs[i] : rs[i - n_in] * hp[i - n_in], dcp[l & 15], accc[k]);
        }
        if (l < GRU_H) accbc += dcp[l];
        double dr = 0.0;
        if (l < GRU_H) {
            double drh = 0.0;                                                 // d loss / d (r o h)_l
            for (int j = 0; j < GRU_H; ++j) drh = fma(a.Wc[(n_in + l) * 16 + j], dcp[j], drh);
            dr = drh * h;
            dhn = fma(drh, r, dhn);
            dgp[l] = dr * r * (1.0 - r);                                      // through the sigmoids
            dgp[16 + l] = dz * z * (1.0 - z);
        }
        __syncthreads();
        // gates: [r | u] = sigmoid([x, h] W_g + b_g)
#pragma unroll
        for (int k = 0; k < NG; ++k) {
            const int i = (l >> 5) + 2 * k;
            if (i < nrow) accg[k] = fma((i < n_in) ? xs[i] : hp[i - n_in], dgp[l & 31], accg[k]);
        }
        if (l < 2 * GRU_H) accbg += dgp[l];
        if (l < GRU_H) {
            for (int j = 0; j < 2 * GRU_H; ++j) dhn = fma(a.Wg[(n_in + l) * 32 + j], dgp[j], dhn);
            dh = dhn;
        }
        if (IN && l < n_in) {
            // the step's input x = [u, y][R - 1 - step] enters both pre-activations: gates first, ascending j
            double gx = 0.0;
            for (int j = 0; j < 2 * GRU_H; ++j) gx = fma(a.Wg[l * 32 + j], dgp[j], gx);
            for (int j = 0; j < GRU_H; ++j) gx = fma(a.Wc[l * 16 + j], dcp[j], gx);
            a.gwin[(int64_t(b) * a.R + (a.R - 1 - step)) * n_in + l] = gx;
        }
        __syncthreads();                                                      // the shared vectors are rewritten above
    }
#pragma unroll
    for (int k = 0; k < NG; ++k) {
        const int i = (l >> 5) + 2 * k;
        if (i < nrow) gWg[i * 32 + (l & 31)] = accg[k];
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const int i = (l >> 4) + 4 * k;
        if (i < nrow) gWc[i * 16 + (l & 15)] = accc[k];
    }
    if (l < 2 * GRU_H) gbg[l] = accbg;
    if (l < GRU_H) gbc[l] = accbc;
}

static int fill_gru(GruArgs& a, int B, int T, int dim_u, int dim_y, int dim_x, int recog_len, const double* u, const double* y,
                    const double* params)
{
    if (B < 1 || T < 1 || dim_u < 0 || dim_y < 1 || dim_x < 1 || recog_len < 1) return fail(-1, "bad dimensions");
    if (dim_u + dim_y > GRU_MAXIN || dim_x > GRU_H) return fail(-3, "recognition kernel limits: dim_u + dim_y <= 32, dim_x <= 16");
    if (recog_len > T) return fail(-1, "recog_len exceeds the sequence length");
    if (!u && dim_u > 0) return fail(-1, "null pointer");
    if (!y || !params) return fail(-1, "null pointer");
    const int nrow = dim_u + dim_y + GRU_H;
    a.B = B; a.T = T; a.dim_u = dim_u; a.dim_y = dim_y; a.dim_x = dim_x; a.R = recog_len;
    a.u = u; a.y = y;
    a.Wg = params; a.bg = a.Wg + int64_t(nrow) * 32; a.Wc = a.bg + 32; a.bc = a.Wc + int64_t(nrow) * 16;
    a.Wd = a.bc + 16; a.bd = a.Wd + int64_t(GRU_H) * dim_x;
    a.P = int64_t(nrow) * 48 + 48 + int64_t(GRU_H) * dim_x + dim_x;
    a.x0 = nullptr; a.act = nullptr; a.gx0 = nullptr; a.gpart = nullptr; a.gwin = nullptr;
    return 0;
}

// ---- PR-SSM's conv recognition model (cbfssm/model/prssm.py:146-157) ---------------------------------------------------
// x_0 = dense(flatten(max_pool(2, 2)(relu(conv1d(5 filters, width 3, valid)(float32(first recog_len steps of [u, y]))))))
// in float32 arithmetic, as the reference casts it.  ONE wave per sequence: the window and the four tensors are staged
// in LDS (rounded to float32 as they are read); lane j = 5 p + f owns pooled output (p, f) -- its two pre-activations, the
// relu and the max stay in registers, so pooling needs no exchange; lanes d < dim_x then do the dense layer.  The
// backward kernel keeps no activations: it recomputes the forward in the same device function (same operation order =>
// the same pooling winners and relu mask, bit for bit) and then its lanes own entries of the sequence's gradient slab.
constexpr int CONV_F = 5, CONV_W = 3;     // prssm.py:150
constexpr int CONV_MAXR = 64;             // recog_len: an 8 KB window at 32 inputs
constexpr int CONV_MAXP = (CONV_MAXR - 2) / 2;

struct ConvArgs {
    int B, T, dim_u, dim_y, dim_x, R, P;
    const double* u;
    const double* y;
    const double* K;      // [3][n_in][5]   (TensorFlow's layout)
    const double* bc;     // [5]
    const double* Wd;     // [5 P][dim_x]   rows in (time, channel) order
    const double* bd;     // [dim_x]
    double* x0;           // [B][dim_x]
    const double* gx0;    // [B][dim_x]   d loss / d x_0
    double* gpart;        // [B][E]       per-sequence gradient slabs, the four tensors behind each other
    int64_t E;
    double* gwin;         // [B][R][n_in] d loss / d window [u, y][:, :R], or null (weights only)
};

struct ConvShared {
    float x[CONV_MAXR * GRU_MAXIN];       // the window, [t][i]
    float K[CONV_W * GRU_MAXIN * CONV_F];
    float Wd[CONV_F * CONV_MAXP * GRU_H];
    float pool[CONV_F * CONV_MAXP];
    float gpre[(CONV_MAXR - 2) * CONV_F]; // d loss / d pre-activation, [t][f]
    float bc[CONV_F], bd[GRU_H], gx[GRU_H];
    int win[CONV_F * CONV_MAXP];          // position of the pooling winner when its pre-activation is positive, else -1
};

__device__ __forceinline__ float conv_pre(const ConvShared& s, int n_in, int t, int f)
{
    float acc = s.bc[f];
    const float* xr = s.x + t * n_in;                                        // rows t .. t + 2 are contiguous: [w][i]
    for (int k = 0; k < CONV_W * n_in; ++k) acc = fmaf(xr[k], s.K[k * CONV_F + f], acc);
    return acc;
}

// stages the operands and leaves pool / win in LDS (synchronised); returns x_0[b][l] on lanes l < dim_x
__device__ __forceinline__ float conv_forward(const ConvArgs& a, ConvShared& s, int b, int l)
{
    const int n_in = a.dim_u + a.dim_y, npool = CONV_F * a.P;
    for (int e = l; e < a.R * n_in; e += 64) {
        const int t = e / n_in, i = e - t * n_in;
        s.x[e] = float((i < a.dim_u) ? a.u[(int64_t(b) * a.T + t) * a.dim_u + i]
                                     : a.y[(int64_t(b) * a.T + t) * a.dim_y + (i - a.dim_u)]);
    }
    for (int e = l; e < CONV_W * n_in * CONV_F; e += 64) s.K[e] = float(a.K[e]);
    for (int e = l; e < npool * a.dim_x; e += 64) s.Wd[e] = float(a.Wd[e]);
    if (l < CONV_F) s.bc[l] = float(a.bc[l]);
    if (l < a.dim_x) s.bd[l] = float(a.bd[l]);
    __syncthreads();
    for (int j = l; j < npool; j += 64) {
        const int p = j / CONV_F, f = j - p * CONV_F;
        const float p0 = conv_pre(s, n_in, 2 * p, f), p1 = conv_pre(s, n_in, 2 * p + 1, f);
        const float a0 = fmaxf(p0, 0.0f), a1 = fmaxf(p1, 0.0f);
        const bool first = a0 >= a1;                                         // a tie goes to the first element
        s.pool[j] = first ? a0 : a1;
        s.win[j] = ((first ? p0 : p1) > 0.0f) ? 2 * p + (first ? 0 : 1) : -1;   // relu'(0) = 0
    }
    __syncthreads();
    float acc = 0.0f;
    if (l < a.dim_x) {
        acc = s.bd[l];
        for (int j = 0; j < npool; ++j) acc = fmaf(s.pool[j], s.Wd[j * a.dim_x + l], acc);
    }
    return acc;
}

__global__ __launch_bounds__(64) void conv_forward_kernel(ConvArgs a)
{
    __shared__ ConvShared s;
    const int l = threadIdx.x, b = blockIdx.x;
    const float v = conv_forward(a, s, b, l);
    if (l < a.dim_x) a.x0[int64_t(b) * a.dim_x + l] = double(v);
}

template <bool IN>      // IN: also the adjoint of the window (ConvArgs::gwin); a template flag like the GRU kernel's
__global__ __launch_bounds__(64) void conv_backward_kernel(ConvArgs a)
{
    __shared__ ConvShared s;
    const int l = threadIdx.x, b = blockIdx.x;
    const int n_in = a.dim_u + a.dim_y, npool = CONV_F * a.P, npre = a.R - 2, dx = a.dim_x;
    double* gK = a.gpart + int64_t(b) * a.E;
    double* gbc = gK + CONV_W * n_in * CONV_F;
    double* gWd = gbc + CONV_F;
    double* gbd = gWd + npool * dx;
    conv_forward(a, s, b, l);
    if (l < dx) s.gx[l] = float(a.gx0[int64_t(b) * dx + l]);
    for (int e = l; e < npre * CONV_F; e += 64) s.gpre[e] = 0.0f;
    __syncthreads();
    // dense layer: x_0 = pool W_d + b_d
    for (int e = l; e < npool * dx; e += 64) {
        const int j = e / dx;
        gWd[e] = double(s.pool[j] * s.gx[e - j * dx]);
    }
    if (l < dx) gbd[l] = double(s.gx[l]);
    // through the pooling and the relu: the winner of each pair takes the pooled output's adjoint if it is positive
    for (int j = l; j < npool; j += 64) {
        float g = 0.0f;
        for (int d = 0; d < dx; ++d) g = fmaf(s.Wd[j * dx + d], s.gx[d], g);
        if (s.win[j] >= 0) s.gpre[s.win[j] * CONV_F + (j % CONV_F)] = g;
    }
    __syncthreads();
    // conv kernel entry (w, i, f) and the conv bias: one lane sums over the positions in ascending order
    for (int e = l; e < CONV_W * n_in * CONV_F; e += 64) {
        const int k = e / CONV_F, f = e - k * CONV_F;                        // k = w n_in + i: x[t + w][i] = x[t n_in + k]
        float g = 0.0f;
        for (int t = 0; t < npre; ++t) g = fmaf(s.x[t * n_in + k], s.gpre[t * CONV_F + f], g);
        gK[e] = double(g);
    }
    if (l < CONV_F) {
        float g = 0.0f;
        for (int t = 0; t < npre; ++t) g += s.gpre[t * CONV_F + l];
        gbc[l] = double(g);
    }
    // window entry (t, i): conv position t - w reads it through tap w (the casts' adjoint is the identity)
    if (IN) {
        for (int e = l; e < a.R * n_in; e += 64) {
            const int t = e / n_in, i = e - t * n_in;
            float g = 0.0f;
            for (int w = 0; w < CONV_W; ++w) {
                const int pos = t - w;
                if (pos < 0 || pos >= npre) continue;
                for (int f = 0; f < CONV_F; ++f) g = fmaf(s.K[(w * n_in + i) * CONV_F + f], s.gpre[pos * CONV_F + f], g);
            }
            a.gwin[int64_t(b) * a.R * n_in + e] = double(g);
        }
    }
}

static int64_t conv_elems(int dim_u, int dim_y, int dim_x, int recog_len)
{
    const int64_t n_in = int64_t(dim_u) + dim_y, P = (recog_len - 2) / 2;
    return CONV_W * n_in * CONV_F + CONV_F + CONV_F * P * dim_x + dim_x;
}

// -1: not a conv recognition model at all; -3: one the kernels have no room for; 0: fine
static int conv_dims(int dim_u, int dim_y, int dim_x, int recog_len)
{
    if (dim_u < 0 || dim_y < 1 || dim_x < 1 || recog_len < 4) return -1;
    if (int64_t(dim_u) + dim_y > GRU_MAXIN || dim_x > GRU_H || recog_len > CONV_MAXR) return -3;
    return 0;
}

static int fill_conv(ConvArgs& a, int B, int T, int dim_u, int dim_y, int dim_x, int recog_len, const double* u, const double* y,
                     const double* params)
{
    if (B < 1 || T < 1) return fail(-1, "bad dimensions");
    const int rc = conv_dims(dim_u, dim_y, dim_x, recog_len);
    if (rc == -1) return fail(-1, "bad dimensions (conv recognition: dim_y >= 1, dim_x >= 1, recog_len >= 4)");
    if (rc) return fail(-3, "conv recognition kernel limits: dim_u + dim_y <= 32, dim_x <= 16, recog_len <= 64");
    if (recog_len > T) return fail(-1, "recog_len exceeds the sequence length");
    if (!u && dim_u > 0) return fail(-1, "null pointer");
    if (!y || !params) return fail(-1, "null pointer");
    const int n_in = dim_u + dim_y;
    a.B = B; a.T = T; a.dim_u = dim_u; a.dim_y = dim_y; a.dim_x = dim_x; a.R = recog_len; a.P = (recog_len - 2) / 2;
    a.u = u; a.y = y;
    a.K = params; a.bc = a.K + CONV_W * n_in * CONV_F; a.Wd = a.bc + CONV_F; a.bd = a.Wd + CONV_F * a.P * dim_x;
    a.E = conv_elems(dim_u, dim_y, dim_x, recog_len);
    a.x0 = nullptr; a.gx0 = nullptr; a.gpart = nullptr; a.gwin = nullptr;
    return 0;
}

}  // namespace cbfssm

using namespace cbfssm;

extern "C" {

int64_t cbfssm_gru_recog_param_elems(int dim_u, int dim_y, int dim_x)
{
    if (dim_u < 0 || dim_y < 1 || dim_x < 1) return -1;
    return int64_t(dim_u + dim_y + GRU_H) * 48 + 48 + int64_t(GRU_H) * dim_x + dim_x;
}

int64_t cbfssm_gru_recog_act_elems(int B, int recog_len)
{
    if (B < 1 || recog_len < 1) return -1;
    return int64_t(B) * recog_len * 64 + int64_t(B) * GRU_H;
}

int cbfssm_gru_recog_f64(int B, int T, int dim_u, int dim_y, int dim_x, int recog_len, const double* u, const double* y,
                         const double* params, double* x0, double* act, void* stream)
{
    GruArgs a;
    int rc = fill_gru(a, B, T, dim_u, dim_y, dim_x, recog_len, u, y, params);
    if (rc) return rc;
    if (!x0) return fail(-1, "null pointer");
    a.x0 = x0; a.act = act;
    hipLaunchKernelGGL(gru_forward_kernel, dim3(unsigned(B)), dim3(64), 0, (hipStream_t)stream, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail(-int(e) - 1000, "gru forward launch failed");
}

static int gru_backward(int B, int T, int dim_u, int dim_y, int dim_x, int recog_len, const double* u, const double* y,
                        const double* params, const double* act, const double* gx0, double* gpart, double* gwin,
                        bool want_in, void* stream)
{
    GruArgs a;
    int rc = fill_gru(a, B, T, dim_u, dim_y, dim_x, recog_len, u, y, params);
    if (rc) return rc;
    if (!act || !gx0 || !gpart || (want_in && !gwin)) return fail(-1, "null pointer");
    a.act = const_cast<double*>(act); a.gx0 = gx0; a.gpart = gpart; a.gwin = gwin;
    if (want_in) hipLaunchKernelGGL(gru_backward_kernel<true>, dim3(unsigned(B)), dim3(64), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(gru_backward_kernel<false>, dim3(unsigned(B)), dim3(64), 0, (hipStream_t)stream, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail(-int(e) - 1000, "gru backward launch failed");
}

int cbfssm_gru_recog_bwd_f64(int B, int T, int dim_u, int dim_y, int dim_x, int recog_len, const double* u, const double* y,
                             const double* params, const double* act, const double* gx0, double* gpart, void* stream)
{
    return gru_backward(B, T, dim_u, dim_y, dim_x, recog_len, u, y, params, act, gx0, gpart, nullptr, false, stream);
}

int cbfssm_gru_recog_bwd_in_f64(int B, int T, int dim_u, int dim_y, int dim_x, int recog_len, const double* u, const double* y,
                                const double* params, const double* act, const double* gx0, double* gpart, double* gwin,
                                void* stream)
{
    return gru_backward(B, T, dim_u, dim_y, dim_x, recog_len, u, y, params, act, gx0, gpart, gwin, true, stream);
}

int64_t cbfssm_conv_recog_param_elems(int dim_u, int dim_y, int dim_x, int recog_len)
{
    const int rc = conv_dims(dim_u, dim_y, dim_x, recog_len);
    return rc ? rc : conv_elems(dim_u, dim_y, dim_x, recog_len);
}

int cbfssm_conv_recog_f32(int B, int T, int dim_u, int dim_y, int dim_x, int recog_len, const double* u, const double* y,
                          const double* params, double* x0, void* stream)
{
    ConvArgs a;
    int rc = fill_conv(a, B, T, dim_u, dim_y, dim_x, recog_len, u, y, params);
    if (rc) return rc;
    if (!x0) return fail(-1, "null pointer");
    a.x0 = x0;
    hipLaunchKernelGGL(conv_forward_kernel, dim3(unsigned(B)), dim3(64), 0, (hipStream_t)stream, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail(-int(e) - 1000, "conv recognition forward launch failed");
}

static int conv_backward(int B, int T, int dim_u, int dim_y, int dim_x, int recog_len, const double* u, const double* y,
                         const double* params, const double* gx0, double* gpart, double* gwin, bool want_in, void* stream)
{
    ConvArgs a;
    int rc = fill_conv(a, B, T, dim_u, dim_y, dim_x, recog_len, u, y, params);
    if (rc) return rc;
    if (!gx0 || !gpart || (want_in && !gwin)) return fail(-1, "null pointer");
    a.gx0 = gx0; a.gpart = gpart; a.gwin = gwin;
    if (want_in) hipLaunchKernelGGL(conv_backward_kernel<true>, dim3(unsigned(B)), dim3(64), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(conv_backward_kernel<false>, dim3(unsigned(B)), dim3(64), 0, (hipStream_t)stream, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail(-int(e) - 1000, "conv recognition backward launch failed");
}

int cbfssm_conv_recog_bwd_f32(int B, int T, int dim_u, int dim_y, int dim_x, int recog_len, const double* u, const double* y,
                              const double* params, const double* gx0, double* gpart, void* stream)
{
    return conv_backward(B, T, dim_u, dim_y, dim_x, recog_len, u, y, params, gx0, gpart, nullptr, false, stream);
}

int cbfssm_conv_recog_bwd_in_f32(int B, int T, int dim_u, int dim_y, int dim_x, int recog_len, const double* u, const double* y,
                                 const double* params, const double* gx0, double* gpart, double* gwin, void* stream)
{
    return conv_backward(B, T, dim_u, dim_y, dim_x, recog_len, u, y, params, gx0, gpart, gwin, true, stream);
}

}  // extern "C"
