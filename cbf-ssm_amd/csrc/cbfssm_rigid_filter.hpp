// The per-chain arithmetic of Voliro's forward filter run (cbfssm/model/voliro.py:188-242,314-338 with
// cbfssm/utils/quaternions.py): one rigid-body symplectic-Euler step and its adjoint, as plain inline functions of
// doubles in registers.  Shared by the forward and the reverse kernel of cbfssm_rigid_filter.hip (the reverse sweep
// recomputes every step's f from the previous state), and callable on the host.
//
// State: pos 0:3, quaternion 3:7 (scalar first, Hamilton product as quaternions.py:8-13), linvel 7:10, angvel 10:13.
//
//   fg = rot_vec(u[0:3], rot),  tg = rot_vec(inertia_inv * u[3:6], rot)          rot_vec(v, q) = (q (0,v) q*)[1:] = R(q) v
//   linvel' = linvel + (mass_inv fg + gravity) dt,   angvel' = angvel + tg dt
//   pos' = pos + linvel' dt,   rot~ = rot + 0.5 ((0,angvel') (x) rot) dt,   rot' = rot~ / |rot~|
//
// R(q) is the homogeneous quadratic form of q (NOT normalised: the filtered state's quaternion is not unit, and
// quaternions.py does not normalise either, so rot_vec scales by |q|^2).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/cbfssm_hip.h"

namespace cbfssm {

constexpr int RF_DX = 13;       // state
constexpr int RF_DU = 6;        // force, torque
constexpr int RF_WG = 64;       // chains per workgroup: one wave, one lane per chain
constexpr int RF_SLAB = 32;     // [d/d var_x (13) | d/d var_y (13) | padding]

#define CBF_RF_FN __host__ __device__ __forceinline__

CBF_RF_FN void rf_rotmat(const double* q, double* R)
{
    const double a = q[0], b = q[1], c = q[2], d = q[3];
    const double aa = a * a, bb = b * b, cc = c * c, dd = d * d;
    R[0] = aa + bb - cc - dd; R[1] = 2.0 * (b * c - a * d); R[2] = 2.0 * (b * d + a * c);
    R[3] = 2.0 * (b * c + a * d); R[4] = aa - bb + cc - dd; R[5] = 2.0 * (c * d - a * b);
    R[6] = 2.0 * (b * d - a * c); R[7] = 2.0 * (c * d + a * b); R[8] = aa - bb - cc + dd;
}

// f = symplectic_euler(x, u); inv_n (optional) = 1 / |rot~|, which the adjoint needs
CBF_RF_FN void rf_step(const cbfssm_rigid_body& rb, const double* x, const double* u, double* f, double* inv_n)
{
    double R[9];
    rf_rotmat(x + 3, R);
    const double dt = rb.dt;
    const double t0 = rb.inertia_inv[0] * u[3], t1 = rb.inertia_inv[1] * u[4], t2 = rb.inertia_inv[2] * u[5];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double fg = R[3 * i] * u[0] + R[3 * i + 1] * u[1] + R[3 * i + 2] * u[2];
        const double tg = R[3 * i] * t0 + R[3 * i + 1] * t1 + R[3 * i + 2] * t2;
        f[7 + i] = x[7 + i] + (rb.mass_inv * fg + rb.gravity[i]) * dt;
        f[10 + i] = x[10 + i] + tg * dt;
        f[i] = x[i] + f[7 + i] * dt;
    }
    const double wx = f[10], wy = f[11], wz = f[12];
    const double r0 = x[3], r1 = x[4], r2 = x[5], r3 = x[6];
    const double h = 0.5 * dt;
    const double q0 = r0 + h * (-wx * r1 - wy * r2 - wz * r3);
    const double q1 = r1 + h * (wx * r0 + wy * r3 - wz * r2);
    const double q2 = r2 + h * (-wx * r3 + wy * r0 + wz * r1);
    const double q3 = r3 + h * (wx * r2 - wy * r1 + wz * r0);
    const double in = 1.0 / sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    f[3] = q0 * in; f[4] = q1 * in; f[5] = q2 * in; f[6] = q3 * in;
    if (inv_n) *inv_n = in;
}

// gf = d loss / d f  ->  gx = d loss / d x (written), gu = d loss / d u (written); f, inv_n from rf_step(x, u)
CBF_RF_FN void rf_step_bwd(const cbfssm_rigid_body& rb, const double* x, const double* u, const double* f, double inv_n,
                           const double* gf, double* gx, double* gu)
{
    const double dt = rb.dt;
    const double r0 = x[3], r1 = x[4], r2 = x[5], r3 = x[6];
    // rot' = rot~ / n
    const double dot = f[3] * gf[3] + f[4] * gf[4] + f[5] * gf[5] + f[6] * gf[6];
    double gq[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) gq[i] = (gf[3 + i] - f[3 + i] * dot) * inv_n;
    // rot~ = rot + 0.5 dt (0, w') (x) rot
    const double h = 0.5 * dt;
    const double h0 = h * gq[0], h1 = h * gq[1], h2 = h * gq[2], h3 = h * gq[3];
    const double wx = f[10], wy = f[11], wz = f[12];
    double gw[3], gv[3], gr[4];
    gw[0] = gf[10] + (-h0 * r1 + h1 * r0 - h2 * r3 + h3 * r2);
    gw[1] = gf[11] + (-h0 * r2 + h1 * r3 + h2 * r0 - h3 * r1);
    gw[2] = gf[12] + (-h0 * r3 - h1 * r2 + h2 * r1 + h3 * r0);
    gr[0] = gq[0] + (h1 * wx + h2 * wy + h3 * wz);
    gr[1] = gq[1] + (-h0 * wx + h2 * wz - h3 * wy);
    gr[2] = gq[2] + (-h0 * wy - h1 * wz + h3 * wx);
    gr[3] = gq[3] + (-h0 * wz + h1 * wy - h2 * wx);
    // pos' = pos + linvel' dt
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        gx[i] = gf[i];
        gv[i] = gf[7 + i] + gf[i] * dt;
        gx[7 + i] = gv[i];
        gx[10 + i] = gw[i];
    }
    // linvel' = linvel + (mass_inv R F + g) dt, angvel' = angvel + R T dt
    const double gfg[3] = {gv[0] * rb.mass_inv * dt, gv[1] * rb.mass_inv * dt, gv[2] * rb.mass_inv * dt};
    const double gtg[3] = {gw[0] * dt, gw[1] * dt, gw[2] * dt};
    double R[9];
    rf_rotmat(x + 3, R);
    const double tq[3] = {rb.inertia_inv[0] * u[3], rb.inertia_inv[1] * u[4], rb.inertia_inv[2] * u[5]};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        gu[j] = R[j] * gfg[0] + R[3 + j] * gfg[1] + R[6 + j] * gfg[2];
        gu[3 + j] = rb.inertia_inv[j] * (R[j] * gtg[0] + R[3 + j] * gtg[1] + R[6 + j] * gtg[2]);
    }
    double G[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) G[3 * i + j] = gfg[i] * u[j] + gtg[i] * tq[j];
    const double tr = G[0] + G[4] + G[8];
    const double s10 = G[3] - G[1], s02 = G[2] - G[6], s21 = G[7] - G[5];     // antisymmetric part
    const double p01 = G[1] + G[3], p02 = G[2] + G[6], p12 = G[5] + G[7];     // symmetric off-diagonal part
    gx[3] = gr[0] + 2.0 * (r0 * tr + r3 * s10 + r2 * s02 + r1 * s21);
    gx[4] = gr[1] + 2.0 * (r1 * (G[0] - G[4] - G[8]) + r2 * p01 + r3 * p02 + r0 * s21);
    gx[5] = gr[2] + 2.0 * (r2 * (G[4] - G[0] - G[8]) + r1 * p01 + r0 * s02 + r3 * p12);
    gx[6] = gr[3] + 2.0 * (r3 * (G[8] - G[0] - G[4]) + r0 * s10 + r1 * p02 + r2 * p12);
}

// loop-invariant filter constants of one state dimension (voliro.py:227-232,238)
struct RfGain {
    double k;        // q / (q + r)
    double omk;      // 1 - k
    double s;        // sqrt(sig),  sig = (1-k)^2 q + k^2 r
    double c;        // k^2 / q: weight of 0.5 (y - f)^2 in the KL
    double kl0;      // 0.5 (log q - log sig + sig / q - 1): the data-independent KL of one step
};

CBF_RF_FN RfGain rf_gain(double q, double r)
{
    RfGain g;
    g.k = q / (q + r);
    g.omk = 1.0 - g.k;
    const double sig = g.omk * g.omk * q + g.k * g.k * r;
    g.s = sqrt(sig);
    g.c = g.k * g.k / q;
    g.kl0 = 0.5 * (log(q) - log(sig) + sig / q - 1.0);
    return g;
}

// d loss / d (q, r) of one dimension from the sums of one chain:
//   A = sum_t gx (y - f),  Bn = sum_t gx eps,  Cn = g_kl sum_t (y - f)^2,  W = g_kl * steps
CBF_RF_FN void rf_gain_bwd(double q, double r, double A, double Bn, double Cn, double W, double* gq, double* gr)
{
    const double s = q + r, k = q / s, omk = 1.0 - k;
    const double sig = omk * omk * q + k * k * r;
    const double sd = sqrt(sig);
    // x = (1-k) f + k y + eps sqrt(sig);  kl = 0.5 k^2 (y-f)^2 / q + kl0
    const double gk_x = A + Cn * k / q;
    double gsig = Bn * 0.5 / sd + W * 0.5 * (1.0 / q - 1.0 / sig);
    const double gk = gk_x + gsig * (2.0 * k * r - 2.0 * omk * q);
    *gq = gk * (r / (s * s)) + gsig * (omk * omk) - 0.5 * Cn * k * k / (q * q) + W * 0.5 * (1.0 / q - sig / (q * q));
    *gr = -gk * (q / (s * s)) + gsig * (k * k);
}

}  // namespace cbfssm
