/*
 * cbfssm_hip.h -- C ABI of the MI355X (gfx950) implementation of the CBF-SSM ELBO hot path.
 *
 * The reference (silvanmelchior/CBF-SSM) has no FFI / plugin interface: the path is Python graph-building code over
 * TensorFlow ops.  Each entry point below therefore replaces a *set of TensorFlow op call sites*; the cited
 * file:line ranges are relative to the reference repository root.
 *
 * Conventions
 *   - every pointer is a caller-owned DEVICE pointer to contiguous row-major float64 unless marked "host";
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), never allocates, never synchronises;
 *   - return value: 0 = OK, <0 = argument / launch error (text in cbfssm_last_error(), thread local);
 *   - numerical failure of the Cholesky (leading minor not positive definite; TensorFlow raises
 *     InvalidArgumentError there) is reported asynchronously in pack[scal + CBFSSM_SCAL_INFO] (k>0 = minor k);
 *   - chains: N = B*S particle chains, chain index c = b*S + s; trajectories are kept TIME-MAJOR on the device:
 *     x[t][c][d], y2[t][c][d] (the reference's (B,T,S,d) tensors are stride-permuted views of these).
 */
#ifndef CBFSSM_HIP_H
#define CBFSSM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CBFSSM_MAX_DOUT 16   /* GP output dimension (dim_x) handled by one 16-row MFMA block */
#define CBFSSM_MAX_DIN 64    /* GP input dimension dim_x + dim_u */
#define CBFSSM_MAX_M 320     /* inducing points */

/* indices into the scalar block of a GP pack */
enum {
    CBFSSM_SCAL_SIGMA2 = 0,  /* kernel variance */
    CBFSSM_SCAL_LOGDET = 1,  /* log det (K_mm + jitter I) */
    CBFSSM_SCAL_KLZ = 2,     /* prior_kl() */
    CBFSSM_SCAL_INFO = 3,    /* 0 = OK, k>0 = leading minor k not positive definite */
    CBFSSM_SCAL_COND = 4,    /* infinity-norm condition number of K_mm + jitter I: |K|_inf |K^-1|_inf */
    CBFSSM_SCAL_JITTER = 5,  /* the jitter this pack was prepared with */
    CBFSSM_SCAL_COUNT = 16
};

/* how GPModel.predict is evaluated by the pass / predict kernels (cbfssm_pack_layout.gp_form) */
enum {
    CBFSSM_GP_FORM_DENSE = 0,   /* A2 = K^-1 k as one dense product, fvar_0 = sigma^2 - k.A2                      */
    CBFSSM_GP_FORM_TRI = 1      /* the reference's own order (gp_tf.py:137-145): A = L^-1 k, fvar_0 = sigma^2 - |A|^2,
                                   A2 = L^-T A, as two triangular products -- same multiply-adds, no cancellation
                                   of k.(K^-1 k) against sigma^2 on an ill-conditioned K_mm                        */
};

/* Offsets (in doubles) of the sections of one GP pack; filled by cbfssm_gp_pack_layout (host struct). */
typedef struct {
    int64_t total;    /* doubles to allocate */
    int64_t Bp;       /* [NBLK][KS][64]  K^-1 as MFMA A-operand image, zero padded to Mp = 16*NBLK           */
    int64_t Zp;       /* [NBLK][DK][64]  Z/lengthscale as MFMA A-operand image                               */
    int64_t cz;       /* [Mp]            -0.5|z~|^2 + log sigma^2 (padding rows: -1e30)                      */
    int64_t muA;      /* [NBLK][4][64]   zeta_mean as A-operand image of the epilogue product                */
    int64_t s2A;      /* [NBLK][4][64]   zeta_var  as A-operand image                                        */
    int64_t invl;     /* [Dp]            1/lengthscale, zero padded                                          */
    int64_t scal;     /* [CBFSSM_SCAL_COUNT]                                                                 */
    int64_t Kmm;      /* [M][M]          kernel matrix, no jitter          (gp_tf.py:129)                    */
    int64_t L;        /* [M][M]          lower Cholesky factor             (gp_tf.py:130)                    */
    int64_t Kinv;     /* [M][M]          (K_mm + jitter I)^-1                                                */
    int64_t Linvt;    /* [M][M]          L^-T (upper triangular), by-product of the factorisation            */
    int64_t Zs;       /* [M][D]          Z / lengthscale                                                     */
    int64_t muB;      /* [NBLK][4][64]   zeta_mean as A-operand image A[row m][k = d]      (adjoint kernels)        */
    int64_t s2B;      /* [NBLK][4][64]   zeta_var, same image                                                        */
    int64_t ZT;       /* [NBLK][JB][4][64] (Z/lengthscale)^T as A-operand image A[row j][k = m]; row D = ones        */
    int64_t rev_slab; /* doubles of one adjoint partial slab (0: no adjoint kernel for this tile height)            */
    int64_t work;     /* [M][M|1]        factorisation workspace when M is too large for LDS                        */
    int64_t Wp;       /* [NBLK][KS][64]  W = L^-1 (lower triangular) as MFMA A-operand image      (gp_tf.py:137)         */
    int64_t WTp;      /* [NBLK][KS][64]  W^T = L^-T as MFMA A-operand image                        (gp_tf.py:145)         */
    int32_t M, D, Do, NBLK, DK, Mp, Dp, KS, JB, rev_stash;   /* rev_stash: 1 = adjoint runs in stash mode (M > 112) */
    int32_t gp_form;  /* CBFSSM_GP_FORM_*: set by the caller after cbfssm_gp_pack_layout (which fills in DENSE); read by
                         cbfssm_gp_predict_f64 and the pass kernels.  Both forms read the same pack.               */
    int32_t reserved;
} cbfssm_pack_layout;

/* Problem description shared by the pass kernels (host struct, passed by pointer). */
typedef struct {
    int32_t B, S, T;            /* sequences, particles per sequence, time steps                             */
    int32_t dim_x, dim_u, dim_y;
    int32_t M;                  /* inducing points                                                           */
    int32_t recog_len;          /* config['recog_len']      cbfssm.py:120,190                                */
    int32_t condition;          /* feed of model.condition  cbfssm.py:227                                    */
    int32_t half;               /* 1: CBFSSMHALF forward pass (cbfssmhalf.py:117-172), 0: CBFSSM                  */
    int32_t group0, ngroups;    /* chain-group split: this call handles the 16-chain groups [group0, group0+ngroups) of
                                   ceil(B*S/16); ngroups = 0 means all.  Chains never interact, so a pass may be issued
                                   in pieces on different streams; partial/slab buffers keep their full-size layout.  */
    double k_factor;            /* config['k_factor']       cbfssm.py:191,214                                */
} cbfssm_problem;

const char* cbfssm_last_error(void);
int cbfssm_version(void);

/* Layout of a GP pack for (M, D = dim_x + dim_u, Do).  Host only. */
int cbfssm_gp_pack_layout(int M, int D, int Do, cbfssm_pack_layout* out);

/*
 * K_mm and its Cholesky factor.
 * Replaces: RBF.K(zeta_pos) (gp_tf.py:33-49,129) and cast_cholesky/_jitter_cholesky (gp_tf.py:52-65,130).
 *   Z (M,D), lengthscales (D), variance (1)  ->  Kmm (M,M) without jitter, L (M,M) lower (upper part zero),
 *   info (1 double: 0 or the failing leading minor).  work: >= M*D + M*(M+1) doubles.
 */
int cbfssm_kmm_chol_f64(int M, int D, const double* Z, const double* lengthscales, const double* variance,
                        double jitter, double* Kmm, double* L, double* info, double* work, void* stream);

/*
 * Everything that is loop invariant for one GPModel, once per ELBO evaluation.
 * Replaces: GPModel.__init__ tail (gp_tf.py:129-130), the operand preparation of GPModel.predict
 * (gp_tf.py:134-159: X/lengthscales, K^-1 instead of two triangular solves) and GPModel.prior_kl (gp_tf.py:163-172).
 *   inputs are the *constrained* values: Z (M,D), lengthscales (D), variance (1), zeta_mean (M,Do), zeta_var (M,Do)
 *   pack: layout.total doubles.
 */
int cbfssm_gp_prepare_f64(const cbfssm_pack_layout* layout, const double* Z, const double* lengthscales,
                          const double* variance, const double* zeta_mean, const double* zeta_var,
                          double jitter, double* pack, void* stream);

/* The same for two GPModels in one launch (gp_f and gp_b of CBFSSM._setup_vars, cbfssm.py:30-48): one workgroup each.
 * The two layouts need not agree in M, D or Do.  The factorisation keeps its working matrix in LDS up to M = 140 and in
 * the pack's `work` section above; when exactly one of the two M exceeds 140 the call issues two single-GP launches on
 * `stream` (as two cbfssm_gp_prepare_f64 calls would), otherwise the one two-workgroup launch.  Either way each pack is
 * bitwise what cbfssm_gp_prepare_f64 writes for the same inputs. */
int cbfssm_gp_prepare2_f64(const cbfssm_pack_layout* layout0, const double* Z0, const double* lengthscales0,
                           const double* variance0, const double* zeta_mean0, const double* zeta_var0, double* pack0,
                           const cbfssm_pack_layout* layout1, const double* Z1, const double* lengthscales1,
                           const double* variance1, const double* zeta_mean1, const double* zeta_var1, double* pack1,
                           double jitter, void* stream);

/*
 * GPModel.predict(Xnew) (gp_tf.py:132-161): X (npts, D) -> fmean (npts, Do), fvar (npts, Do).
 */
int cbfssm_gp_predict_f64(const cbfssm_pack_layout* layout, const double* pack, const double* X, int64_t npts,
                          double* fmean, double* fvar, void* stream);

/*
 * The remaining pieces of gp_tf.py as stand-alone calls (none of them is on a time loop):
 *   cbfssm_cholesky_f64      cast_cholesky / _jitter_cholesky of a GIVEN matrix (gp_tf.py:52-65): mat (M,M) symmetric ->
 *                            L (M,M) lower with mat + jitter I = L L^T, info (1 double: 0 or the failing leading minor);
 *                            work: >= M*(M+1) doubles.  The blocked MFMA factorisation of cbfssm_gp_prepare_f64.
 *   cbfssm_rbf_k_f64         RBF.K(X, X2) (gp_tf.py:33-49): X (n,D), X2 (m,D) -> out (n,m).
 *   cbfssm_gp_predict_fullq_f64   conditional() with a full-matrix q_sqrt (gp_tf.py:68-100, the q_sqrt.ndims == 3 branch):
 *                            the pack is prepared with f as zeta_mean and zeta_var = 0; q_sqrt (Do,M,M) lower triangular
 *                            per output dimension; fvar += sum_j (q_sqrt[d]^T A2)_j^2.  work: cbfssm_gp_predict_fullq_work_elems
 *                            doubles (the A2 tiles).  (The q_sqrt.ndims == 2 branch IS cbfssm_gp_predict_f64 with
 *                            zeta_var = q_sqrt^2; q_sqrt = None is zeta_var = 0.)
 */
int cbfssm_cholesky_f64(int M, const double* mat, double jitter, double* L, double* info, double* work, void* stream);
int cbfssm_rbf_k_f64(int n, int m, int D, const double* X, const double* X2, const double* lengthscales,
                     const double* variance, double* out, void* stream);
int64_t cbfssm_gp_predict_fullq_work_elems(const cbfssm_pack_layout* layout, int64_t npts);
int cbfssm_gp_predict_fullq_f64(const cbfssm_pack_layout* layout, const double* pack, const double* q_sqrt, const double* X,
                                int64_t npts, double* fmean, double* fvar, double* work, void* stream);

/*
 * ---- differentiable GPModel: what tf.gradients gives a graph that calls gp.predict / gp.prior_kl outside a CBF-SSM
 * (gp_tf.py:132-172 differentiated; cbfssm/model/voliro.py:106-123 calls gp_f.predict once over all B T points).
 *
 * cbfssm_gp_predict_bwd_f64: batch adjoint of cbfssm_gp_predict_f64 (gp_tf.py:132-161).  pack: prepared with the
 * parameters of the forward call; X (npts, D); gmean, gvar (npts, Do): d loss / d fmean, d loss / d fvar.
 *   -> gX (npts, D): d loss / d X (the unscaled inputs), every entry written exactly once;
 *      gpart: cbfssm_gp_predict_bwd_workgroups partial slabs of layout->rev_slab doubles in the slab layout of the
 *      time-loop adjoints below ("Slab layout of the parameter adjoints of one GP"; the var_x / var_y entries are zero), with
 *      room for CBFSSM_REDUCE_SPLIT more: cbfssm_reduce_partials_f64(gpart, layout->rev_slab, workgroups, red) sums them;
 *      M > 112 (layout->rev_stash): the slab has no d/dK^-1 section; the call writes the MFMA operand images of
 *      d loss / d K^-1 += A2bar K^T per 16-point block to `work` (cbfssm_gp_predict_bwd_work_elems doubles) and
 *      contracts them (cbfssm_stash_contract_f64) into gB_image, [NBLK][NBLK][4][64] doubles, which it clears first:
 *      hand it to cbfssm_gp_tail_f64 as gB_dense with gB_ld = 0.  M <= 112: work and gB_image may be NULL.
 * Both GP forms (layout->gp_form) have this adjoint: it is evaluated with the K^-1 contraction.  No atomics; two calls are
 * bitwise identical.  Limits as cbfssm_gp_predict_f64 (M <= 320, D <= 24, Do <= 16), else -3 before any launch; the two
 * counts are host arithmetic and return -1 for a bad layout or npts < 0.
 *
 * cbfssm_gp_tail_f64: adjoint of GPModel.__init__ / prior_kl (gp_tf.py:33-65,129-130,163-172) and the chain through the
 * positivity transforms for ONE GP: d (data loss + kl_weight * prior_kl) / d parameters.  Flat vectors (pflat unconstrained,
 * cflat constrained, gflat the gradient) in the order zeta_pos [M][D] | zeta_mean [M][Do] | zeta_var [M][Do] | variance [1] |
 * lengthscales [D].  red_slab: the reduced slab, or NULL for the prior-KL terms alone (gB_dense then NULL too); gB_dense /
 * gB_ld as in cbfssm_train_tail_f64.  work: cbfssm_train_tail_half_work_elems doubles.  (cbfssm_train_tail_half_f64 is the
 * same with kl_weight = 1 and the var_x / var_y entries behind.)
 */
int64_t cbfssm_gp_predict_bwd_workgroups(const cbfssm_pack_layout* layout, int64_t npts);
int64_t cbfssm_gp_predict_bwd_work_elems(const cbfssm_pack_layout* layout, int64_t npts);
int cbfssm_gp_predict_bwd_f64(const cbfssm_pack_layout* layout, const double* pack, const double* X, int64_t npts,
                              const double* gmean, const double* gvar, double* gX, double* gpart, double* work,
                              double* gB_image, void* stream);
int cbfssm_gp_tail_f64(const cbfssm_pack_layout* layout, const double* pack, const double* red_slab, const double* gB_dense,
                       int64_t gB_ld, double kl_weight, const double* pflat, const double* cflat, double* work, double* gflat,
                       void* stream);

/*
 * ---- full-covariance q(z), differentiable: conditional() with q_sqrt of shape (Do, M, M) (gp_tf.py:68-100, the
 * q_sqrt.ndims == 3 branch at :89-98) and GPModel.predict with zeta_std.ndims == 3 (gp_tf.py:150-159), differentiated as
 * tf.gradients does.  L_d = tril(q_sqrt[d]) (entries above the diagonal are never read), S_d = L_d L_d^T, unwhitened:
 *
 *   fvar[n][d] = sigma^2 - k_n^T a_n + a_n^T S_d a_n,  a_n = K^-1 k_n                                  gp_tf.py:79,91-98
 *   prior_kl   = 0.5 sum_d [ tr(K^-1 S_d) + f_d^T K^-1 f_d - M + log det K - sum_i log L_d[i][i]^2 ]   gp_tf.py:163-172 with
 *                                                                                   MultivariateNormalTriL for q
 *
 * The pack is prepared with f as zeta_mean; no call below reads its zeta_var.
 *
 * cbfssm_gp_fullq_prepare_f64 (gp_tf.py:91-93): q_sqrt (Do, M, M) -> qpack (cbfssm_gp_fullq_pack_elems doubles): the MFMA
 *   operand images of S_d, S_d dense, and sum_d S_d.  Once per call of the functions below.
 * cbfssm_gp_fullq_predict_f64 (gp_tf.py:76-98): the forward on the f64 MFMA units, X (npts, D) -> fmean, fvar (npts, Do); A2 in
 *   the form layout->gp_form asks for, then per output dimension S_d A2 from the qpack's images and the column sums
 *   a^T S_d a.  Only the lower triangle of q_sqrt enters.
 * cbfssm_gp_fullq_kl_f64 (gp_tf.py:163-172): zeta_mean (M, Do) -> kl (ONE double on the device).
 * cbfssm_gp_fullq_bwd_f64 (gp_tf.py:76-98 differentiated): the batch adjoint, arguments and results as
 *   cbfssm_gp_predict_bwd_f64 (gX, gpart with cbfssm_gp_fullq_bwd_workgroups slabs and room for CBFSSM_REDUCE_SPLIT more,
 *   the sigma_z^2 section zero; work of cbfssm_gp_fullq_bwd_work_elems doubles and gB_image above M = 112), plus
 *   a2_image (cbfssm_gp_fullq_a2_elems doubles): A2 = K^-1 k of every 16-point block, for cbfssm_gp_fullq_wd_f64.
 * cbfssm_gp_fullq_wd_f64 (gp_tf.py:91-98 differentiated): a2_image, gvar (npts, Do) -> W (Do, M, M),
 *   W_d = sum_n gvar[n][d] a_n a_n^T = d loss / d S_d, exactly symmetric; work: cbfssm_gp_fullq_wd_work_elems doubles
 *   (partial tiles of up to 8 slices of the points, summed in a fixed order).
 * cbfssm_gp_fullq_lbar_f64 (gp_tf.py:91-98,163-172 differentiated): gq (Do, M, M) = tril((2 W_d + kl_weight K^-1) L_d)
 *   - kl_weight diag(1 / L_d[i][i]), exactly zero above the diagonal.  W NULL: the prior-KL part alone; pack NULL: the
 *   data part alone.
 * cbfssm_gp_tail_fullq_f64 (gp_tf.py:33-65,129-130,163-172 differentiated): cbfssm_gp_tail_f64 with the prior-KL part of
 *   the K^-1 adjoint taken from sum_d S_d; the flat vectors keep their order, the zeta_var entries of pflat / cflat are
 *   not read and those of gflat are written as zero.
 * No atomics, no host synchronisation, every output entry has one writer, two calls are bitwise identical; nothing is
 * launched at npts = 0.  Limits as cbfssm_gp_predict_f64 (M <= 320, D <= 24, Do <= 16), else -3 before any launch; NULL
 * pointers -1.  The counts are host arithmetic in 64 bits and return -1 for a bad layout or npts < 0.
 */
int64_t cbfssm_gp_fullq_pack_elems(const cbfssm_pack_layout* layout);
int cbfssm_gp_fullq_prepare_f64(const cbfssm_pack_layout* layout, const double* q_sqrt, double* qpack, void* stream);
int cbfssm_gp_fullq_predict_f64(const cbfssm_pack_layout* layout, const double* pack, const double* qpack, const double* X,
                                int64_t npts, double* fmean, double* fvar, void* stream);
int cbfssm_gp_fullq_kl_f64(const cbfssm_pack_layout* layout, const double* pack, const double* q_sqrt, const double* qpack,
                           const double* zeta_mean, double* kl, void* stream);
int64_t cbfssm_gp_fullq_bwd_workgroups(const cbfssm_pack_layout* layout, int64_t npts);
int64_t cbfssm_gp_fullq_a2_elems(const cbfssm_pack_layout* layout, int64_t npts);
int64_t cbfssm_gp_fullq_bwd_work_elems(const cbfssm_pack_layout* layout, int64_t npts);
int cbfssm_gp_fullq_bwd_f64(const cbfssm_pack_layout* layout, const double* pack, const double* qpack, const double* X,
                            int64_t npts, const double* gmean, const double* gvar, double* gX, double* gpart,
                            double* a2_image, double* work, double* gB_image, void* stream);
int64_t cbfssm_gp_fullq_wd_work_elems(const cbfssm_pack_layout* layout, int64_t npts);
int cbfssm_gp_fullq_wd_f64(const cbfssm_pack_layout* layout, const double* a2_image, const double* gvar, int64_t npts,
                           double* work, double* W, void* stream);
int cbfssm_gp_fullq_lbar_f64(const cbfssm_pack_layout* layout, const double* pack, const double* q_sqrt, const double* W,
                             double kl_weight, double* gq, void* stream);
int cbfssm_gp_tail_fullq_f64(const cbfssm_pack_layout* layout, const double* pack, const double* qpack, const double* red_slab,
                             const double* gB_dense, int64_t gB_ld, double kl_weight, const double* pflat, const double* cflat,
                             double* work, double* gflat, void* stream);

/*
 * ---- local linear model of ONE sparse GP: the Jacobians of GPModel.predict (gp_tf.py:132-161) with respect to its inputs,
 * what the reference gets from tf.gradients(fmean[:, d], Xnew) and tf.gradients(fvar[:, d], Xnew), once per output
 * dimension d, through gp_tf.py:132-161 -- for EKF-style filtering, iLQR / MPC around a learned transition, sensitivities.
 *
 *   dmean[n][d][i] = d fmean[n][d] / d X[n][i],   dvar[n][d][i] = d fvar[n][d] / d X[n][i]      (the unscaled inputs)
 *
 * cbfssm_gp_linearize_f64: pack prepared (diagonal q(z)); X (npts, D) -> dmean (npts, Do, D), and when the pointers are not
 *   NULL fmean, fvar (npts, Do) and dvar (npts, Do, D).  dvar NULL: the mean part alone, without the K^-1 product per output
 *   dimension that the variance needs; dmean and fmean are then bitwise those of the full call.  One pre-kernel forms
 *   alpha = K^-1 mu in `work` (cbfssm_gp_linearize_work_elems doubles; dense form: Kinv mu, two-triangular form:
 *   L^-T (L^-1 mu)), then ONE launch does all output dimensions: per 16 points the kernel tile, A2 = K^-1 k and fvar in the
 *   form layout->gp_form asks for, and per dimension alpha_d o k, 2 (K^-1 (A2 o zeta_var_d) - A2) o k (dense K^-1 image in
 *   both forms) and their products with the pack's (Z / lengthscale)^T image on the f64 MFMA units.  Persistent workgroups,
 *   at most as many as cbfssm_gp_predict_bwd_workgroups names.
 * No atomics, no allocation, no host synchronisation, every output entry has one writer, two calls are bitwise identical,
 * and the results of a point do not depend on the other points of the call; nothing is launched at npts = 0.  Limits as
 * cbfssm_gp_predict_f64 (M <= 320, D <= 24, Do <= 16), else -3 before any launch; NULL layout, pack, X, dmean or work, or
 * npts < 0: -1.  The count is host arithmetic in 64 bits and returns -1 for a bad layout.
 */
int64_t cbfssm_gp_linearize_work_elems(const cbfssm_pack_layout* layout);
int cbfssm_gp_linearize_f64(const cbfssm_pack_layout* layout, const double* pack, const double* X, int64_t npts,
                            double* fmean, double* fvar, double* dmean, double* dvar, double* work, void* stream);

/*
 * ---- exact Gaussian moments of ONE sparse GP under a Gaussian input: for x ~ N(mean[n], cov[n]) and the posterior of
 * GPModel.predict (gp_tf.py:132-161, diagonal q(z), RBF kernel) the mean of the output, its full covariance -- with the
 * correlation between output dimensions that sharing the uncertain input brings -- and its covariance with the input, in
 * closed form (the moment matching of PILCO and of the GP assumed-density filter): nothing is linearised or sampled.
 *
 *   fmean[n][d]   = E[f_d]           fcov[n][d][e] = Cov(f_d, f_e)  (npts, Do, Do)      xcov[n][d][i] = Cov(f_d, x_i)  (npts, Do, D)
 *
 * with f_d | x ~ N(fmean_d(x), fvar_d(x)) independent over d given x, as in predict: diag fcov = E[fvar] + Var[fmean], the
 * off-diagonal is Cov[fmean_d, fmean_e].
 *
 * cbfssm_gp_moment_match_f64: pack prepared (diagonal q(z)); mean (npts, D), cov (npts, D, D) of which only the lower triangle
 *   is read, NULL = zero -> fmean (npts, Do), fcov, info (npts) and, when the pointer is not NULL, xcov; without it the other
 *   results are bitwise the same.  cov need only be positive semi-definite: the two matrices that are factorised, I + S~ and
 *   I / 2 + S~ (S~ = cov in lengthscale units), are positive definite then, so zero blocks, rank one and cov = 0 are ordinary
 *   inputs; cov = 0 gives predict back and xcov exactly zero.  A non-positive pivot sets info[n] = 1 (first factor) or 2
 *   (second) and makes the three results of that point NaN; nothing else is affected.  fcov[n] is bitwise symmetric.
 *   Two pre-kernels form alpha = K^-1 mu (in the order layout->gp_form asks for, as cbfssm_gp_linearize_f64) and the tiles of
 *   W_d = K^-1 - K^-1 diag(zeta_var[:, d]) K^-1 (dense K^-1 in both forms, f64 MFMA) in `work`
 *   (cbfssm_gp_moment_match_work_elems doubles), then ONE launch does the rest: per point the two D x D Cholesky
 *   factorisations in registers, and the M x M matrix Q of expected kernel products as 16 x 16 tiles that never leave the
 *   registers -- the point-dependent part of its exponent is a Gram product on the f64 MFMA units, as is its contraction
 *   with alpha.  Persistent workgroups of 16 points, at most as many as cbfssm_gp_predict_bwd_workgroups names.
 * No atomics, no allocation, no host synchronisation, every output entry has one writer, two calls are bitwise identical,
 * and the results of a point do not depend on the other points of the call; nothing is launched at npts = 0.  Limits as
 * cbfssm_gp_predict_f64 (M <= 320, D <= 24, Do <= 16), else -3 before any launch; NULL layout, pack, mean, fmean, fcov, info
 * or work, or npts < 0: -1.  The count is host arithmetic in 64 bits and returns -1 for a bad layout.
 */
int64_t cbfssm_gp_moment_match_work_elems(const cbfssm_pack_layout* layout);      /* gp_tf.py:132-161 */
int cbfssm_gp_moment_match_f64(const cbfssm_pack_layout* layout, const double* pack, const double* mean, const double* cov,
                               int64_t npts, double* fmean, double* fcov, double* xcov, double* info, double* work, void* stream);

/*
 * The adjoint of cbfssm_gp_moment_match_f64 with respect to the INPUTS of the call, mean and cov; the model (the pack) is a
 * constant.  What planning and policy search through a propagated belief over a fixed, learned model needs.
 *
 * cbfssm_gp_moment_match_bwd_f64: pack, mean, cov as in the forward call; gfmean (npts, Do), gfcov (npts, Do, Do), which need
 *   not be symmetric, and gxcov (npts, Do, D): the cotangents of the three results, each NULL for a zero cotangent (its terms
 *   are skipped; all three NULL: -1) -> gmean (npts, D), gcov (npts, D, D), which is NULL exactly when cov is, and, when the
 *   pointer is not NULL, info (npts) as in the forward.  gcov is the gradient of the function of tril(cov) + tril(cov, -1)^T:
 *   exactly zero above the diagonal (written by the kernel), and a strictly lower entry carries both symmetric contributions.
 *   With cov NULL, gmean is the input gradient of predict.  Where info[n] != 0 the rows of point n of both gradients are NaN,
 *   by select; no other point is affected.  The forward quantities are recomputed: no state of the forward call is needed.
 *   The forward's two pre-kernels (alpha, the W_d tiles) run once per call into `work`
 *   (cbfssm_gp_moment_match_bwd_work_elems doubles: the forward's sections and a scratch per workgroup behind them), then
 *   ONE launch does the rest: per pair of points the forward's factorisations and tile walk, per tile
 *   Qbar = alpha (gfcov + gfcov^T) / 2 alpha^T on the f64 MFMA units less sum_d gfcov_dd W_d, E = Qbar o Q, its row and
 *   column sums and U^T E with the tile as the B operand; then substitutions with the two D x D factors.  No Cholesky
 *   adjoint and no M x M cotangent in memory.
 * No atomics, no allocation, no host synchronisation, every output entry has one writer, every sum over waves in a fixed
 * order: two calls are bitwise identical and the gradient of a point does not depend on the other points of the call;
 * nothing is launched at npts = 0.  Limits as cbfssm_gp_predict_f64 (M <= 320, D <= 24, Do <= 16), else -3 before any
 * launch; NULL layout, pack, mean, gmean or work, no cotangent, gcov without cov or cov without gcov, or npts < 0: -1.  The
 * count is host arithmetic in 64 bits and returns -1 for a bad layout.
 */
int64_t cbfssm_gp_moment_match_bwd_work_elems(const cbfssm_pack_layout* layout);  /* gp_tf.py:132-161 */
int cbfssm_gp_moment_match_bwd_f64(const cbfssm_pack_layout* layout, const double* pack, const double* mean,  /* gp_tf.py:132-161 */
                                   const double* cov, int64_t npts, const double* gfmean, const double* gfcov,
                                   const double* gxcov, double* gmean, double* gcov, double* info, double* work, void* stream);

/*
 * The adjoint of cbfssm_gp_moment_match_f64 with respect to the MODEL: what the five leaves behind the pack receive through
 * alpha = K^-1 mu, W_d, Z / lengthscale, the lengthscales and the variance, as ONE reduced slab in the slab layout of the
 * parameter adjoints of one GP (sections gMu, gS2, gB, gZ; glx, gsig, glogsig; the var_x / var_y entries zero), which
 * cbfssm_gp_tail_f64 (kl_weight 0) takes as it is.
 *
 * cbfssm_gp_moment_match_params_bwd_f64: pack, mean, cov, npts and the three cotangents as in
 *   cbfssm_gp_moment_match_bwd_f64 (each NULL for a zero cotangent, all three NULL: -1); cflat: the constrained flat vector
 *   the pack was prepared from (zeta_pos [M][D] | zeta_mean [M][Do] | zeta_var [M][Do] | variance [1] | lengthscales [D]);
 *   gmean, gcov: the results of cbfssm_gp_moment_match_bwd_f64 for the same call (gcov NULL exactly when cov is) -- the
 *   lengthscales reach the belief only through mean / l, cov / (l l^T) and the scaling of xcov, so the belief's side of their
 *   adjoint is the contraction of the input adjoint with the inputs; xcov: the forward's result, read only with gxcov.
 *   -> red_slab (layout->rev_slab doubles), every entry written, rows and columns >= M exactly zero; gB_dense: the K^-1
 *   adjoint as a row-major [M][M] matrix (hand it to the tail with gB_ld = M), required exactly when layout->rev_stash
 *   (the slab then has no such section), else NULL.  The Z~ section carries the adjoint of Z / lengthscale itself; its ones
 *   column is zero.  A point with a non-positive pivot contributes exact zeros and makes every data entry of the slab and of
 *   gB_dense NaN, by select.
 *   Launches: alpha and (with gfcov) W_d from the dense K^-1; a per-point pass (factorisations, substitutions, the mean-side
 *   terms; t_i = B^-1 r_i, g_i, m~, log c2 and the flag per point into `work`); with gfcov a tile-outer pass -- one
 *   workgroup per 16 x 16 tile of the M x M images and chunk of points, the Do + 1 accumulators of an entry in registers --;
 *   the fixed-order sums; X_d = K^-1 Wbar_d; the slab.  `work`: cbfssm_gp_moment_match_params_bwd_work_elems(layout, npts)
 *   doubles, sized by the launch.
 * No atomics, no allocation, no host synchronisation, one writer per entry, every sum in a fixed order: two calls are
 * bitwise identical; nothing is launched at npts = 0.  Limits as cbfssm_gp_predict_f64 and a layout with an adjoint slab,
 * else -3 before any launch; NULL layout, pack, cflat, mean, gmean, red_slab or work, no cotangent, gcov without cov or cov
 * without gcov, gxcov without xcov, gB_dense against layout->rev_stash, or npts < 0: -1.  The count is host arithmetic in 64
 * bits and returns -1 for a bad layout or npts < 0.
 */
int64_t cbfssm_gp_moment_match_params_bwd_work_elems(const cbfssm_pack_layout* layout, int64_t npts);  /* gp_tf.py:132-161 */
int cbfssm_gp_moment_match_params_bwd_f64(const cbfssm_pack_layout* layout, const double* pack, const double* cflat,  /* gp_tf.py:132-161 */
                                          const double* mean, const double* cov, int64_t npts, const double* gfmean,
                                          const double* gfcov, const double* gxcov, const double* gmean, const double* gcov,
                                          const double* xcov, double* red_slab, double* gB_dense, double* work, void* stream);

/*
 * Assumed-density (moment-matching) Kalman filter over the transition of one sparse GP, and the Rauch-Tung-Striebel
 * smoother behind it: the recursion of cbfssm_gp_ekf_f64 with the exact moments of cbfssm_gp_moment_match_f64 in place of
 * the linearisation at the mean (GP-ADF).  Per chain n and step t, with x = concat(m, a[t]) and S = blockdiag(P, 0):
 *
 *   fmean, fcov, xcov = moment_match(x, S);  Cx = xcov[:, :Do]
 *   m- = m + fmean;  cross[t] = P + Cx;  P- = P + Cx + Cx^T + fcov + diag(var_x);  pmeans[t], pcovs[t] = m-, P-
 *   where cond[t][n] != 0: the Dy scalar updates of cbfssm_gp_ekf_f64;  means[t], covs[t] = m, P = m-, P-
 *
 * cbfssm_gp_adf_f64: the inputs of cbfssm_gp_ekf_f64 -> means, covs, loglik, pmeans (T, N, Do), pcovs, cross (T, N, Do, Do)
 *   and info (N) doubles.  info[n] = 0, or t + 1 of the first step at which a factorisation of chain n met a pivot <= 0,
 *   not finite, or below what a positive semi-definite belief can give (1 for I + S~, 1/2 for I/2 + S~, less rounding) --
 *   P0 not positive semi-definite: from that step on the chain's results and its loglik are NaN, no other
 *   chain is affected.  Every covs[t][n] and pcovs[t][n] is bitwise symmetric; only the lower triangle of P0 is read; a y
 *   entry at cond = 0 is chosen away by a select.  Three launches on one stream: alpha = K^-1 mu and the W_d tiles once per
 *   call in `work` (cbfssm_gp_adf_work_elems doubles: 16 * 16 * NBLK + Do * NBLK^2 * 256), then ONE launch for all steps,
 *   one workgroup per 16 chains.  No atomics, no allocation, no host synchronisation, two calls are bitwise identical, a
 *   chain's results do not depend on the other chains of the call; nothing is launched at N = 0 or T = 0.
 * cbfssm_gp_ads_f64: the same forward pass (its seven results bitwise), then the gain and sweep launches of
 *   cbfssm_gp_eks_f64 on cross[t] = P + Cx -> smeans, scovs, sm_init, sP_init, lag1 (or NULL) as there.  info: the forward
 *   pass's where that is non-zero (the chain's smoothed results are then NaN throughout), else the sweep's.  cross is
 *   workspace here: once the gains are formed its first N entries carry the sweep's info to the kernel that merges the two.
 *
 * Limits and refusals as cbfssm_gp_ekf_f64, the limits first, before any pointer is looked at: -3; NULL layout, pack, m0, y,
 * var_y, work or any output but lag1, NULL a with D > Do, or N, T, Dy < 0: -1.  The count returns -1 for a bad layout.
 */
int64_t cbfssm_gp_adf_work_elems(const cbfssm_pack_layout* layout);      /* gp_tf.py:132-161, cbfssm.py:199-221,245-251 */
int cbfssm_gp_adf_f64(const cbfssm_pack_layout* layout, const double* pack, const double* m0, const double* P0,
                      const double* a, const double* y, const double* cond, const double* var_x, const double* var_y,
                      int Dy, int64_t N, int64_t T, double* means, double* covs, double* loglik, double* pmeans,
                      double* pcovs, double* cross, double* info, double* work, void* stream);
int cbfssm_gp_ads_f64(const cbfssm_pack_layout* layout, const double* pack, const double* m0, const double* P0,
                      const double* a, const double* y, const double* cond, const double* var_x, const double* var_y,
                      int Dy, int64_t N, int64_t T, double* means, double* covs, double* loglik, double* pmeans,
                      double* pcovs, double* cross, double* smeans, double* scovs, double* sm_init, double* sP_init,
                      double* lag1, double* info, double* work, void* stream);

/*
 * The adjoint of cbfssm_gp_adf_f64 with respect to the INPUTS of the call -- m0, P0, a, y, var_x, var_y; the model (the pack)
 * is a constant -- from the cotangents of means, covs and loglik: what optimising an input sequence, an initial belief or
 * the noise levels through a propagated belief over a fixed, learned model needs.
 *
 * cbfssm_gp_adf_bwd_f64: the inputs of the forward call; means, covs, pmeans, pcovs, info as cbfssm_gp_adf_f64 left them (the
 *   forward saves nothing else: the moments of the GP are recomputed); gmeans (T, N, Do), gcovs (T, N, Do, Do), which need
 *   not be symmetric, gloglik (N), each NULL where the loss does not use the result -> gm0 (N, Do), gP0 (N, Do, Do), ga
 *   (T, N, D - Do), gy (T, N, Dy), gvar_x (Do), gvar_y (Dy).  gP0 is the gradient of the function of tril(P0) + tril(P0, -1)^T:
 *   exactly zero above the diagonal (written here), both symmetric contributions on a strictly lower entry; gP0 is NULL
 *   exactly when P0 is, gvar_x exactly when var_x is, ga only when D == Do.  gy is exactly 0 where cond = 0 (a select: y may
 *   be NaN there); cond = 0 everywhere gives zero gy and gvar_y.  Where info[n] != 0 the rows of chain n of gm0, gP0, ga and
 *   gy are NaN, by select, gvar_x and gvar_y are NaN, and the rows of every other chain are unaffected.  On one stream: the
 *   forward's two pre-kernels once per call, ONE launch for all steps in reverse time (one workgroup per 16 chains: the
 *   adjoint of the scalar updates and of the transition on the VALU, then the per-pair body of
 *   cbfssm_gp_moment_match_bwd_f64's kernel on the step's staged problem), and a small launch that adds the workgroups'
 *   var_x / var_y sums in the order of the workgroups.  `work`: cbfssm_gp_adf_bwd_work_elems(layout, N) doubles -- the
 *   forward's sections and a block per workgroup of the launch, ceil(N / 16) of them; nothing of it is read that the call
 *   did not write.  No atomics, no allocation, no host synchronisation; two calls are bitwise identical and a chain's rows
 *   do not depend on the other chains of the call; nothing is launched and nothing written at N = 0 or T = 0.
 *
 * Limits and refusals as cbfssm_gp_adf_f64, the limits first, before any pointer is looked at: -3; NULL layout, pack, m0, y,
 * var_y, a record, gm0, gy, gvar_y or work, NULL a or ga with D > Do, all three cotangents NULL, gP0 without P0 or P0 without
 * gP0, the same for gvar_x and var_x, or N, T, Dy < 0: -1.  The count is host arithmetic in 64 bits and returns -1 for a bad
 * layout or N < 0.
 */
int64_t cbfssm_gp_adf_bwd_work_elems(const cbfssm_pack_layout* layout, int64_t N);  /* gp_tf.py:132-161, cbfssm.py:199-221 */
int cbfssm_gp_adf_bwd_f64(const cbfssm_pack_layout* layout, const double* pack, const double* m0, const double* P0,
                          const double* a, const double* y, const double* cond, const double* var_x, const double* var_y,
                          int Dy, const double* means, const double* covs, const double* pmeans, const double* pcovs,
                          const double* info, const double* gmeans, const double* gcovs, const double* gloglik, int64_t N,
                          int64_t T, double* gm0, double* gP0, double* ga, double* gy, double* gvar_x, double* gvar_y,
                          double* work, void* stream);

/*
 * ---- extended Kalman filter over the transition of ONE sparse GP: a Gaussian belief (m, P) per chain, carried through
 * time by the local linear model above inside the recurrence of CBF-SSM (cbfssm/model/cbfssm.py:199-221) and conditioned
 * on observations of the first Dy state dimensions (cbfssm.py:245-251), y = x[:Dy] + N(0, diag(var_y)).  Forward in time,
 * evaluation only, diagonal q(z).
 *
 *   for t = 0 .. T-1:
 *       x = concat(m, a[t]);  f, fv = GPModel.predict(x);  J = d fmean / d x [:, :Do]            gp_tf.py:132-161
 *       A = I + J;  m- = m + f;  P- = A P A^T + diag(fv + var_x)                                 cbfssm.py:199-206
 *       cond[t, n] != 0, for j = 0 .. Dy-1 in this order:                                        cbfssm.py:212-221,245-251
 *           s = P-[j][j] + var_y[j];  delta = y[t][n][j] - m-[j]
 *           m- += P-[:, j] delta / s;  P-[i][k] -= (P-[i][j] P-[k][j]) / s;  loglik[n] -= (log(2 pi s) + delta^2 / s) / 2
 *       m, P = m-, P-;  means[t][n] = m;  covs[t][n] = P
 *
 * The scalar updates in this order are the joint Kalman update with H = [I_Dy 0], R = diag(var_y), and loglik[n] is
 * sum_t log N(y[t][n]; H m-, H P- H^T + R) over the conditioned steps.
 *
 * cbfssm_gp_ekf_f64 (gp_tf.py:132-161, cbfssm.py:199-221,245-251): pack prepared (diagonal q(z)); m0 (N, Do), P0
 * (N, Do, Do) of which only the lower triangle is read, or NULL = 0, a (T, N, D - Do) or NULL when D == Do, y (T, N, Dy),
 * cond (T, N) doubles 0 / 1 or NULL = condition everywhere, var_x (Do) constrained values or NULL, var_y (Dy) constrained
 * values -> means (T, N, Do), covs (T, N, Do, Do), loglik (N): every entry written once, covs[t][n] bitwise symmetric.
 * The branch is a select: a y entry at cond = 0 may be NaN and reaches no output; cond = 0 everywhere propagates the
 * belief without data (loglik exactly 0).  One pre-kernel forms alpha = K^-1 mu in `work` (cbfssm_gp_ekf_work_elems
 * doubles, as cbfssm_gp_linearize_f64 does), then ONE launch runs all steps, one workgroup per 16 chains, both GP forms
 * (layout->gp_form; A of the two-triangular form through LDS and workgroup barriers, no flag hand-off).
 * No atomics, no allocation, no host synchronisation, two calls are bitwise identical, and the results of a chain do not
 * depend on the other chains of the call; nothing is launched (and nothing written) at N = 0 or T = 0.  Limits as
 * cbfssm_gp_predict_f64 (M <= 320, D <= 24, Do <= 16) plus Do <= D, 1 <= Dy <= Do, N <= 2^30, T <= 2^24, else -3 before any
 * launch; NULL layout, pack, m0, y, var_y, means, covs, loglik or work, NULL a with D > Do, or N, T, Dy < 0: -1.  The
 * count is host arithmetic in 64 bits and returns -1 for a bad layout.
 */
int64_t cbfssm_gp_ekf_work_elems(const cbfssm_pack_layout* layout);      /* gp_tf.py:132-161, cbfssm.py:199-221,245-251 */
int cbfssm_gp_ekf_f64(const cbfssm_pack_layout* layout, const double* pack, const double* m0, const double* P0,
                      const double* a, const double* y, const double* cond, const double* var_x, const double* var_y,
                      int Dy, int64_t N, int64_t T, double* means, double* covs, double* loglik, double* work,
                      void* stream);                                     /* gp_tf.py:132-161, cbfssm.py:199-221,245-251 */

/*
 * ---- Rauch-Tung-Striebel smoother behind that filter: the posterior of every state given ALL observations of its chain.
 * The forward pass is cbfssm_gp_ekf_f64 itself (means, covs, loglik bitwise its results) and leaves in addition
 *
 *   pmeans[t][n] = m-_t,  pcovs[t][n] = P-_t (before conditioning),  cross[t][n] = A_t P_{t-1}  (P_{-1} = P0)
 *
 * then, for t = T-1 .. 0 from (ms_{T-1}, Ps_{T-1}) = (means[T-1], covs[T-1]) copied bitwise:
 *
 *       G_t      = cross[t]^T (P-_t)^-1                  a Cholesky factorisation of P-_t and two triangular solves
 *       ms_{t-1} = m_{t-1} + G_t (ms_t - m-_t)
 *       Ps_{t-1} = P_{t-1} + G_t (Ps_t - P-_t) G_t^T     lower triangle computed and mirrored: bitwise symmetric
 *       lag1[t]  = G_t Ps_t = Cov(x_{t-1}, x_t | y)      when lag1 is not NULL
 *
 * with (m_{t-1}, P_{t-1}) the filtered moments and (m0, P0) at t = 0, so the last iteration gives the smoothed initial
 * belief (sm_init, sP_init).
 *
 * cbfssm_gp_eks_f64 (gp_tf.py:132-161, cbfssm.py:199-221,245-251): the inputs of cbfssm_gp_ekf_f64 -> means, covs, loglik
 * as there; pmeans (T, N, Do), pcovs, cross (T, N, Do, Do); smeans (T, N, Do), scovs (T, N, Do, Do), sm_init (N, Do),
 * sP_init (N, Do, Do), lag1 (T, N, Do, Do) or NULL, info (N) doubles: every entry written once.  info[n] = 0, or t + 1
 * where a pivot of the factorisation of P-_t was <= 0 or not finite (the largest such t; P-_t is positive definite
 * whenever P0 is positive semi-definite and fvar + var_x > 0): that chain's smeans, scovs at times < t, sm_init, sP_init and
 * lag1[<= t] are then NaN, its results at times >= t and every other chain are unaffected, nothing traps.  Four launches on
 * one stream: the alpha pre-kernel (`work`: cbfssm_gp_eks_work_elems doubles), the filter kernel, the gains G_t in
 * parallel over (t, n) -- kept in the output slots of time t - 1 until the sweep has used them -- and the sweep, serial in
 * time, one wave per four chains.  No atomics, no allocation, no host synchronisation, two calls are bitwise identical, and the results of a
 * chain do not depend on the other chains of the call; nothing is launched (and nothing written) at N = 0 or T = 0.  Limits
 * and refusals as cbfssm_gp_ekf_f64, the limits first: -3; NULL layout, pack, m0, y, var_y, work or any output but lag1,
 * NULL a with D > Do, or N, T, Dy < 0: -1.  The count is host arithmetic in 64 bits and returns -1 for a bad layout.
 */
int64_t cbfssm_gp_eks_work_elems(const cbfssm_pack_layout* layout);      /* gp_tf.py:132-161, cbfssm.py:199-221,245-251 */
int cbfssm_gp_eks_f64(const cbfssm_pack_layout* layout, const double* pack, const double* m0, const double* P0,
                      const double* a, const double* y, const double* cond, const double* var_x, const double* var_y,
                      int Dy, int64_t N, int64_t T, double* means, double* covs, double* loglik, double* pmeans,
                      double* pcovs, double* cross, double* smeans, double* scovs, double* sm_init, double* sP_init,
                      double* lag1, double* info, double* work,
                      void* stream);                                     /* gp_tf.py:132-161, cbfssm.py:199-221,245-251 */

/*
 * ---- differentiable GPModel.ekf: what tf.gradients gives a graph that builds the filter above from gp.predict and its
 * Jacobian (gp_tf.py:132-161 differentiated twice in the inputs; cbfssm.py:199-221,245-251), as one adjoint launch.
 *
 * cbfssm_gp_ekf_save_f64: the forward under grad.  cbfssm_gp_ekf_f64 (means, covs, loglik bitwise its results; `work`:
 * cbfssm_gp_ekf_work_elems doubles) which also leaves pmeans (T, N, Do), pcovs, cross (T, N, Do, Do) as cbfssm_gp_eks_f64
 * does, and jac (T, N, Do, Do): J_t[d][i] = d fmean[d] / d x[i] at the input of step t.  No smoother launches.  Refusals as
 * cbfssm_gp_ekf_f64; the four records may not be NULL.
 *
 * cbfssm_gp_ekf_bwd_f64: the adjoint.  pack, m0, P0, a, y, cond, var_x, var_y, Dy as in the forward call; means .. jac as
 * the forward left them; gmeans (T, N, Do), gcovs (T, N, Do, Do), gloglik (N): d loss / d means, covs, loglik, each may
 * be NULL (zero); gcovs need not be symmetric.
 *   -> gm0 (N, Do); gP0 (N, Do, Do) or NULL: the gradient of the function of tril(P0) + tril(P0, -1)^T, exactly zero above
 *      the diagonal; ga (T, N, D - Do); gy (T, N, Dy), exactly 0 where cond = 0 (y may be NaN there);
 *      gpart: cbfssm_gp_ekf_bwd_workgroups slabs of layout->rev_slab doubles ("Slab layout of the parameter adjoints of
 *      one GP"; [0, Do) of its scalars: d / d var_x, [16, 16 + Dy): d / d var_y), with room for CBFSSM_REDUCE_SPLIT more;
 *      work: cbfssm_gp_ekf_bwd_work_elems doubles (always needed); M > 112 (layout->rev_stash): gB_image
 *      ([NBLK][NBLK][4][64], cleared and filled by cbfssm_stash_contract_f64; slot = workgroup * T + step, and one more
 *      slot per workgroup behind them for alpha = K^-1 mu), else it may be NULL.
 * One workgroup per 16 chains, no atomics, no spin waits; two calls are bitwise identical.  Nothing is launched at N = 0
 * or T = 0.  Limits and refusals as cbfssm_gp_ekf_f64 (-3 before any launch: M, D, Do, D < Do, Dy, a layout without an
 * adjoint slab); NULL layout, pack, m0, y, var_y, a record, gm0, gy, gpart or work, NULL a / ga with D > Do: -1.  The counts
 * are host arithmetic in 64 bits and return -1 for a bad layout.
 */
int cbfssm_gp_ekf_save_f64(const cbfssm_pack_layout* layout, const double* pack, const double* m0, const double* P0,
                           const double* a, const double* y, const double* cond, const double* var_x, const double* var_y,
                           int Dy, int64_t N, int64_t T, double* means, double* covs, double* loglik, double* pmeans,
                           double* pcovs, double* cross, double* jac, double* work,
                           void* stream);                                /* gp_tf.py:132-161, cbfssm.py:199-221,245-251 */
int64_t cbfssm_gp_ekf_bwd_workgroups(const cbfssm_pack_layout* layout, int64_t N);              /* tf.gradients of the above */
int64_t cbfssm_gp_ekf_bwd_work_elems(const cbfssm_pack_layout* layout, int64_t N, int64_t T);   /* tf.gradients of the above */
int cbfssm_gp_ekf_bwd_f64(const cbfssm_pack_layout* layout, const double* pack, const double* m0, const double* P0,
                          const double* a, const double* y, const double* cond, const double* var_x, const double* var_y,
                          int Dy, const double* means, const double* covs, const double* pmeans, const double* pcovs,
                          const double* cross, const double* jac, const double* gmeans, const double* gcovs,
                          const double* gloglik, int64_t N, int64_t T, double* gm0, double* gP0, double* ga, double* gy,
                          double* gpart, double* work, double* gB_image,
                          void* stream);                                 /* tf.gradients of gp_tf.py:132-161, cbfssm.py:199-251 */

/*
 * ---- differentiable GP rollout: the time loop of ONE sparse GP with per-chain inputs, and its adjoint.
 * Replaces the loop bodies of Voliro's recognition run (cbfssm/model/voliro.py:139-186: one run from h = 0, backwards in
 * time, GP input (h, u_t, y_t) with a per-particle u_t) and of the free-running transition of a trained CBF-SSM
 * (cbfssm/model/cbfssm.py:199-206,224), which the pass kernels above cannot run: their u / y are shared by the particles.
 *
 *   for t = 0 .. T-1 (reverse != 0: T-1 .. 0):
 *       fmean, fvar = GPModel.predict(concat(h, a[t]))               gp_tf.py:132-161
 *       v = fvar + var_add                                           (var_add NULL: v = fvar)
 *       h = h + fmean + eps[t] sqrt(v);  traj[t] = h                 one normal per chain and step (cbfssm.py:149,209)
 *       entropy += 0.5 sum log(2 pi e v)                             cbfssm.py:154-155, voliro.py:182-183
 *
 * cbfssm_gp_rollout_f64 (voliro.py:139-186, cbfssm.py:199-206,224): h0 (N, Do), a (T, N, Da) with Da = D - Do (NULL when
 * Da = 0), eps (T, N), var_add (Do) constrained values or NULL -> traj (T, N, Do), every entry written once; vsave
 * (T, N, Do) or NULL: v of every step, kept for the adjoint; ent_part: cbfssm_gp_rollout_partials doubles, one partial
 * per 16 chains, whose sum is `entropy`.  One launch, one workgroup per 16 chains, both GP forms (layout->gp_form).
 *
 * cbfssm_gp_rollout_bwd_f64 (voliro.py:139-186, cbfssm.py:199-206,224 differentiated): pack, h0, a, eps, traj, vsave as in / from the forward call,
 * gtraj (T, N, Do) = d loss / d traj, g_ent: ONE double on the device = d loss / d entropy
 *   -> gh0 (N, Do), ga (T, N, Da; NULL when Da = 0): every entry written once;
 *      gpart: cbfssm_gp_rollout_bwd_workgroups slabs of layout->rev_slab doubles ("Slab layout of the parameter adjoints
 *      of one GP" below) with room for CBFSSM_REDUCE_SPLIT more; the d/d var_x entries hold d loss / d var_add by state
 *      dim; cbfssm_reduce_partials_f64 and cbfssm_gp_tail_f64 (kl_weight 0) take them as they are;
 *      M > 112 (layout->rev_stash): work (cbfssm_gp_rollout_bwd_work_elems doubles: the two operand images per
 *      (workgroup, step) slot and the contraction's scratch) and gB_image ([NBLK][NBLK][4][64], cleared by the call) as in
 *      cbfssm_gp_predict_bwd_f64; otherwise both may be NULL.
 * The adjoint recomputes the kernel tile and A2 = K^-1 k of every step (K^-1 contraction, whatever the form of the
 * forward).  No atomics, no host synchronisation; two calls are bitwise identical.  eps has no adjoint.
 * The three counts are host arithmetic: -1 for a bad layout or a negative size.  The calls: NULL pointers and T < 1 -> -1;
 * beyond the limits of cbfssm_gp_predict_f64 (M <= 320, Do <= D <= 24, Do <= 16) or N > 2^30, T > 2^24 -> -3, before
 * any launch.
 */
int64_t cbfssm_gp_rollout_partials(const cbfssm_pack_layout* layout, int64_t N);
int cbfssm_gp_rollout_f64(const cbfssm_pack_layout* layout, const double* pack, const double* h0, const double* a,
                          const double* eps, const double* var_add, int64_t N, int64_t T, int reverse, double* traj,
                          double* vsave, double* ent_part, void* stream);
int64_t cbfssm_gp_rollout_bwd_workgroups(const cbfssm_pack_layout* layout, int64_t N);
int64_t cbfssm_gp_rollout_bwd_work_elems(const cbfssm_pack_layout* layout, int64_t N, int64_t T);
int cbfssm_gp_rollout_bwd_f64(const cbfssm_pack_layout* layout, const double* pack, const double* h0, const double* a,
                              const double* eps, const double* traj, const double* vsave, const double* gtraj,
                              const double* g_ent, int64_t N, int64_t T, int reverse, double* gh0, double* ga,
                              double* gpart, double* work, double* gB_image, void* stream);

/*
 * ---- differentiable GP filter loop: the rollout above with a Gaussian filter update per step and chain behind a mask.
 * The conditioned forward step of CBF-SSM (cbfssm/model/cbfssm.py:185-237) for per-chain inputs, differentiable
 * pseudo-observations and a per-(step, chain) mask: state estimation with a GP transition, warm-up then forecast
 * (cond = 1 on the first K steps), missing observations (cond = 0 where there is no data).
 *
 *   for t = 0 .. T-1 (reverse != 0: T-1 .. 0):
 *       fmean, fvar = GPModel.predict(concat(h, a[t]));  m = h + fmean;  v = fvar + var_x        cbfssm.py:199-206
 *       cond[t, n] != 0:  r = var_y + (k_factor - 1) v;  s = r + v;  k = v / s;  delta = ytilde[t] - m     :212-217
 *                         mu = m + k delta;  sig = (1 - k)^2 v + k^2 r;  h = mu + eps[t] sqrt(sig)         :218-221
 *                         kl += 0.5 (log v - log sig + (sig + (mu - m)^2) / v - 1)                         :232-234
 *       otherwise:        h = m + eps[t] sqrt(v)                                                           :224
 *       traj[t] = h
 *
 * cbfssm_gp_filter_f64 (cbfssm.py:185-237): h0 (N, Do), a (T, N, Da) with Da = D - Do (NULL when Da = 0), ytilde
 * (T, N, Do), cond (T, N) doubles 0 / 1 or NULL = condition everywhere, eps (T, N), var_x (Do) constrained values or
 * NULL, var_y (Do) constrained values, k_factor by value -> traj (T, N, Do), every entry written once; msave, vsave
 * (T, N, Do), or both NULL: m and v of every step, kept for the adjoint; kl_part: cbfssm_gp_filter_partials doubles, one
 * partial per 16 chains, whose sum is `kl` (cbfssm_reduce_partials_f64 with slab 1; NaN when a hand-off poll of the
 * two-triangular form ran out).  The branch is a select: a ytilde entry at cond = 0 may be NaN and reaches no output.
 * One launch, one workgroup per 16 chains, both GP forms (layout->gp_form).  cond = 0 everywhere is
 * cbfssm_gp_rollout_f64 without the entropy.
 *
 * cbfssm_gp_filter_bwd_f64 (cbfssm.py:185-237 differentiated): pack, h0, a, ytilde, cond, eps, var_y, k_factor, traj,
 * msave, vsave as in / from the forward call, gtraj (T, N, Do) = d loss / d traj, g_kl: ONE double on the device =
 * d loss / d kl
 *   -> gh0 (N, Do), ga (T, N, Da; NULL when Da = 0), gytilde (T, N, Do; exactly 0 where cond = 0): every entry written once;
 *      gpart: cbfssm_gp_filter_bwd_workgroups slabs of layout->rev_slab doubles ("Slab layout of the parameter adjoints of
 *      one GP" below) with room for CBFSSM_REDUCE_SPLIT more; the d/d var_x and d/d var_y entries hold d loss / d var_x
 *      and d loss / d var_y by state dim; cbfssm_reduce_partials_f64 and cbfssm_gp_tail_f64 (kl_weight 0) take them as
 *      they are;
 *      M > 112 (layout->rev_stash): work (cbfssm_gp_filter_bwd_work_elems doubles) and gB_image ([NBLK][NBLK][4][64],
 *      cleared by the call) as in cbfssm_gp_rollout_bwd_f64; otherwise both may be NULL.
 * delta, k and sig are recomputed from msave / vsave, the kernel tile and A2 = K^-1 k of every step from the trajectory.
 * No atomics, no host synchronisation; two calls are bitwise identical.  eps, cond and k_factor have no adjoint.
 * Counts and error codes as the rollout's: -1 for a bad layout or a negative size from the three counts; the calls: NULL
 * pointers and T < 1 -> -1; beyond M <= 320, Do <= D <= 24, Do <= 16 or N > 2^30, T > 2^24 -> -3, before any launch.
 */
int64_t cbfssm_gp_filter_partials(const cbfssm_pack_layout* layout, int64_t N);                   /* cbfssm.py:185-237 */
int cbfssm_gp_filter_f64(const cbfssm_pack_layout* layout, const double* pack, const double* h0, const double* a,
                         const double* ytilde, const double* cond, const double* eps, const double* var_x,
                         const double* var_y, double k_factor, int64_t N, int64_t T, int reverse, double* traj,
                         double* msave, double* vsave, double* kl_part, void* stream);           /* cbfssm.py:185-237 */
int64_t cbfssm_gp_filter_bwd_workgroups(const cbfssm_pack_layout* layout, int64_t N);             /* cbfssm.py:185-237 */
int64_t cbfssm_gp_filter_bwd_work_elems(const cbfssm_pack_layout* layout, int64_t N, int64_t T);  /* cbfssm.py:185-237 */
int cbfssm_gp_filter_bwd_f64(const cbfssm_pack_layout* layout, const double* pack, const double* h0, const double* a,
                             const double* ytilde, const double* cond, const double* eps, const double* var_y,
                             double k_factor, const double* traj, const double* msave, const double* vsave,
                             const double* gtraj, const double* g_kl, int64_t N, int64_t T, int reverse, double* gh0,
                             double* ga, double* gytilde, double* gpart, double* work, double* gB_image,
                             void* stream);                                                      /* cbfssm.py:185-237 */

/*
 * ---- Voliro's forward filter run: the rigid-body time loop and its adjoint.
 * Replaces _forward / _forward_body / symplectic_euler of the reference's fourth model (cbfssm/model/voliro.py:188-242,
 * 314-338 with cbfssm/utils/quaternions.py), for S = T - 1 steps and N = B * samples chains:
 *
 *   q = var_x (13), r = var_y (13) constrained values,  k = q / (q + r),  sig = (1-k)^2 q + k^2 r        (loop invariant)
 *   x = x0
 *   for t = 0 .. S-1:
 *       f   = symplectic_euler(x, u[t])       rot_vec(u[:3], rot), rot_vec(inertia_inv * u[3:], rot), linvel += (mass_inv
 *                                             f_glob + gravity) dt, angvel += t_glob dt, pos += linvel dt,
 *                                             rot += 0.5 (0, angvel) (x) rot dt, rot /= |rot|
 *       mu  = f + k (y[t] - f)
 *       x   = mu + eps[t] sqrt(sig);  traj[t] = x                     one normal per chain and step (voliro.py:233)
 *       kl += 0.5 sum_d (log q - log sig + (sig + (mu - f)^2) / q - 1)                              voliro.py:238-239
 *
 * State layout: pos 0:3, quaternion 3:7 (scalar first, the product of quaternions.py:8-13), linvel 7:10, angvel 10:13.
 * The physical constants are host values in a cbfssm_rigid_body, passed by pointer and read before the call returns.
 *
 * cbfssm_rigid_filter_f64 (voliro.py:188-242,314-338): x0 (N, 13), u (S, N, 6), y (S, N, 13), eps (S, N), var_x, var_y (13)
 *   -> traj (S, N, 13), every entry written exactly once; kl_part: cbfssm_rigid_filter_partials(N) doubles, one partial
 *      per workgroup of 64 chains, with room for CBFSSM_REDUCE_SPLIT more: cbfssm_reduce_partials_f64(kl_part, 1, n, out)
 *      sums them to `kl`.  One launch, one lane per chain.
 *
 * cbfssm_rigid_filter_bwd_f64 (voliro.py:188-242,314-338 differentiated): body, x0, u, y, eps, var_x, var_y as in, traj from,
 * the forward call; gtraj (S, N, 13) = d loss / d traj; g_kl: ONE double on the device = d loss / d kl
 *   -> gx0 (N, 13), gu (S, N, 6), gy (S, N, 13): every entry written once, no read of their prior content;
 *      gpart: cbfssm_rigid_filter_partials(N) slabs of 32 doubles [d/d var_x (13) | d/d var_y (13) | padding], with room
 *      for CBFSSM_REDUCE_SPLIT more; cbfssm_reduce_partials_f64(gpart, 32, n, out) sums them.  The 26 numbers include the
 *      data-independent part of the KL (N S g_kl d/d(q, r) of 0.5 sum (log q - log sig + sig / q - 1)) and the
 *      eps d sqrt(sig) path.
 * The reverse sweep recomputes every step's f from traj[t-1] (x0 at t = 0) and u[t]: nothing is saved except the
 * trajectory.  No atomics, no allocation, no synchronisation; two calls are bitwise identical.  eps has no adjoint.
 * cbfssm_rigid_filter_partials is host arithmetic: ceil(N / 64), -1 for N < 0 (or N > 2^30).  The calls: NULL pointers,
 * N < 0 or S < 1 -> -1; N > 2^30 or S > 2^24 -> -3; both decided on the host before any launch.  N = 0 launches nothing.
 */
typedef struct cbfssm_rigid_body {
    double mass_inv;
    double inertia_inv[3];
    double gravity[3];
    double dt;
} cbfssm_rigid_body;
int64_t cbfssm_rigid_filter_partials(int64_t N);
int cbfssm_rigid_filter_f64(const cbfssm_rigid_body* body, const double* x0, const double* u, const double* y,
                            const double* eps, const double* var_x, const double* var_y, int64_t N, int64_t S,
                            double* traj, double* kl_part, void* stream);
int cbfssm_rigid_filter_bwd_f64(const cbfssm_rigid_body* body, const double* x0, const double* u, const double* y,
                                const double* eps, const double* var_x, const double* var_y, const double* traj,
                                const double* gtraj, const double* g_kl, int64_t N, int64_t S, double* gx0, double* gu,
                                double* gy, double* gpart, void* stream);

/*
 * Both backward (recognition) runs, CBFSSM._backward/_backward_run/_backward_body (cbfssm.py:84-158).
 *   u (B,T,dim_u), y (B,T,dim_y), hid_b (2,T,N), eps_b (2,T,N), var_x (dim_x)
 *   -> y2 (T,N,dim_x-dim_y)  [every t written by exactly one run, cbfssm.py:123-128,151]
 *      h_all (2,T,N,dim_x-dim_y) or NULL: every step's output of both runs (kept for the adjoint)
 *      fmv_b (2,T,N,dim_x-dim_y,2) or NULL: every step's (fmean, fvar) after residual and process noise (kept for
 *      the adjoint, which then needs no recomputation of the predictive products)
 *      a2s_b (cbfssm_saved_a2_elems(p, L, 1) doubles) or NULL: every step's A2 = K_mm^-1 K_mn tiles -- and, for tile
 *      heights up to seven row blocks (M <= 112), its kernel tile K_mn next to it -- kept for the adjoint (which
 *      otherwise recomputes them: one M x M x 16 product, resp. the kernel tile's MFMAs and exponentials, per step less)
 *      ent_part (n_ent_part doubles): per-workgroup partial sums of 0.5*sum(log(2 pi e) + log fvar) over the
 *      written steps (cbfssm.py:154-156); their sum is `entropy` (cbfssm.py:99).
 *   cbfssm_backward_pass_partials(problem) gives n_ent_part.
 */
int64_t cbfssm_backward_pass_partials(const cbfssm_problem* p);
int cbfssm_backward_pass_f64(const cbfssm_problem* p, const cbfssm_pack_layout* layout_b, const double* pack_b,
                             const double* var_x, const double* u, const double* y, const double* hid_b,
                             const double* eps_b, double* y2, double* h_all, double* fmv_b, double* a2s_b,
                             double* ent_part, void* stream);

/*
 * Forward (filter) pass, CBFSSM._forward/_forward_body (cbfssm.py:160-237).
 *   y2 (T,N,dim_x-dim_y) from the backward pass, eps_f (T-1,N), var_x (dim_x), var_y (dim_x)
 *   -> x (T,N,dim_x)   [x[0] = y_tilde[0], cbfssm.py:168]
 *      fmv_f (T-1,N,dim_x,2) or NULL: every step's (fmean, fvar), kept for the adjoint
 *      a2s_f (cbfssm_saved_a2_elems(p, L, 0) doubles) or NULL: every step's A2 (and, M <= 112, kernel) tiles, kept
 *      for the adjoint
 *      kl_part (n_kl_part doubles): per-workgroup partial sums of kl_reg (cbfssm.py:232-235); sum = kl_x.
 */
int64_t cbfssm_forward_pass_partials(const cbfssm_problem* p);

/* Doubles in the optional saved-tile buffer of the backward (backward != 0) or forward pass: one record per step and
 * 16-chain group, T*2 resp. T-1 steps; a record is the M_pad x 16 tile A2 and, when M <= 112, the kernel tile K_mn of
 * the same shape behind it.  The buffer is opaque to the caller: the passes write it, their adjoints read it (no
 * reference counterpart: TF keeps its forward activations for tf.gradients the same way, base_model.py:34-36). */
int64_t cbfssm_saved_a2_elems(const cbfssm_problem* p, const cbfssm_pack_layout* layout, int backward);
int cbfssm_forward_pass_f64(const cbfssm_problem* p, const cbfssm_pack_layout* layout_f, const double* pack_f,
                            const double* var_x, const double* var_y, const double* u, const double* y,
                            const double* y2, const double* eps_f, double* x, double* fmv_f, double* a2s_f,
                            double* kl_part, void* stream);

/*
 * CBFSSMHALF (cbfssm/model/cbfssmhalf.py:97-172): the forward pass with x_0 = recognition-model output x0 (B,dim_x),
 * Kalman update on the first dim_y state dims only (var_y has dim_y entries), no backward runs.  problem->half must be 1.
 * The adjoint also returns gx0 (N,dim_x) = d loss / d x_0 per particle chain (sum over the S particles of a sequence is
 * the gradient of the recognition output).  t range / stash arguments as in cbfssm_forward_pass_bwd_ex_f64.
 */
int cbfssm_half_forward_pass_f64(const cbfssm_problem* p, const cbfssm_pack_layout* layout_f, const double* pack_f,
                                 const double* var_x, const double* var_y, const double* u, const double* y,
                                 const double* x0, const double* eps_f, double* x, double* fmv_f, double* a2s_f,
                                 double* kl_part, void* stream);
int cbfssm_half_forward_pass_bwd_f64(const cbfssm_problem* p, const cbfssm_pack_layout* layout_f, const double* pack_f,
                                     const double* var_x, const double* var_y, const double* u, const double* y,
                                     const double* eps_f, const double* x, const double* fmv_f, const double* a2s_f, double cL,
                                     double* gx0, double* gpart, int t_hi, int t_lo, double* gx_carry, double* stash_a,
                                     double* stash_k, int64_t stash_ld, void* stream);

/*
 * Log-likelihood and predictive moments, CBFSSM._build_loss (cbfssm.py:245-251) and _build_prediction
 * (cbfssm.py:264-269).
 *   x (T,N,dim_x), y (B,T,dim_y), var_y (dim_x)
 *   -> ll_part (cbfssm_loglik_partials(problem) doubles, laid out [block][dim_y]: per-workgroup, per-dimension partial
 *      sums of the log-likelihood in a fixed order; their total is `loglik`, their per-dimension totals drive the
 *      gradient with respect to var_y), pred_mean (B,T,dim_y), pred_var (B,T,dim_y),
 *      int_mean (B,T,dim_x) / int_var (B,T,dim_x) or NULL.
 */
int64_t cbfssm_loglik_partials(const cbfssm_problem* p);
int cbfssm_loglik_moments_f64(const cbfssm_problem* p, const double* var_y, const double* y, const double* x,
                              double* ll_part, double* pred_mean, double* pred_var, double* int_mean,
                              double* int_var, void* stream);

/*
 * ELBO combination, CBFSSM._build_loss (cbfssm.py:257-262): deterministic sums of the partial buffers.
 *   out[0..7] = loglik, kl_x, entropy, kl_z_f, kl_z_b, elbo, loss, info (max of the two packs' info).
 */
int cbfssm_elbo_combine_f64(const cbfssm_problem* p, double lambda0, double lambda1,
                            const double* ll_part, int64_t n_ll, const double* kl_part, int64_t n_kl,
                            const double* ent_part, int64_t n_ent, const double* scal_f, const double* scal_b,
                            double* out, void* stream);

/*
 * ---- adjoint (reverse-mode) entry points: what tf.train.AdamOptimizer.minimize differentiates (cbfssm.py:273-275).
 *
 * Slab layout of the parameter adjoints of one GP (layout->rev_slab doubles; C = MFMA accumulator layout,
 * element [blk][r][lane] -> row 16*blk_row + (lane>>4) + 4r, col 16*blk_col + (lane&15)):
 *   [0, NBLK*256)                       d loss / d zeta_mean   (Mp x 16)
 *   [NBLK*256, 2*NBLK*256)              d loss / d zeta_var    (Mp x 16)
 *   then NBLK*NBLK*256                  d loss / d K^-1        (Mp x Mp), data terms only
 *   then NBLK*JB*256                    d loss / d (Z/ls)      (Mp x 16*JB): column D holds the row sums of Ebar,
 *                                       the caller subtracts (Z/ls) o rowsum
 *   then 128 scalars: [0,16) d/d var_x (by state dim), [16,32) d/d var_y, [32,32+16*JB) sum_n xbar~ x~ by input
 *                     row (lengthscale adjoint of the inputs), [96] d/d sigma^2 (direct), [97] d/d log sigma^2
 */
int64_t cbfssm_rev_workgroups(const cbfssm_problem* p, int backward_runs);

/*
 * The schedule of the backward-run adjoint (host only, no GPU work): the live steps of both runs cut into chunks of
 * consecutive whole resample-to-resample segments, in launch order.  Run 0 is live on t = 0 .. T-1; run 1 from
 * t = recog_len (its segment t = recog_len-1 .. 0 reaches nothing the loss sees, cbfssm.py:112,123-128; no live step for
 * T <= recog_len): the backward-pass kernels skip it and leave those rows of h_all, fmv_b and a2s_b unwritten.
 * Entry i is nsteps[i] steps from t_begin[i] upwards of run[i]; every live step is in exactly one entry, nsteps is
 * non-increasing and the table ends on single segments.  A function of (T, recog_len, B*S) only: group0 / ngroups do
 * not enter.  Returns the number of entries (at most 32) and fills the arrays when they are given (cap: their
 * length); cbfssm_rev_workgroups(p, 1) is that count times the chain groups.
 */
int cbfssm_bwd_schedule(const cbfssm_problem* p, int cap, int* run, int* t_begin, int* nsteps);

/*
 * Adjoint of cbfssm_forward_pass_f64 (reverse of the tf.while_loop in CBFSSM._forward, cbfssm.py:176-237) including
 * the log-likelihood's pull on x (cbfssm.py:245-251).
 *   x, y2, eps_f, fmv_f (and a2s_f, or NULL to recompute A2) as saved by the forward evaluation; cL = loss_factors[0]/S.
 *   -> gy2 (T,N,dim_x-dim_y): d loss / d y2 ; gpart: cbfssm_rev_workgroups(p,0) slabs of layout_f->rev_slab doubles.
 */
int cbfssm_forward_pass_bwd_f64(const cbfssm_problem* p, const cbfssm_pack_layout* layout_f, const double* pack_f,
                                const double* var_x, const double* var_y, const double* u, const double* y,
                                const double* y2, const double* eps_f, const double* x, const double* fmv_f,
                                const double* a2s_f, double cL, double* gy2, double* gpart, void* stream);

/*
 * Adjoint of cbfssm_backward_pass_f64 (both runs; reverse of the tf.while_loops in CBFSSM._backward_run,
 * cbfssm.py:107-158).  h_all, fmv_b (and a2s_b, or NULL) as saved by the forward evaluation, gy2 from cbfssm_forward_pass_bwd_f64,
 * cE = loss_factors[1]/S.  -> gpart: cbfssm_rev_workgroups(p,1) slabs of layout_b->rev_slab doubles.
 */
int cbfssm_backward_pass_bwd_f64(const cbfssm_problem* p, const cbfssm_pack_layout* layout_b, const double* pack_b,
                                 const double* var_x, const double* u, const double* y, const double* hid_b,
                                 const double* eps_b, const double* h_all, const double* fmv_b, const double* a2s_b,
                                 const double* gy2, double cE, double* gpart, void* stream);

/*
 * General forms of the two adjoint passes: a time range per launch, and "stash mode" for tile heights whose
 * K^-1-adjoint accumulator does not fit the VGPR file (layout->rev_stash == 1, M > 112; the slab then has no
 * d/dK^-1 block).  In stash mode every step writes the two MFMA operand images of d loss / d K^-1 += A2bar K^T to
 * stash_a / stash_k: [slot][NBLK][4][64] doubles each, slot = workgroup * steps_per_workgroup + step, stash_ld = 16 x
 * (slots the buffer can hold) -- "columns" below are 16 per slot -- and cbfssm_stash_contract_f64 contracts them after
 * the launch.
 *   forward:  steps t = t_hi .. t_lo (descending; full pass: T-2 .. 0).  A launch that does not start at T-2 reads the
 *             adjoint of x_{t_hi+1} from gx_carry (N,dim_x); a launch that does not end at 0 writes it there.
 *             columns used: groups * (t_hi - t_lo + 1) * 16.
 *   backward: resample-to-resample segments [seg0, seg1) of both runs (cbfssm_bwd_segments(p) in total), split over
 *             nchunk <= 16 independent workgroup sets per run.  The dead steps t < recog_len of run 1 are left out
 *             (their stash slots read as zeros).  gpart: groups * 2 * nchunk slabs.
 *             columns used: groups * 2 * nchunk * ceil((seg1-seg0)/nchunk) * 2*recog_len * 16.
 *             nchunk = 0 with the whole range [0, cbfssm_bwd_segments(p)): the table of cbfssm_bwd_schedule, as
 *             cbfssm_backward_pass_bwd_f64 runs it (cbfssm_rev_workgroups(p,1) slabs; not in stash mode).
 */
int cbfssm_bwd_segments(const cbfssm_problem* p);
int cbfssm_forward_pass_bwd_ex_f64(const cbfssm_problem* p, const cbfssm_pack_layout* layout_f, const double* pack_f,
                                   const double* var_x, const double* var_y, const double* u, const double* y,
                                   const double* y2, const double* eps_f, const double* x, const double* fmv_f,
                                   const double* a2s_f, double cL, double* gy2, double* gpart, int t_hi, int t_lo,
                                   double* gx_carry, double* stash_a, double* stash_k, int64_t stash_ld, void* stream);
int cbfssm_backward_pass_bwd_ex_f64(const cbfssm_problem* p, const cbfssm_pack_layout* layout_b, const double* pack_b,
                                    const double* var_x, const double* u, const double* y, const double* hid_b,
                                    const double* eps_b, const double* h_all, const double* fmv_b, const double* a2s_b,
                                    const double* gy2, double cE, double* gpart, int seg0, int seg1, int nchunk,
                                    double* stash_a, double* stash_k, int64_t stash_ld, void* stream);

/*
 * ---- input gradients: d loss / d u (B,T,dim_u) and d loss / d y (B,T,dim_y).  Replaces tf.gradients(model.loss,
 * model.sample_in) and tf.gradients(model.loss, model.sample_out), i.e. the gradient of the loss with respect to the
 * placeholders of base_model.py:22-27, which the reference's graph gives for free (cbfssm/model/voliro.py:106-137 trains
 * through it).  CBFSSM, float64 only.
 *
 * The `_in` forms of the two adjoint passes take the arguments of the `_ex` forms plus per-chain output buffers, and run
 * instantiations of the adjoint kernel that multiply every 16-row block of the input adjoint again (the default ones keep
 * only the state rows).  The parameter slabs are written as by the `_ex` forms (same layout; the lengthscale adjoint of the
 * input rows j >= 16 is accumulated per step instead of rebuilt, so it agrees to rounding, not bitwise).  Every launch
 * writes the entries of its own time range and chain groups only; entries of padded chains do not exist.
 *   gin_f (cbfssm_input_adjoint_fwd_elems doubles, (T-1, dim_u, N)): adjoint of the scaled u rows of gp_f's input, steps 0 .. T-2
 *   gyo   (cbfssm_input_adjoint_obs_elems doubles, (T, dim_y, N)):   adjoint of the observed dimensions of y_tilde[t]
 *                                                                    (t = 0: of x_0 = y_tilde[0])
 *   gin_b (cbfssm_input_adjoint_bwd_elems doubles, (2, T, dim_u+dim_y, N)): adjoint of the scaled u and y rows of gp_b's
 *                                                                    input, per run and step (both runs evaluate gp_b at every t)
 * cbfssm_input_grads_f64: one launch, after both adjoints are complete: sums the S particles of a sequence in particle
 * order, then forward pass + run 0 + run 1, scales each row by 1/lengthscale of its GP and row (from the packs), and adds
 * to d loss / d y the log-likelihood's direct term cL sum_s (y - x) / var_y (cbfssm.py:245-251; x: the trajectory
 * cbfssm_loglik_moments_f64 reads).  Fixed order, no atomics: two evaluations are bitwise identical.
 */
int64_t cbfssm_input_adjoint_fwd_elems(const cbfssm_problem* p);
int64_t cbfssm_input_adjoint_bwd_elems(const cbfssm_problem* p);
int64_t cbfssm_input_adjoint_obs_elems(const cbfssm_problem* p);
int cbfssm_forward_pass_bwd_in_f64(const cbfssm_problem* p, const cbfssm_pack_layout* layout_f, const double* pack_f,
                                   const double* var_x, const double* var_y, const double* u, const double* y,
                                   const double* y2, const double* eps_f, const double* x, const double* fmv_f,
                                   const double* a2s_f, double cL, double* gy2, double* gpart, int t_hi, int t_lo,
                                   double* gx_carry, double* stash_a, double* stash_k, int64_t stash_ld, double* gin_f,
                                   double* gyo, void* stream);
int cbfssm_backward_pass_bwd_in_f64(const cbfssm_problem* p, const cbfssm_pack_layout* layout_b, const double* pack_b,
                                    const double* var_x, const double* u, const double* y, const double* hid_b,
                                    const double* eps_b, const double* h_all, const double* fmv_b, const double* a2s_b,
                                    const double* gy2, double cE, double* gpart, int seg0, int seg1, int nchunk,
                                    double* stash_a, double* stash_k, int64_t stash_ld, double* gin_b, void* stream);
int cbfssm_input_grads_f64(const cbfssm_problem* p, const cbfssm_pack_layout* layout_f, const double* pack_f,
                           const cbfssm_pack_layout* layout_b, const double* pack_b, const double* var_y, const double* y,
                           const double* x, const double* gin_f, const double* gin_b, const double* gyo, double cL,
                           double* grad_u, double* grad_y, void* stream);

/* out[i] = sum over the nwg slabs, in a fixed order (bitwise reproducible).  gpart must have room for
 * nwg + CBFSSM_REDUCE_SPLIT slabs: the tail is scratch for the first of the two reduction stages. */
#define CBFSSM_REDUCE_SPLIT 32
int cbfssm_reduce_partials_f64(double* gpart, int64_t slab, int64_t nwg, double* out, void* stream);

/*
 * Stash mode (layout->rev_stash, M > 112): the `*_bwd_ex_f64` launches write, per (workgroup, step) slot, the two MFMA
 * operand images of  d loss / d K^-1 += A2bar K^T  (stash_a: A2bar^T, stash_k: K^T; [slot][NBLK][4][64] doubles each, i.e.
 * 16 NBLK x stash_ld doubles per buffer with stash_ld = 16 x slots).  This contracts `nslots` slots and ADDS the SYMMETRIC
 * PART of the result, (B + B^T) / 2 with B = sum A2bar K^T, to ginv_image, an MFMA C-layout image [NBLK][NBLK][4][64] (the
 * layout of the in-register variant's slab section; row = 16 rb + (lane >> 4) + 4 r, column = 16 cb + (lane & 15)).  The
 * symmetric part is all the train tail uses (d loss / d K_mm = -K^-1 (.) K^-1 contracted with a symmetric dK_mm/dtheta), and
 * it halves the accumulator: the kernel holds the lower-triangular blocks of A2bar K^T + K A2bar^T only (cbfssm_contract.hip).
 * CBFSSM_CONTRACT_FULL=1 (measurement switch) adds B itself.  work: cbfssm_stash_contract_work_elems doubles.
 */
int64_t cbfssm_stash_contract_work_elems(const cbfssm_pack_layout* layout, int64_t nslots);
int cbfssm_stash_contract_f64(const cbfssm_pack_layout* layout, const double* stash_a, const double* stash_k, int64_t nslots,
                              double* work, double* ginv_image, void* stream);

/*
 * float32-ARITHMETIC variant of the forward evaluation and of the adjoint (BASELINE.json configs[4]; the reference's model dtype argument,
 * cbfssm.py:12: `CBFSSM(config, dtype=tf.float32)`).  As in the reference's float32 mode the Cholesky of K_mm is computed
 * in float64 and cast (gp_tf.py:57-65): the operands are the float64 pack of cbfssm_gp_prepare_f64 re-packed as float32
 * MFMA images; kernel tile, exp, the K^-1 K contraction (v_mfma_f32_16x16x4_f32) and the step epilogues are float32.
 * Storage stays float64: u, y, noise, trajectories and partial sums are the buffers of the float64 entry points.
 *   cbfssm_pack_f32_elems   floats of a float32 pack for this layout (host)
 *   cbfssm_gp_pack_f32      float64 pack -> float32 pack (after every cbfssm_gp_prepare*_f64)
 *   cbfssm_gp_predict_f32   GPModel.predict (gp_tf.py:132-161)
 *   cbfssm_backward_pass_f32 / cbfssm_forward_pass_f32   CBFSSM._backward / _forward (cbfssm.py:84-237); the partial-sum
 *                           buffers have cbfssm_backward_pass_partials / cbfssm_forward_pass_partials entries; feed
 *                           cbfssm_loglik_moments_f64 and cbfssm_elbo_combine_f64 as usual.
 *   cbfssm_gp_pack_bf16     the same pack with the K^-1 operand rounded to bfloat16; the _f32 passes given such a pack
 *                           also round the kernel tile to bfloat16, i.e. they evaluate the K^-1 K contraction with
 *                           bf16 operands and float32 accumulation (on the float32 MFMA: bf16 x bf16 products are exact in
 *                           float32).  A precision probe for the fp32-vs-bf16 tolerance sweep, not a throughput path.
 *   fmv_* / h_all (may be NULL): what the float32 adjoint below reads of the forward evaluation -- every step's
 *                           (fmean, fvar) and, for the backward runs, every step's output -- in the float64 buffers of
 *                           cbfssm_backward_pass_f64 / cbfssm_forward_pass_f64 (same layout; float32 values).
 *
 * float32 ADJOINT (what `minimize` differentiates when the model dtype is float32, cbfssm.py:12,273-275): the reverse
 * sweeps on v_mfma_f32_16x16x4_f32 with float32 accumulation over the time steps; the kernel tile and A2 = K^-1 k are
 * read back when the passes kept them (a2s_*), recomputed otherwise.  The partial slabs leave as float64 in the layout of the float64 adjoint for NON-stash tile
 * heights -- [mubar | s2bar | G (NBLK x NBLK C-layout images) | Zbar | small] = cbfssm_rev32_slab_elems doubles per
 * workgroup, cbfssm_rev_workgroups workgroups -- so cbfssm_reduce_partials_f64 and cbfssm_train_tail_f64 (the K_mm ->
 * Cholesky -> K^-1 adjoint stays float64, as the reference keeps the Cholesky in float64, gp_tf.py:57-65) take them, with ONE
 * difference: the matrix section holds G = sum (K^-1 A2bar) A2^T = K^-1 (d loss / d K^-1) K^-1, the data part of the K_mm
 * adjoint itself (a float32 accumulator of d loss / d K^-1 would have its rounding multiplied by K^-1 from both sides in the
 * tail).  cbfssm_train_tail_g_f64 takes the section as it is: g_mode = 1 for tile heights up to 10 row blocks (the full
 * matrix G), g_mode = 2 from 13 row blocks (M > 160: two row blocks per wave) -- there the kernel accumulates only the
 * lower-triangular 16 x 16 blocks of S = C A2^T + A2 C^T, C = K^-1 A2bar (diagonal blocks: C A2^T; blocks above the diagonal
 * are never written), the symmetric part (S + S^T) / 2 of G being all that d loss / d K_mm uses: one pass over the time loop at
 * every tile height.  For tile heights above 112 rows hand that section to the tail as gB_dense_* with gB_ld = 0.
 */
int64_t cbfssm_pack_f32_elems(const cbfssm_pack_layout* layout);
int cbfssm_gp_pack_f32(const cbfssm_pack_layout* layout, const double* pack, float* pack32, void* stream);
int cbfssm_gp_pack_bf16(const cbfssm_pack_layout* layout, const double* pack, float* pack32, void* stream);
int cbfssm_gp_predict_f32(const cbfssm_pack_layout* layout, const float* pack32, const double* X, int64_t npts,
                          double* fmean, double* fvar, void* stream);
int cbfssm_backward_pass_f32(const cbfssm_problem* p, const cbfssm_pack_layout* layout_b, const float* pack32_b,
                             const double* var_x, const double* u, const double* y, const double* hid_b,
                             const double* eps_b, double* y2, double* h_all, double* fmv_b, float* a2s_b, double* ent_part,
                             void* stream);
int cbfssm_forward_pass_f32(const cbfssm_problem* p, const cbfssm_pack_layout* layout_f, const float* pack32_f,
                            const double* var_x, const double* var_y, const double* u, const double* y,
                            const double* y2, const double* eps_f, double* x, double* fmv_f, float* a2s_f, double* kl_part,
                            void* stream);
/* a2s_*: NULL, or cbfssm_saved_a2_f32_elems floats -- every step's [A2 | kernel tile] accumulator registers, kept for the float32
 * adjoint, which then reads them back instead of recomputing the kernel tile and the K^-1 K product (2 F instead of 3 F per GP
 * evaluation; C3: 3.4 GB for both GPs).  Opaque to the host. */
int64_t cbfssm_saved_a2_f32_elems(const cbfssm_problem* p, const cbfssm_pack_layout* layout, int backward_runs);
/* The forward pass of the forward-only variants (problem->half = 1: x_0 from the recognition model, Kalman update on the observed
 * dims only; cbfssmhalf.py:117-172, prssm.py:96-118) in float32 arithmetic, and its adjoint (-> gx0 (N, dim_x): d loss / d x_0
 * per chain): the float32 counterparts of cbfssm_half_forward_pass_f64 / _bwd_f64. */
int cbfssm_half_forward_pass_f32(const cbfssm_problem* p, const cbfssm_pack_layout* layout_f, const float* pack32_f,
                                 const double* var_x, const double* var_y, const double* u, const double* y,
                                 const double* x0, const double* eps_f, double* x, double* fmv_f, float* a2s_f,
                                 double* kl_part, void* stream);
int cbfssm_half_forward_pass_bwd_f32(const cbfssm_problem* p, const cbfssm_pack_layout* layout_f, const float* pack32_f,
                                     const double* var_x, const double* var_y, const double* u, const double* y,
                                     const double* eps_f, const double* x, const double* fmv_f, const float* a2s_f, double cL,
                                     double* gx0, double* gpart, void* stream);
int64_t cbfssm_rev32_slab_elems(const cbfssm_pack_layout* layout);
int cbfssm_forward_pass_bwd_f32(const cbfssm_problem* p, const cbfssm_pack_layout* layout_f, const float* pack32_f,
                                const double* var_x, const double* var_y, const double* u, const double* y,
                                const double* y2, const double* eps_f, const double* x, const double* fmv_f, const float* a2s_f,
                                double cL, double* gy2, double* gpart, void* stream);
int cbfssm_backward_pass_bwd_f32(const cbfssm_problem* p, const cbfssm_pack_layout* layout_b, const float* pack32_b,
                                 const double* var_x, const double* u, const double* y, const double* hid_b,
                                 const double* eps_b, const double* h_all, const double* fmv_b, const float* a2s_b,
                                 const double* gy2, double cE, double* gpart, void* stream);

/*
 * ---- once-per-step tail of a train step ------------------------------------------------------------------------------
 * The twelve trainable tensors of CBFSSM._setup_vars (cbfssm.py:30-58) as ONE flat float64 vector, in this order:
 *   f.zeta_pos (M,D) f.zeta_mean (M,dim_x) f.zeta_var_unc (M,dim_x) f.variance_unc (1) f.lengthscales_unc (D)
 *   b.zeta_pos (M,D) b.zeta_mean (M,dob)   b.zeta_var_unc (M,dob)   b.variance_unc (1) b.lengthscales_unc (D)
 *   var_x_unc (dim_x) var_y_unc (dim_x)                      D = dim_x + dim_u, dob = dim_x - dim_y
 */
typedef struct cbfssm_param_layout {
    int64_t off[12];
    int64_t total;
    int32_t M, D, dim_x, dim_y;
} cbfssm_param_layout;

int cbfssm_param_layout_init(int M, int dim_x, int dim_u, int dim_y, cbfssm_param_layout* out);

/* Positivity transform softplus(x) + 1e-10 of every *_unc tensor (tf_transform.py:19-21); the other tensors are copied.
 * cflat has the layout of pflat. */
int cbfssm_constrain_f64(const cbfssm_param_layout* pl, const double* pflat, double* cflat, void* stream);

/* Scratch doubles cbfssm_train_tail_f64 needs. */
int64_t cbfssm_train_tail_work_elems(const cbfssm_pack_layout* layout_f, const cbfssm_pack_layout* layout_b);

/*
 * What tf.gradients (base_model.py:34-36) does after the time loops: the adjoint of GPModel.__init__ / prior_kl
 * (K_mm -> Cholesky -> K^-1, gp_tf.py:33-65,129-130,163-172) for gp_f and gp_b from the reduced adjoint slabs, and the
 * chain through the positivity transforms.  red = [slab_f | slab_b | loglik, kl_x, entropy, dloss/dvar_y[dim_y]] as
 * produced by cbfssm_reduce_partials_f64 (summed over the ranks for a multi-GPU step); gB_dense_*: the K^-1 adjoints
 * of stash mode (M > 112), NULL otherwise -- dense [.][gB_ld] matrices, or with gB_ld = 0 the C-layout images of
 * cbfssm_stash_contract_f64.  Writes d loss / d (flat parameter vector) to gflat.
 */
int cbfssm_train_tail_f64(const cbfssm_param_layout* pl, const cbfssm_pack_layout* layout_f, const double* pack_f,
                          const cbfssm_pack_layout* layout_b, const double* pack_b, const double* red,
                          const double* gB_dense_f, const double* gB_dense_b, int64_t gB_ld, const double* pflat,
                          const double* cflat, double* work, double* gflat, void* stream);
/* The same with the matrix section in another form (what the float32 adjoint leaves, cbfssm_*_pass_bwd_f32):
 * g_mode 0: d loss / d K^-1 (= cbfssm_train_tail_f64); 1: G = K^-1 (d loss / d K^-1) K^-1, the data part of d loss / d K_mm
 * itself, as a full matrix; 2: the lower-triangular 16 x 16 blocks of G + G^T (diagonal blocks: of G), blocks above the
 * diagonal ignored.  Only the symmetric part of G enters (dK_mm/dtheta is symmetric, gp_tf.py:33-49). */
int cbfssm_train_tail_g_f64(const cbfssm_param_layout* pl, const cbfssm_pack_layout* layout_f, const double* pack_f,
                            const cbfssm_pack_layout* layout_b, const double* pack_b, const double* red,
                            const double* gB_dense_f, const double* gB_dense_b, int64_t gB_ld, int g_mode, const double* pflat,
                            const double* cflat, double* work, double* gflat, void* stream);

/*
 * The same tail for the forward-only variants -- CBFSSMHALF (cbfssmhalf.py:20-47,174-199) and the PR-SSM baseline
 * (prssm.py:28-47,81-82,96): ONE GP (gp_f), var_y with dim_y entries.  Flat vectors (pflat unconstrained, cflat constrained,
 * gflat the gradient) in the order zeta_pos [M][D] | zeta_mean [M][Do] | zeta_var [M][Do] | variance [1] | lengthscales [D, or
 * 1 with shared_ls: PR-SSM's one lengthscale for all input dimensions, prssm.py:40] | var_x [Do] | var_y [dim_y].
 * red = [slab | loglik, kl_x, entropy (0), dloss/dvar_y[dim_y]] (cbfssm_reduce_partials_f64 + cbfssm_data_tail_f64).
 * pack_kl: NULL, or (PR-SSM) the pack of the same parameters prepared with jitter 0 -- the prior-KL terms then use the
 * jitter-free K_mm^-1 as the reference factorises the prior without jitter.  g_mode: the form of the matrix section, as in
 * cbfssm_train_tail_g_f64 (0 after the float64 adjoint, 1 / 2 after cbfssm_half_forward_pass_bwd_f32).
 * work: cbfssm_train_tail_half_work_elems doubles.
 */
int64_t cbfssm_train_tail_half_work_elems(const cbfssm_pack_layout* layout);
int cbfssm_train_tail_half_f64(const cbfssm_pack_layout* layout, const double* pack, const double* pack_kl, int shared_ls,
                               const double* red, const double* gB_dense, int64_t gB_ld, int g_mode, int dim_y,
                               const double* pflat, const double* cflat, double* work, double* gflat, void* stream);

/*
 * Recognition model of the forward-only variants: x_0 = dense(GRUCell(16)(the first recog_len steps of [u, y], reversed))
 * (cbfssm/model/cbfssmhalf.py:82-93, cbfssm/model/prssm.py:132-141; TF-1.8 GRUCell gate layout).  params: the six tensors
 * behind each other -- gate kernel [dim_u + dim_y + 16][32], gate bias [32], candidate kernel [dim_u + dim_y + 16][16],
 * candidate bias [16], dense kernel [16][dim_x], dense bias [dim_x] = cbfssm_gru_recog_param_elems doubles.  One wave per
 * sequence; act (cbfssm_gru_recog_act_elems doubles, or NULL when no gradient follows) keeps every step's h, r, u, c.
 * The backward call takes d loss / d x_0 per sequence (the adjoint pass's gx0 summed over the particles) and writes one
 * gradient slab of cbfssm_gru_recog_param_elems doubles per sequence (gpart: room for B + CBFSSM_REDUCE_SPLIT slabs);
 * cbfssm_reduce_partials_f64(gpart, elems, B, out) sums them in a fixed order.
 * The two counts are host arithmetic: -1 for dim_u < 0, dim_y < 1, dim_x < 1, B < 1 or recog_len < 1, and no upper limit.
 * Limits of the compute entry points, decided on the host before anything is launched: 1 <= recog_len <= T, dim_y >= 1
 * (else -1); dim_u + dim_y <= 32, dim_x <= 16 (else -3).  u may be NULL when dim_u = 0.
 */
int64_t cbfssm_gru_recog_param_elems(int dim_u, int dim_y, int dim_x);
int64_t cbfssm_gru_recog_act_elems(int B, int recog_len);
int cbfssm_gru_recog_f64(int B, int T, int dim_u, int dim_y, int dim_x, int recog_len, const double* u, const double* y,
                         const double* params, double* x0, double* act, void* stream);
int cbfssm_gru_recog_bwd_f64(int B, int T, int dim_u, int dim_y, int dim_x, int recog_len, const double* u, const double* y,
                             const double* params, const double* act, const double* gx0, double* gpart, void* stream);

/*
 * PR-SSM's conv recognition model (cbfssm/model/prssm.py:146-157): x_0 = dense(flatten(max_pooling1d(2, 2)(conv1d(5
 * filters, width 3, relu)(float32(the first recog_len steps of [u, y]))))), cast back to float64.  `_f32`: the arithmetic is
 * float32 as the reference casts it; every buffer is float64 like the other buffers of this interface, each value
 * rounded to float32 as it is read.  With n_in = dim_u + dim_y, P = (recog_len - 2) / 2 (an odd last conv position is
 * dropped by the pooling), params: the four tensors behind each other -- conv kernel [3][n_in][5] (TensorFlow's layout),
 * conv bias [5], dense kernel [5 P][dim_x] (rows in (time, channel) order), dense bias [dim_x] =
 * cbfssm_conv_recog_param_elems doubles (host arithmetic; -1 for bad dimensions, -3 beyond the limits below).
 * One wave per sequence; nothing is kept for the gradient: the backward call recomputes the forward in the same
 * operation order (the same pooling winners and relu mask), takes d loss / d x_0 per sequence (the adjoint pass's gx0
 * summed over the particles) and writes one gradient slab of cbfssm_conv_recog_param_elems doubles per sequence (gpart:
 * room for B + CBFSSM_REDUCE_SPLIT slabs); cbfssm_reduce_partials_f64(gpart, elems, B, out) sums them in a fixed order.
 * Sub-gradients: relu'(0) = 0, a pooling tie goes to the first element.
 * Limits: 4 <= recog_len <= T, dim_y >= 1 (else -1); dim_u + dim_y <= 32, dim_x <= 16, recog_len <= 64 (else -3).
 */
int64_t cbfssm_conv_recog_param_elems(int dim_u, int dim_y, int dim_x, int recog_len);
int cbfssm_conv_recog_f32(int B, int T, int dim_u, int dim_y, int dim_x, int recog_len, const double* u, const double* y,
                          const double* params, double* x0, void* stream);
int cbfssm_conv_recog_bwd_f32(int B, int T, int dim_u, int dim_y, int dim_x, int recog_len, const double* u, const double* y,
                              const double* params, const double* gx0, double* gpart, void* stream);

/*
 * ---- input gradients of the forward-only variants (CBFSSMHALF, PR-SSM): d loss / d u (B,T,dim_u), d loss / d y (B,T,dim_y).
 * Replaces tf.gradients(model.loss, model.sample_in) and tf.gradients(model.loss, model.sample_out) on the graphs of
 * cbfssm/model/cbfssmhalf.py:82-93,117-199 and cbfssm/model/prssm.py:96-157 (placeholders: base_model.py:22-27).  float64 only.
 * There u and y reach the loss three ways: through gp_f's input and the Kalman update in the time loop, through the
 * log-likelihood, and through x_0, the recognition model's output over the window [u, y][:, :recog_len].
 *
 * cbfssm_gru_recog_bwd_in_f64 / cbfssm_conv_recog_bwd_in_f32: the recognition backward calls above (same arguments, the
 * same kernel source with the window adjoint compiled in, the same bits in gpart) which also write gwin (B, recog_len, dim_u + dim_y): the adjoint of the window, row t
 * in SEQUENCE time order (cbfssmhalf.py:86 reverses the window for the GRU; not here), u columns first.  Every entry is
 * written exactly once, no atomics.  GRU (float64): per step, gx[i] = sum_j W_g[i][j] dgp[j] + sum_j W_c[i][j] dcp[j] over the
 * gate and candidate pre-activation adjoints.  conv (float32 arithmetic, prssm.py:146-157; the adjoint of the casts is the
 * identity): gx[t][i] = sum_w sum_f K[w][i][f] dpre[t - w][f] over the valid taps, dpre the pre-activation adjoint (the pooled
 * adjoint at the pooling winner where its pre-activation is positive, else 0: relu'(0) = 0, a tie goes to the first element).
 * Limits and return codes as for the calls above; gwin must not be NULL.
 *
 * cbfssm_half_forward_pass_bwd_in_f64: cbfssm_half_forward_pass_bwd_f64 (cbfssmhalf.py:117-172, prssm.py:96-118) through
 * the input-gradient instantiations of the adjoint kernel, as cbfssm_forward_pass_bwd_in_f64 is to the `_ex` form: also
 * writes gin_f (cbfssm_input_adjoint_fwd_elems doubles, (T-1, dim_u, N)) and the rows t >= 1 of gyo
 * (cbfssm_input_adjoint_obs_elems doubles, (T, dim_y, N); zeros where a step does not condition, i.e. everywhere for
 * PR-SSM).  Row 0 of gyo is not written: x_0 is the recognition output here, its adjoint leaves as gx0.
 *
 * cbfssm_half_input_grads_f64: one launch after the adjoint and the recognition backward call, one thread per entry, the S
 * particles summed in particle order, terms added in this order:
 *   grad_u[b,t,k] = [t <= T-2] 1/l_f[dim_x+k] sum_s gin_f[t][k][bS+s]  +  [t < recog_len, gwin] gwin[b][t][k]
 *   grad_y[b,t,d] = [t >= 1] sum_s gyo[t][d][bS+s]  +  cL sum_s (y[b,t,d] - x[t,bS+s,d]) / var_y[d]      (all T rows:
 *                   cbfssmhalf.py:174-189, prssm.py:96)  +  [t < recog_len, gwin] gwin[b][t][dim_u+d]
 *                   +  [t = 0, gx0] sum_s gx0[bS+s][d]
 * Exactly one of gx0 (the `output` recogniser: x_0 = [y_0, 0]; the adjoint pass's (N, dim_x) buffer) and gwin (rnn / conv;
 * recog_len = its row count, 1 <= recog_len <= T) is not NULL.  cL: lambda_0 / S for CBFSSMHALF, lambda_0 for PR-SSM.
 * grad_u may be NULL when dim_u = 0.  Fixed order, no atomics: two evaluations are bitwise identical.
 */
int cbfssm_gru_recog_bwd_in_f64(int B, int T, int dim_u, int dim_y, int dim_x, int recog_len, const double* u, const double* y,
                                const double* params, const double* act, const double* gx0, double* gpart, double* gwin,
                                void* stream);
int cbfssm_conv_recog_bwd_in_f32(int B, int T, int dim_u, int dim_y, int dim_x, int recog_len, const double* u, const double* y,
                                 const double* params, const double* gx0, double* gpart, double* gwin, void* stream);
int cbfssm_half_forward_pass_bwd_in_f64(const cbfssm_problem* p, const cbfssm_pack_layout* layout_f, const double* pack_f,
                                        const double* var_x, const double* var_y, const double* u, const double* y,
                                        const double* eps_f, const double* x, const double* fmv_f, const double* a2s_f,
                                        double cL, double* gx0, double* gpart, int t_hi, int t_lo, double* gx_carry,
                                        double* stash_a, double* stash_k, int64_t stash_ld, double* gin_f, double* gyo,
                                        void* stream);
int cbfssm_half_input_grads_f64(const cbfssm_problem* p, const cbfssm_pack_layout* layout_f, const double* pack_f,
                                const double* var_y, const double* y, const double* x, const double* gin_f, const double* gyo,
                                const double* gx0, const double* gwin, int recog_len, double cL, double* grad_u, double* grad_y,
                                void* stream);

/* The rank-local data terms of the flat reduce buffer: tail[0..2] = loglik, kl_x, entropy (from the ELBO combination's
 * out[0..2]); tail[3 + d] = d loss / d var_y[d] through the log-likelihood (cbfssm.py:245-251), d < dim_y, from the
 * per-dimension totals of ll_part (cbfssm_loglik_moments_f64).  cL = loss_factors[0] / S. */
int cbfssm_data_tail_f64(const cbfssm_problem* p, const double* var_y, const double* ll_part, const double* out8, double cL,
                         double* tail, void* stream);

/* tf.train.AdamOptimizer(learning_rate).minimize (cbfssm.py:273-275; TF 1.8 rule): t_dev (one double on the device)
 * is incremented, then lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t), p -= lr_t m / (sqrt(v) + eps). */
int cbfssm_adam_step_f64(int64_t n, double* pflat, const double* gflat, double* m, double* v, double* t_dev, double lr,
                         double beta1, double beta2, double eps, void* stream);

/* ---- noise.  The reference draws its standard normals inside the graph (tf.random_normal: cbfssm.py:134,149,209;
 * cbfssmhalf.py:142; prssm.py:126), one per (b, s) chain and step; the passes above take them as arrays (hid_b, eps_b, eps_f).
 * cbfssm_normal_f64 fills such an array on the device: Philox4x32-10 (counter = element pair index, key = seed) + Box-Muller in
 * float64.  out[i] is a pure function of (seed, offset + i) -- a caller that advances `offset` by the elements it has drawn
 * gets one reproducible stream per seed, however the draws are split over calls, streams or devices.
 * cbfssm_philox4x32_10_u32: the generator's four 32-bit words for the counters first_counter .. first_counter + ncounters - 1
 * (out: 4 * ncounters words) -- the known-answer vectors of the Philox paper are checked through it. */
int cbfssm_normal_f64(uint64_t seed, uint64_t offset, int64_t n, double* out, void* stream);
int cbfssm_philox4x32_10_u32(uint64_t seed, uint64_t first_counter, int64_t ncounters, uint32_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
