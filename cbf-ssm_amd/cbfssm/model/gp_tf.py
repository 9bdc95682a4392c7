"""cbfssm.model.gp_tf on the MI355X HIP path: the GP primitives of the reference's cbfssm/model/gp_tf.py with the same
names and argument meaning -- `RBF`, `cast_cholesky`, `conditional`, `GPModel.predict / prior_kl` -- evaluated by the
library behind include/cbfssm_hip.h.  Inputs are numpy arrays or torch tensors; results are float64 torch tensors on the
device.  (The model classes do not go through this module: they drive the fused pass kernels directly.  This is the
stand-alone surface of the same kernels, for callers that hold GP objects rather than a whole model.)

    kern = RBF(variance, lengthscales)                 gp_tf.py:20-49
    kern.K(X), kern.K(X, X2), kern.Kdiag(X)
    cast_cholesky(mat, jitter=1e-8)                    gp_tf.py:52-65  (float64 whatever the input dtype)
    conditional(Xnew, X, kern, f, q_sqrt, Lm=None)     gp_tf.py:68-100 (q_sqrt None, (M, Do) or (Do, M, M))
    GPModel(in_dim, out_dim, num_points, gp_var, gp_len, zeta_mean, zeta_pos, zeta_var, q_full=False)     gp_tf.py:103-172

Every function here that the reference can differentiate is differentiable.  `conditional` returns tensors with a grad_fn
when grad is enabled and one of Xnew, X, f, q_sqrt, kern.variance_unc, kern.lengthscales_unc requires it, in all three
q_sqrt branches: None and (M, Do) through the batch adjoint of GPModel.predict, (Do, M, M) through the full-covariance
adjoint (cbfssm.hip.autograd.gp_predict_fullq: the S_d A2 product on the f64 MFMA units, d loss / d q_sqrt exactly zero
above the diagonal).  `GPModel(..., q_full=True)` holds a full-covariance q(z) -- lower-triangular factors `zeta_sqrt`
(Do, M, M), the zeta_std.ndims == 3 branch of gp_tf.py:150-159 -- and trains with torch.optim through the same kernels;
`rollout` / `filter` are for the diagonal q(z) only.

GPModel is differentiable: when one of its five leaf tensors (`GPModel.parameters()`) or `Xnew` requires grad, `predict`
and `prior_kl` return tensors with a grad_fn (cbfssm.hip.autograd.gp_predict / gp_prior_kl: hand-written adjoint kernels,
no tensor-library fallback), so a model built around a sparse GP -- the reference's Voliro pattern, gp_f.predict plus a
physics term (cbfssm/model/voliro.py:106-123) -- trains with torch.optim.  Without a gradient request both are the
evaluation-only calls they always were.  `GPModel.rollout` (not in the reference) runs the GP's recurrence over time with
per-chain inputs as one fused launch, differentiable in the same way.

`GPModel.linearize(Xnew)` hands out the local linear model of the learned function: fmean, fvar and their Jacobians with
respect to Xnew for all output dimensions in one launch -- what the reference gets from tf.gradients(fmean[:, d], Xnew) per
output dimension through gp_tf.py:132-161 -- and `GPModel.transition_jacobians(h, a)` the matrices A = d m / d h,
B = d m / d a of the recurrence m = h + fmean(concat(h, a)) that `rollout` and `filter` run (EKF-style filtering, iLQR / MPC
around a learned transition).  Both are evaluation only and for the diagonal q(z).

`GPModel.ekf(m0, P0, a, y, var_x, var_y, cond=None)` runs the recursion those Jacobians are for: the extended Kalman filter
over the GP as a transition -- per chain a mean and a full state covariance propagated through m = h + fmean, conditioned
on observations of the first Dy state dimensions where `cond` says so (cbfssm/model/cbfssm.py:199-221,245-251) -- with the
log-likelihood of each chain, as one fused launch.  cond = 0 everywhere is a deterministic multi-step forecast with its
covariances.  Diagonal q(z).  Evaluation only by default; `ekf(..., differentiable=True)` gives means, covs and loglik a
grad_fn into m0, P0, a, y, var_x, var_y and the five parameter tensors (one fused adjoint launch over the whole time loop,
cbfssm.hip.autograd.gp_ekf): -loglik.sum() is the marginal likelihood of the GP state-space model as a training objective,
with no particles and no sampling noise.
`GPModel.eks(..., lag_one=False)` is that filter followed by the Rauch-Tung-Striebel sweep: smoothed and one-step predictive
moments, the smoothed initial belief and, on request, the lag-one cross-covariances (the E-step of EM), in four launches.

`GPModel.moment_match(mean, cov)` is the exact counterpart of `linearize` for a Gaussian input x ~ N(mean, cov): E[f], the
full output covariance Cov(f, f) and Cov(f, x) in closed form for the RBF kernel (the moment matching of PILCO and of the GP
assumed-density filter), right where the belief is as wide as a lengthscale and a first-order model is not -- one launch,
the (N, M, M) matrix of expected kernel products never reaches memory.  `GPModel.transition_moments(h, P, a)` is the
Gaussian one-step prediction of the recurrence on top of it: m+, P+ and Cov(h, h+).  Both are for the diagonal q(z) and
evaluation only by default; with `input_grads=True` their results carry a grad_fn into the belief -- `mean` and `cov`, or
`h`, `P` and `a` -- through one fused adjoint launch (cbfssm.hip.autograd.gp_moment_match), so that an input sequence, a
policy or an initial belief can be optimised through a propagated belief over the learned model.  The model is a constant of
such a call: its five leaves receive no gradient from these results (the reference has no moment matching to differentiate).

`GPModel.adf(m0, P0, a, y, var_x, var_y, cond)` is the recursion that primitive was written for: the assumed-density
(moment-matching) Kalman filter, `ekf` with the exact moments in place of the linearisation at the mean, as one launch for
all steps -- the moment-match work of a step inside the time loop, alpha and the W_d tiles formed once per call.
`GPModel.ads(...)` is the Rauch-Tung-Striebel smoother behind it (`eks`'s sweep on Cov(h_t, h_{t-1}) = P + Cx).  Both are
for the diagonal q(z); `ads` is evaluation only, and so is `adf` by default.  `adf(..., input_grads=True)` gives means, covs
and loglik a grad_fn into m0, P0, a, y, var_x and var_y -- one fused reverse-time adjoint launch over the whole propagated
belief (cbfssm.hip.autograd.gp_adf), the model a constant of the call as for `moment_match`: an open-loop input sequence
under an expected cost (cond = 0), an initial belief, or the noise levels by the ADF marginal likelihood -loglik.sum() become
one-call objectives on the device.
"""
import ctypes as C
import numpy as np
import torch

from ..hip import lib as _l
from ..hip import ops
from ..hip.ops import _f64, _ptr, _stream
from ..synthetic import softplus_inverse
from .session import InvalidArgumentError


def _device(device=None):
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise RuntimeError('cbfssm needs an MI355X: no HIP device is visible and there is no CPU fallback')
    return torch.device('cuda', torch.cuda.current_device())


def forward(x):
    """softplus(x) + 1e-10 (tf_transform.py:19-21)"""
    return ops.tf_forward(x)


def backward(y):
    """inverse of forward on the host (tf_transform.py:13-16)"""
    return softplus_inverse(y)


class RBF:
    """ARD squared-exponential kernel, parameters kept unconstrained like the reference's tf.Variables."""

    def __init__(self, variance, lengthscales, dtype='float64', device=None):
        self.device = _device(device)
        self.variance_unc = torch.tensor(np.atleast_1d(backward(variance)), dtype=torch.float64, device=self.device)
        self.lengthscales_unc = torch.tensor(np.atleast_1d(backward(lengthscales)), dtype=torch.float64, device=self.device)

    @property
    def variance(self):
        return forward(self.variance_unc)

    @property
    def lengthscales(self):
        return forward(self.lengthscales_unc)

    def Kdiag(self, X):
        X = _f64(X, self.device)
        return self.variance.reshape(()).expand(X.shape[0]).clone()

    def K(self, X, X2=None):
        X = _f64(X, self.device)
        X2 = X if X2 is None else _f64(X2, self.device)
        assert X.dim() == 2 and X2.dim() == 2 and X.shape[1] == X2.shape[1] == self.lengthscales.numel()
        out = torch.empty(X.shape[0], X2.shape[0], dtype=torch.float64, device=self.device)
        ls, var = self.lengthscales.contiguous(), self.variance.contiguous()     # (named: they must outlive the launch)
        rc = _l.load().cbfssm_rbf_k_f64(X.shape[0], X2.shape[0], X.shape[1], _ptr(X), _ptr(X2), _ptr(ls), _ptr(var),
                                        _ptr(out), _stream())
        _l.check(rc, 'cbfssm_rbf_k_f64')
        return out


def cast_cholesky(mat, jitter=1e-8):
    """Lower Cholesky factor of mat + jitter I, computed in float64 whatever dtype comes in (gp_tf.py:57-65); a matrix
    that is not positive definite raises InvalidArgumentError as tf.cholesky does."""
    dev = mat.device if torch.is_tensor(mat) and mat.is_cuda else _device()
    in_dtype = mat.dtype if torch.is_tensor(mat) else None
    m = _f64(mat, dev)
    assert m.dim() == 2 and m.shape[0] == m.shape[1]
    M = m.shape[0]
    L = torch.empty_like(m)
    info = torch.zeros(1, dtype=torch.float64, device=dev)
    work = torch.empty(M * (M + 1) + 64, dtype=torch.float64, device=dev)
    rc = _l.load().cbfssm_cholesky_f64(M, _ptr(m), float(jitter), _ptr(L), _ptr(info), _ptr(work), _stream())
    _l.check(rc, 'cbfssm_cholesky_f64')
    if float(info[0]) != 0.0:
        raise InvalidArgumentError('Cholesky decomposition was not successful: leading minor %d is not positive definite'
                                   % int(info[0]))
    return L.to(in_dtype) if in_dtype is not None and in_dtype != torch.float64 else L


def _pack_for(kern, X, f, zeta_var):
    M, D = X.shape
    Do = f.shape[1]
    pack = ops.GPPack(M, D, Do, kern.device)
    pack.prepare(X, kern.lengthscales, kern.variance, f, zeta_var)
    if float(pack.scal[_l.SCAL_INFO]) != 0.0:
        raise InvalidArgumentError('Cholesky decomposition was not successful: leading minor %d of K(X) + 1e-8 I is not '
                                   'positive definite' % int(pack.scal[_l.SCAL_INFO]))
    return pack


def conditional(Xnew, X, kern, f, q_sqrt, Lm=None):
    """GPflow-1.0-style conditional (gp_tf.py:68-100): p(f* | q(f) = N(f, q_sqrt q_sqrt^T)), unwhitened.
    q_sqrt: None, (M, Do) standard deviations, or (Do, M, M) lower-triangular factors.  `Lm` is accepted for signature
    compatibility; the factor is recomputed from (X, kern) on the device (it is what Lm must equal, gp_tf.py:71-72).
    Returns (fmean (N, Do), fvar (N, Do)).  When grad is enabled and Xnew, X, f, q_sqrt, kern.variance_unc or
    kern.lengthscales_unc requires grad, the results carry a grad_fn (hand-written adjoint kernels in all three branches;
    the gradient of a (Do, M, M) q_sqrt is exactly zero above the diagonal, whose entries that path never reads).  Without a
    gradient request the call is evaluation only, the code and the bits it always was: it hands q_sqrt to its kernel as it
    is, and like the reference's matmul (gp_tf.py:94) that kernel reads the whole matrix, so pass lower-triangular factors."""
    dev = kern.device
    if torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad
                                       for t in (Xnew, X, f, q_sqrt, kern.variance_unc, kern.lengthscales_unc)):
        return _conditional_grad(Xnew, X, kern, f, q_sqrt)
    X, Xnew, f = _f64(X, dev), _f64(Xnew, dev), _f64(f, dev)
    M, Do = f.shape
    if q_sqrt is None:
        pack = _pack_for(kern, X, f, torch.zeros(M, Do, dtype=torch.float64, device=dev))
        return pack.predict(Xnew)
    q = _f64(q_sqrt, dev).contiguous()
    if q.dim() == 2:
        assert q.shape == (M, Do)
        return _pack_for(kern, X, f, q * q).predict(Xnew)
    if q.dim() != 3:
        raise ValueError("bad dimension for q_sqrt")
    assert q.shape == (Do, M, M)
    pack = _pack_for(kern, X, f, torch.zeros(M, Do, dtype=torch.float64, device=dev))
    lib = _l.load()
    n = Xnew.shape[0]
    fmean = torch.empty(n, Do, dtype=torch.float64, device=dev)
    fvar = torch.empty_like(fmean)
    work = torch.empty(int(lib.cbfssm_gp_predict_fullq_work_elems(C.byref(pack.layout), n)), dtype=torch.float64, device=dev)
    rc = lib.cbfssm_gp_predict_fullq_f64(C.byref(pack.layout), _ptr(pack.buf), _ptr(q), _ptr(Xnew), n,
                                         _ptr(fmean), _ptr(fvar), _ptr(work), _stream())
    _l.check(rc, 'cbfssm_gp_predict_fullq_f64')
    return fmean, fvar


def _conditional_grad(Xnew, X, kern, f, q_sqrt):
    """conditional() under a gradient request: the same three branches through cbfssm.hip.autograd"""
    from ..hip import autograd as _ag
    dev = kern.device
    as64 = lambda t: torch.as_tensor(t, dtype=torch.float64, device=dev)
    X, Xnew, f = as64(X), as64(Xnew), as64(f)
    M, Do = f.shape
    pack = ops.GPPack(M, X.shape[1], Do, dev)
    if q_sqrt is None or as64(q_sqrt).dim() == 2:
        if q_sqrt is None:
            s2 = torch.zeros(M, Do, dtype=torch.float64, device=dev)
        else:
            q = as64(q_sqrt)
            assert q.shape == (M, Do)
            s2 = q * q                                                       # (its chain rule, 2 q o s2bar, is torch's)
        out = _ag.gp_conditional_diag(pack, Xnew, X, f, s2, kern.variance_unc, kern.lengthscales_unc)
    else:
        q = as64(q_sqrt)
        if q.dim() != 3:
            raise ValueError("bad dimension for q_sqrt")
        assert q.shape == (Do, M, M)
        out = _ag.gp_predict_fullq(pack, Xnew, X, f, q, kern.variance_unc, kern.lengthscales_unc)
    if float(pack.scal[_l.SCAL_INFO]) != 0.0:
        raise InvalidArgumentError('Cholesky decomposition was not successful: leading minor %d of K(X) + 1e-8 I is not '
                                   'positive definite' % int(pack.scal[_l.SCAL_INFO]))
    return out


class GPModel:
    """Sparse GP with diagonal q(z) (gp_tf.py:103-172): inducing inputs / means drawn as the reference draws them
    (unseeded unless `seed` is given), `predict(Xnew)` and `prior_kl()` on the device.  The five tensors of `parameters()`
    are leaves: set `requires_grad_()` on them (or hand `predict` an `Xnew` that requires grad) and both calls are
    differentiable; see the module docstring.

    q_full=True: a full-covariance q(z_d) = N(zeta_mean[:, d], L_d L_d^T) per output dimension (the zeta_std.ndims == 3
    branch of gp_tf.py:150-159).  The third leaf is then `zeta_sqrt` (Do, M, M), unconstrained, initialised to
    sqrt(zeta_var) I; only its lower triangle is read and its gradient above the diagonal is exactly zero.  `zeta_std`
    returns the factors L_d, `zeta_var` the marginal variances diag(L_d L_d^T) as (M, Do).  `rollout`, `filter`,
    `linearize`, `transition_jacobians`, `ekf`, `eks`, `moment_match`, `transition_moments`, `adf` and `ads` raise ValueError
    on such a model."""

    def __init__(self, in_dim, out_dim, num_points, gp_var, gp_len, zeta_mean, zeta_pos, zeta_var, dtype='float64',
                 device=None, seed=None, q_full=False):
        self.in_dim, self.out_dim, self.num_points, self.dtype = in_dim, out_dim, num_points, dtype
        rng = np.random.default_rng(seed)
        dev = _device(device)
        self.zeta_pos = torch.tensor(rng.uniform(-zeta_pos, zeta_pos, size=(num_points, in_dim)), device=dev)   # :112-115
        self.zeta_mean = torch.tensor(zeta_mean * rng.random((num_points, out_dim)), device=dev)                 # :117-118
        self.q_full = bool(q_full)
        if self.q_full:
            eye = np.sqrt(zeta_var) * np.eye(num_points)
            self.zeta_sqrt = torch.tensor(np.broadcast_to(eye, (out_dim, num_points, num_points)).copy(), device=dev)
        else:
            self.zeta_var_unc = torch.tensor(backward(zeta_var * np.ones((num_points, out_dim))), device=dev)   # :120-121
        self.kern = RBF(gp_var, np.asarray([gp_len] * in_dim, dtype=np.float64), device=dev)                     # :125-127
        self._pack = ops.GPPack(num_points, in_dim, out_dim, dev)

    @property
    def zeta_var(self):
        if self.q_full:
            L = self.zeta_std
            return (L * L).sum(dim=2).t().contiguous()                       # diag(L_d L_d^T): row sums of squares
        return forward(self.zeta_var_unc)

    @property
    def zeta_std(self):
        if self.q_full:
            return torch.tril(self.zeta_sqrt.detach())                       # what gp_tf.py:153 reads
        return torch.sqrt(self.zeta_var)

    def _prepared(self):
        if self.q_full:                                                      # (zeta_var = 0: cbfssm_gp_predict_fullq_f64's pack)
            self._pack.prepare(self.zeta_pos, self.kern.lengthscales, self.kern.variance, self.zeta_mean,
                               torch.zeros_like(self.zeta_mean))
            return self._pack
        self._pack.prepare(self.zeta_pos, self.kern.lengthscales, self.kern.variance, self.zeta_mean, self.zeta_var)
        return self._pack

    @property
    def cholesky(self):
        return self._prepared().L.clone()                                                                        # :129-130

    def parameters(self):
        """The five trainable leaves, in the order of cbfssm.hip.autograd.GP_PARAM_NAMES (q_full: GP_FULLQ_PARAM_NAMES)."""
        if self.q_full:
            return [self.zeta_pos, self.zeta_mean, self.zeta_sqrt, self.kern.variance_unc, self.kern.lengthscales_unc]
        return [self.zeta_pos, self.zeta_mean, self.zeta_var_unc, self.kern.variance_unc, self.kern.lengthscales_unc]

    def _wants_grad(self, *more):
        return torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in self.parameters() + list(more))

    def _no_full_q(self, what):
        if self.q_full:
            raise ValueError('GPModel.%s runs a diagonal q(z) only: this model was built with q_full=True (use predict / '
                             'prior_kl)' % what)

    def predict(self, Xnew):
        if self.q_full:
            return self._predict_full(Xnew)
        if self._wants_grad(Xnew):
            from ..hip import autograd as _ag
            return _ag.gp_predict(self._pack, Xnew, *self.parameters())
        return self._prepared().predict(Xnew)                                                                    # :132-161

    def _predict_full(self, Xnew):                                                                               # :150-159
        from ..hip import autograd as _ag
        if self._wants_grad(Xnew):
            return _ag.gp_predict_fullq(self._pack, Xnew, *self.parameters())
        Xnew = _f64(Xnew, self.zeta_pos.device).contiguous()
        pack = self._prepared() if Xnew.shape[0] else self._pack                 # (nothing runs without a point)
        return _ag.gp_fullq_eval(pack, Xnew, self.zeta_sqrt, self.zeta_mean)

    def prior_kl(self):
        if self.q_full:
            from ..hip import autograd as _ag
            if self._wants_grad():
                return _ag.gp_prior_kl_fullq(self._pack, *self.parameters())
            return _ag.gp_fullq_eval(self._prepared(), None, self.zeta_sqrt, self.zeta_mean)
        if self._wants_grad():
            from ..hip import autograd as _ag
            return _ag.gp_prior_kl(self._pack, *self.parameters())
        return self._prepared().scal[_l.SCAL_KLZ].clone()                                                        # :163-172

    def rollout(self, h0, a, eps, var_add=None, reverse=False):
        """An addition to the reference's surface (its GPModel has predict and prior_kl only): the recurrence

            for t in 0..T-1 (reverse: T-1..0):  fmean, fvar = predict(concat(h, a[t]));  v = fvar + var_add
                                                h = h + fmean + eps[t][:, None] * sqrt(v);  traj[t] = h
            entropy = 0.5 * sum(log(2 pi e v))

        as one launch -- the loop of Voliro's recognition run (cbfssm/model/voliro.py:139-186: reverse=True, h0 = 0,
        a = (u_t, y_t) per particle) and of a CBF-SSM's free-running transition (cbfssm/model/cbfssm.py:199-206,224).
        h0 (N, out_dim), a (T, N, in_dim - out_dim) or None when the GP takes the state alone, eps (T, N) standard normals,
        var_add (out_dim) constrained values or None.  Returns (traj (T, N, out_dim), entropy ()).  When a leaf, h0, a or
        var_add requires grad both results carry a grad_fn (cbfssm.hip.autograd.gp_rollout; eps gets no gradient);
        otherwise the forward kernel runs alone and keeps nothing for an adjoint."""
        self._no_full_q('rollout')
        from ..hip import autograd as _ag
        if self._wants_grad(h0, a, var_add):
            return _ag.gp_rollout(self._pack, h0, a, eps, var_add, *self.parameters(), reverse=reverse)
        return _ag.gp_rollout_eval(self._prepared(), h0, a, eps, var_add, reverse=reverse)

    def filter(self, h0, a, ytilde, eps, var_x, var_y, cond=None, k_factor=1.0, reverse=False):
        """An addition to the reference's surface: the conditioned forward step of CBF-SSM (cbfssm/model/cbfssm.py:185-237)
        over this GP from per-chain data, as one launch:

            for t in 0..T-1 (reverse: T-1..0):
                fmean, fvar = predict(concat(h, a[t]));  m = h + fmean;  v = fvar + var_x
                where cond[t, n]:  r = var_y + (k_factor - 1) v;  k = v / (r + v);  mu = m + k (ytilde[t] - m)
                                   sig = (1 - k)^2 v + k^2 r;  h = mu + eps[t][:, None] * sqrt(sig)
                                   kl += 0.5 (log v - log sig + (sig + (mu - m)^2) / v - 1)
                elsewhere:         h = m + eps[t][:, None] * sqrt(v)
                traj[t] = h

        h0 (N, out_dim), a (T, N, in_dim - out_dim) or None, ytilde (T, N, out_dim), eps (T, N) standard normals, var_x
        (out_dim) constrained values or None, var_y (out_dim) constrained values, cond (T, N) of 0 / 1 or None (condition
        everywhere): a prefix of ones is warm-up then forecast, zeros mark missing observations -- ytilde may hold NaN
        there, it is never read into a result.  Returns (traj (T, N, out_dim), kl ()).  When a leaf, h0, a, ytilde, var_x or
        var_y requires grad both results carry a grad_fn (cbfssm.hip.autograd.gp_filter; eps, cond and k_factor get no
        gradient); otherwise the forward kernel runs alone and keeps nothing for an adjoint."""
        self._no_full_q('filter')
        from ..hip import autograd as _ag
        if self._wants_grad(h0, a, ytilde, var_x, var_y):
            return _ag.gp_filter(self._pack, h0, a, ytilde, eps, var_x, var_y, *self.parameters(), cond=cond,
                                 k_factor=k_factor, reverse=reverse)
        pack = self._prepared() if torch.as_tensor(eps).numel() else self._pack      # (nothing runs without a chain or a step)
        return _ag.gp_filter_eval(pack, h0, a, ytilde, eps, var_x, var_y, cond=cond, k_factor=k_factor, reverse=reverse)

    def linearize(self, Xnew, variance=True):
        """An addition to the reference's surface, which takes tf.gradients(fmean[:, d], Xnew) per output dimension d
        through gp_tf.py:132-161: the local linear model of the GP at every row of Xnew (N, in_dim), as one launch,

            fmean, fvar (N, out_dim) = predict(Xnew)
            dmean[n, d, i] = d fmean[n, d] / d Xnew[n, i],   dvar[n, d, i] = d fvar[n, d] / d Xnew[n, i]    (N, out_dim, in_dim)

        Returns (fmean, fvar, dmean, dvar); variance=False leaves the variance Jacobian out (dvar is None, the K^-1 product
        per output dimension it needs is not done; the other three results are bitwise the same).  Evaluation only: the
        results carry no grad_fn whatever the leaves or Xnew ask for -- differentiating a Jacobian is not offered.  Raises
        ValueError on a q_full=True model."""
        self._no_full_q('linearize')
        from ..hip import autograd as _ag
        Xnew = _f64(Xnew, self.zeta_pos.device)
        pack = self._prepared() if Xnew.shape[0] else self._pack                 # (nothing runs without a point)
        return _ag.gp_linearize_eval(pack, Xnew, variance=variance)

    def ekf(self, m0, P0, a, y, var_x, var_y, cond=None, differentiable=False):
        """An addition to the reference's surface: the extended Kalman filter over this GP as the transition of CBF-SSM
        (cbfssm/model/cbfssm.py:199-221) with its observation model (cbfssm.py:245-251: the first Dy state dimensions plus
        N(0, diag(var_y))) -- a Gaussian belief per chain, mean and full covariance, as one launch:

            for t in 0..T-1:
                x = concat(m, a[t]);  f, fv = predict(x);  A = I + d fmean / d x [:, :out_dim]     (linearize's dmean)
                m = m + f;  P = A P A^T + diag(fv + var_x)
                where cond[t, n], for j in 0..Dy-1:  s = P[j, j] + var_y[j];  delta = y[t, n, j] - m[j];  g = P[:, j] / s
                                                     m += g delta;  P -= s g g^T
                                                     loglik[n] -= (log(2 pi s) + delta^2 / s) / 2
                means[t] = m;  covs[t] = P

        which is the joint Kalman update with H = [I_Dy 0], R = diag(var_y), and loglik[n] the log-likelihood of the
        conditioned observations of chain n, free of Monte-Carlo noise.  m0 (N, out_dim), P0 (N, out_dim, out_dim) or None
        (zero; only the lower triangle is read), a (T, N, in_dim - out_dim) or None, y (T, N, Dy) with 1 <= Dy <= out_dim,
        var_x (out_dim) constrained values or None, var_y (Dy) constrained values, cond (T, N) of 0 / 1 or None (condition
        everywhere): zeros mark missing observations -- y may hold NaN there, it is never read into a result -- and
        cond = 0 everywhere is uncertainty propagation, a multi-step forecast with its covariances, loglik exactly 0.
        Returns (means (T, N, out_dim), covs (T, N, out_dim, out_dim), loglik (N)); every covs[t, n] is bitwise symmetric.
        By default evaluation only: the results carry no grad_fn whatever the leaves or the inputs ask for.

        differentiable=True: when a leaf, m0, P0, a, y, var_x or var_y requires grad, the same values (bitwise) carry a
        grad_fn (cbfssm.hip.autograd.gp_ekf: one fused adjoint launch over the whole time loop), so -loglik.sum() is a
        training objective free of sampling noise.  All three results take cotangents (the one for covs need not be
        symmetric); once differentiable; cond gets no gradient.  Conventions: the gradient for P0 is that of the function
        of tril(P0) + tril(P0, -1)^T -- exactly zero above the diagonal, a strictly lower entry carries both symmetric
        contributions; an argument given as None (P0, var_x, a) has no gradient; the gradient for y is exactly 0 where
        cond = 0 (y may be NaN there), and with cond = 0 everywhere those for y and var_y are zero tensors.  `eks` stays
        evaluation only.  Raises ValueError on a q_full=True model and when in_dim < out_dim."""
        self._no_full_q('ekf')
        from ..hip import autograd as _ag
        if differentiable and self._wants_grad(m0, P0, a, y, var_x, var_y):
            return _ag.gp_ekf(self._pack, m0, P0, a, y, var_x, var_y, *self.parameters(), cond=cond)
        y = _f64(y, self.zeta_pos.device)
        pack = self._prepared() if y.shape[0] * y.shape[1] else self._pack       # (nothing runs without a chain or a step)
        return _ag.gp_ekf_eval(pack, m0, P0, a, y, var_x, var_y, cond=cond)

    def eks(self, m0, P0, a, y, var_x, var_y, cond=None, lag_one=False):
        """The Rauch-Tung-Striebel smoother behind `ekf`: the belief about every state given ALL observations of its chain.
        The forward pass is `ekf` itself (arguments, checks and the results means, covs, loglik are its own, bitwise); it
        also hands out the one-step predictive moments, and a backward sweep follows:

            pmeans[t] = m-_t;  pcovs[t] = P-_t = A_t P_{t-1} A_t^T + diag(fv + var_x)        (before conditioning)
            (smeans, scovs)[T-1] = (means, covs)[T-1]
            for t in T-1..0:   G = (A_t P_{t-1})^T (P-_t)^-1
                               smeans[t-1] = means[t-1] + G (smeans[t] - pmeans[t])
                               scovs[t-1]  = covs[t-1] + G (scovs[t] - pcovs[t]) G^T
                               lag_one[t]  = G scovs[t] = Cov(x_{t-1}, x_t | y)

        where time -1 is the initial belief (m0, P0): the last iteration gives (init_mean, init_cov).  Returns the
        namedtuple EksResult(smeans (T, N, out_dim), scovs (T, N, out_dim, out_dim), loglik (N), means, covs, pmeans,
        pcovs, init_mean (N, out_dim), init_cov (N, out_dim, out_dim), lag_one (T, N, out_dim, out_dim) or None unless
        lag_one=True, info (N) int64) -- what offline state estimation and the E-step of EM over the transition and noise
        parameters need.  scovs and init_cov are bitwise symmetric.  info[n] is 0, or t + 1 where P-_t of chain n was not
        positive definite (possible only when P0 is not positive semi-definite): that chain's smoothed results before t,
        its initial belief and lag_one[<= t] are then NaN and nothing else is affected.  Four launches, no host
        synchronisation.  Evaluation only: the results carry no grad_fn whatever the leaves or the inputs ask for.  Raises
        ValueError on a q_full=True model and when in_dim < out_dim."""
        self._no_full_q('eks')
        from ..hip import autograd as _ag
        y = _f64(y, self.zeta_pos.device)
        pack = self._prepared() if y.shape[0] * y.shape[1] else self._pack       # (nothing runs without a chain or a step)
        return _ag.gp_eks_eval(pack, m0, P0, a, y, var_x, var_y, cond=cond, lag_one=lag_one)

    def transition_jacobians(self, h, a=None):
        """The local linear model of the recurrence `rollout` and `filter` run, m = h + fmean(concat(h, a)):

            A[n] = d m[n] / d h[n] = I + dmean[n, :, :out_dim]   (N, out_dim, out_dim)
            B[n] = d m[n] / d a[n] = dmean[n, :, out_dim:]        (N, out_dim, in_dim - out_dim)

        h (N, out_dim), a (N, in_dim - out_dim) or None when the GP takes the state alone.  Returns (A, B); evaluation only,
        through linearize(..., variance=False)."""
        self._no_full_q('transition_jacobians')
        Do, Da = self.out_dim, self.in_dim - self.out_dim
        if Da < 0:
            raise ValueError('transition_jacobians: the GP input dimension %d is smaller than its output dimension %d'
                             % (self.in_dim, self.out_dim))
        dev = self.zeta_pos.device
        h = _f64(h, dev)
        assert h.dim() == 2 and h.shape[1] == Do, 'h (N, out_dim)'
        if Da == 0:
            assert a is None or tuple(a.shape) == (h.shape[0], 0), 'a: None or (N, 0) when the GP takes the state alone'
            X = h
        else:
            a = _f64(a, dev)
            assert tuple(a.shape) == (h.shape[0], Da), 'a (N, in_dim - out_dim)'
            X = torch.cat([h, a], dim=1)
        dmean = self.linearize(X, variance=False)[2]
        A = dmean[:, :, :Do] + torch.eye(Do, dtype=torch.float64, device=dev)
        return A, dmean[:, :, Do:].contiguous()

    def moment_match(self, mean, cov, cross=True, input_grads=False, differentiable=False):
        """An addition to the reference's surface: the exact moments of the GP output under a Gaussian input
        x[n] ~ N(mean[n], cov[n]) -- the moment matching of PILCO and of the GP assumed-density filter, closed form for the
        RBF kernel, where `linearize` is first order at the mean -- as one launch:

            fmean[n, d]    = E[f_d]                                       (N, out_dim)
            fcov[n, d, e]  = Cov(f_d, f_e)                                (N, out_dim, out_dim), bitwise symmetric
            xcov[n, d, i]  = Cov(f_d, x_i)                                (N, out_dim, in_dim), dmean's layout

        with f_d | x ~ N(fmean_d(x), fvar_d(x)) of `predict`, independent over d given x: diag fcov = E[fvar] + Var[fmean],
        and the off-diagonal is the correlation that sharing the uncertain input brings.  mean (N, in_dim); cov
        (N, in_dim, in_dim), only the lower triangle is read, or None (zero).  cov need only be positive semi-definite --
        zero blocks, rank one and cov = 0 are ordinary inputs; cov = 0 gives `predict` back (diag fcov = fvar) and xcov
        exactly zero.  Returns (fmean, fcov, xcov, info); cross=False leaves xcov out (None; the other results are bitwise
        the same).  info (N) int64 is 0, or 1 / 2 where cov[n] is not positive semi-definite (a non-positive pivot in the
        first / second factorisation): the results of that point are NaN and nothing else is affected.  Evaluation only by
        default: the results carry no grad_fn whatever the leaves or the inputs ask for.

        input_grads=True (named after loss_and_grads(..., input_grads=True)): when grad is enabled and `mean` or `cov`
        requires it, fmean, fcov and xcov carry a grad_fn into them -- the same launch forward (bitwise the same values),
        one fused adjoint launch backward, once differentiable; info never does.  The gradient for cov is that of the
        function of tril(cov) + tril(cov, -1)^T: exactly zero above the diagonal, both symmetric contributions on a strictly
        lower entry; cov=None has no gradient and the gradient for mean is then the input gradient of `predict`.  The model
        is a constant of the call -- the values its leaves had at the call: the five leaves get no gradient from these
        results whatever their requires_grad says (their .grad stays None, torch.autograd.grad(loss, leaf) fails as for any
        unconnected tensor).  Where info[n] != 0 the rows of point n of both gradients are NaN.

        differentiable=True (the keyword of `ekf`; it takes precedence over input_grads): when grad is enabled and a leaf,
        `mean` or `cov` requires it, the pack is prepared from the leaves and fmean, fcov and xcov (bitwise the values of
        the evaluation call) carry a grad_fn into the five leaves of `parameters()` AND into mean and cov
        (cbfssm.hip.autograd.gp_moment_match_params): the input adjoint launch, then the model adjoint -- a per-point pass
        and a tile-outer pass that deliver one slab -- and the tail that `predict` and `ekf` use.  So a loss of a
        moment-matched belief trains the inducing outputs, their variances, the inducing inputs, the lengthscales and the
        signal variance.  The conventions are those above (lower triangle of cov, unused results, cov=None: the leaf
        gradients are then those of `predict` for gmean = gfmean, gvar = diag gfcov); without a point nothing is prepared or
        launched and the leaf gradients are zeros; where info[n] != 0 all five leaf gradients are NaN as well.  If nothing
        requires grad, or grad is disabled, the call is the evaluation call.  Once differentiable, float64, no host
        synchronisation.
        Raises ValueError on a q_full=True model."""
        self._no_full_q('moment_match')
        from ..hip import autograd as _ag
        dev = self.zeta_pos.device
        mean = _f64(mean, dev)
        assert mean.dim() == 2 and mean.shape[1] == self.in_dim, 'mean (N, in_dim)'
        if cov is not None:
            cov = _f64(cov, dev)
            assert tuple(cov.shape) == (mean.shape[0], self.in_dim, self.in_dim), 'cov (N, in_dim, in_dim)'
        if differentiable and self._wants_grad(mean, cov):
            return _ag.gp_moment_match_params(self._pack, mean, cov, *self.parameters(), cross=cross)
        pack = self._prepared() if mean.shape[0] else self._pack                 # (nothing runs without a point)
        if input_grads:
            return _ag.gp_moment_match(pack, mean, cov, cross=cross)
        return _ag.gp_moment_match_eval(pack, mean, cov, cross=cross)

    def transition_moments(self, h, P, a=None, input_grads=False, differentiable=False):
        """The Gaussian one-step prediction of the recurrence `rollout`, `filter` and `ekf` run, h+ = h + f(concat(h, a)),
        for a belief h ~ N(h[n], P[n]) and a known input a (input covariance blockdiag(P, 0)), by `moment_match`:

            C  = Cov(h, f) = xcov[:, :, :out_dim]^T
            m+ = h + fmean;   P+ = P + C + C^T + fcov;   cross = P + C = Cov(h, h+)      (what a smoother gain needs)

        h (N, out_dim), P (N, out_dim, out_dim) of which only the lower triangle is read, a (N, in_dim - out_dim) or None
        when the GP takes the state alone.  Returns (m+, P+, cross, info); P+ is bitwise symmetric; the process noise var_x
        is the caller's to add; info as in `moment_match`.  Evaluation only by default; input_grads=True: m+, P+ and cross
        carry a grad_fn into h, P (the gradient of the function of its lower triangle) and a when one of them requires it --
        `moment_match(..., input_grads=True)` with the tensor-library steps around it on the tape; the model is a constant.
        differentiable=True: `moment_match(..., differentiable=True)` with the same steps on the tape -- m+, P+ and cross
        carry a grad_fn into the five leaves as well, so a Python loop over this call with tensor-library Kalman updates is
        a differentiable GP-ADF whose -loglik trains the model.
        Raises ValueError on a q_full=True model and when in_dim < out_dim."""
        self._no_full_q('transition_moments')
        Do, Da = self.out_dim, self.in_dim - self.out_dim
        if Da < 0:
            raise ValueError('transition_moments: the GP input dimension %d is smaller than its output dimension %d'
                             % (self.in_dim, self.out_dim))
        dev = self.zeta_pos.device
        h, P = _f64(h, dev), _f64(P, dev)
        assert h.dim() == 2 and h.shape[1] == Do, 'h (N, out_dim)'
        assert tuple(P.shape) == (h.shape[0], Do, Do), 'P (N, out_dim, out_dim)'
        Pl = torch.tril(P)
        P = Pl + torch.tril(P, -1).transpose(1, 2)                               # the function of the lower triangle
        if Da == 0:
            assert a is None or tuple(a.shape) == (h.shape[0], 0), 'a: None or (N, 0) when the GP takes the state alone'
            X, S = h, Pl
        else:
            a = _f64(a, dev)
            assert tuple(a.shape) == (h.shape[0], Da), 'a (N, in_dim - out_dim)'
            X = torch.cat([h, a], dim=1)
            S = torch.zeros(h.shape[0], self.in_dim, self.in_dim, dtype=torch.float64, device=dev)
            S[:, :Do, :Do] = Pl
        fmean, fcov, xcov, info = self.moment_match(X, S, input_grads=input_grads, differentiable=differentiable)
        Cm = xcov[:, :, :Do].transpose(1, 2)                                     # Cov(h, f)
        low = torch.tril(P + Cm + Cm.transpose(1, 2) + fcov)
        Pn = low + torch.tril(low, -1).transpose(1, 2)
        return h + fmean, Pn, P + Cm, info

    def adf(self, m0, P0, a, y, var_x, var_y, cond=None, input_grads=False):
        """The assumed-density (moment-matching) Kalman filter over this GP -- GP-ADF, PILCO's propagation: `ekf`'s
        recursion with the linearisation at the mean replaced by the exact moments of `moment_match` under the belief,
        which is what a belief as wide as a lengthscale needs.  One launch for all steps, per chain n:

            for t in 0..T-1:
                x = concat(m, a[t]);  S = blockdiag(P, 0)                     (the auxiliary input is known)
                fmean, fcov, xcov = moment_match(x, S);  Cx = xcov[:, :out_dim]          (Cx[d, i] = Cov(f_d, h_i))
                m- = m + fmean
                cross[t] = P + Cx                          (= Cov(h_t, h_{t-1}), row = new state: the layout `eks` uses)
                P- = P + Cx + Cx^T + fcov + diag(var_x)
                pmeans[t], pcovs[t] = m-, P-
                where cond[t, n], for j in 0..Dy-1:  s = P-[j, j] + var_y[j];  delta = y[t, n, j] - m-[j];  g = P-[:, j] / s
                                                     m- += g delta;  P- -= s g g^T
                                                     loglik[n] -= (log(2 pi s) + delta^2 / s) / 2
                means[t], covs[t] = m, P = m-, P-

        Arguments, shapes, the None conventions and the checks are `ekf`'s: m0 (N, out_dim), P0 (N, out_dim, out_dim) or
        None (zero; only the lower triangle is read), a (T, N, in_dim - out_dim) or None, y (T, N, Dy) with
        1 <= Dy <= out_dim, var_x (out_dim) or None, var_y (Dy), cond (T, N) of 0 / 1 or None (condition everywhere).  The
        branch on cond is a select: y may hold NaN where cond = 0, it reaches no result; cond = 0 everywhere is exact-moment
        uncertainty propagation with loglik exactly 0.  Returns the namedtuple AdfResult(means (T, N, out_dim), covs
        (T, N, out_dim, out_dim), loglik (N), pmeans, pcovs, cross (T, N, out_dim, out_dim), info (N) int64).  Every
        covs[t, n] and pcovs[t, n] is bitwise symmetric.  info[n] is 0, or t + 1 for the first step at which a
        factorisation of chain n met a non-positive or non-finite pivot, or one below the floor that a positive
        semi-definite belief keeps it above (1 for I + S~, 1/2 for I/2 + S~: this flags a negative definite P0 whose two
        factors exist) -- possible only when P0 is not positive semi-definite: from that step on that chain's results and its loglik are NaN, and no other chain is affected.
        Two calls give bitwise-identical results, and a chain's results do not depend on the other chains of the call.  No
        host synchronisation; nothing is launched without a chain or a step.  Float64, diagonal q(z), forward in time.
        Evaluation only by default: the results carry no grad_fn whatever the leaves or the inputs ask for.

        input_grads=True (named as on `moment_match`): when grad is enabled and one of m0, P0, a, y, var_x, var_y requires
        it, means, covs and loglik carry a grad_fn into those six -- the same launch forward (bitwise the same seven
        results), one fused reverse-time adjoint launch backward, once differentiable; pmeans, pcovs, cross and info never
        do.  The model is a constant of the call -- the values its leaves had at the call: the five leaves get no gradient
        from these results whatever their requires_grad says.  The conventions are `ekf`'s: the gradient for P0 is that of
        the function of tril(P0) + tril(P0, -1)^T (exactly zero above the diagonal, both contributions on a strictly lower
        entry); an argument given as None has no gradient; the gradient for y is exactly 0 where cond = 0 (y may be NaN
        there), and with cond = 0 everywhere those for y and var_y are zero tensors; cond gets none; the cotangent for covs
        need not be symmetric; a result the loss does not use costs nothing.  Where info[n] != 0 the rows of chain n of the
        gradients for m0, P0, a and y are NaN, those for var_x and var_y are NaN (the loss itself is), and the rows of every
        other chain are unaffected.  Raises ValueError on a q_full=True model and when in_dim < out_dim."""
        self._no_full_q('adf')
        from ..hip import autograd as _ag
        y = _f64(y, self.zeta_pos.device)
        pack = self._prepared() if y.shape[0] * y.shape[1] else self._pack       # (nothing runs without a chain or a step)
        if input_grads:
            return _ag.gp_adf(pack, m0, P0, a, y, var_x, var_y, cond=cond)
        return _ag.gp_adf_eval(pack, m0, P0, a, y, var_x, var_y, cond=cond)

    def ads(self, m0, P0, a, y, var_x, var_y, cond=None, lag_one=False):
        """The Rauch-Tung-Striebel smoother behind `adf`.  The forward pass is `adf` itself (arguments and checks are its
        own; means, covs, loglik, pmeans, pcovs are its results, bitwise); the backward sweep is `eks`'s, on
        cross[t] = P + Cx:

            (smeans, scovs)[T-1] = (means, covs)[T-1]
            for t in T-1..0:   G = cross[t]^T (P-_t)^-1                                   (the ADF smoother gain)
                               smeans[t-1] = means[t-1] + G (smeans[t] - pmeans[t])
                               scovs[t-1]  = covs[t-1] + G (scovs[t] - pcovs[t]) G^T
                               lag_one[t]  = G scovs[t] = Cov(h_{t-1}, h_t | y)

        where time -1 is the initial belief (m0, P0).  Returns the namedtuple EksResult, fields as in `eks`; scovs and
        init_cov are bitwise symmetric.  info[n] is `adf`'s where that is non-zero -- that chain's smoothed results are then
        NaN throughout -- and otherwise the sweep's, as in `eks`.  No host synchronisation; nothing is launched without a
        chain or a step.  Evaluation only.  Raises ValueError on a q_full=True model and when in_dim < out_dim."""
        self._no_full_q('ads')
        from ..hip import autograd as _ag
        y = _f64(y, self.zeta_pos.device)
        pack = self._prepared() if y.shape[0] * y.shape[1] else self._pack       # (nothing runs without a chain or a step)
        return _ag.gp_ads_eval(pack, m0, P0, a, y, var_x, var_y, cond=cond, lag_one=lag_one)
