"""CBFSSMHALF on the HIP path (reference cbfssm/model/cbfssmhalf.py): forward-only variant -- x_0 comes from a
recognition model, the Kalman-style update acts on the observed state dims only, the ELBO has no backward GP and no
entropy term (cbfssmhalf.py:174-199).

The time loop and its adjoint run in the same kernels as CBFSSM's forward pass (problem.half = 1,
include/cbfssm_hip.h: cbfssm_half_forward_pass_f64 / _bwd_f64).  The recognition model is a GRU(16) over
recog_len steps + a dense layer on B sequences (cbfssmhalf.py:82-93), or for PR-SSM conv1d -> max_pool -> dense in float32
(prssm.py:146-157) -- a few hundred FLOPs per sequence: two launches each (cbfssm_gru_recog[_bwd]_f64,
cbfssm_conv_recog[_bwd]_f32), the backward one taking d loss / d x_0 from the adjoint kernel.  The tensor-library
restatements below stay as cross-checks (CBFSSM_TORCH_GRU=1, CBFSSM_TORCH_CONV=1) and for shapes beyond the kernels' limits.
"""
import ctypes as C
import os
import types
import torch

from . import lib as _l
from . import ops
from .ops import _ptr, _stream, _f64, tf_forward, GPPack
from .dist_utils import all_reduce_sum
from .train import (StashContract, FlatDict, _gp_adjoint, _timed, repacks_f32, repack_f32, g_mode, kgk_image,
                    need_input_grads, gp_unc_grads)

GP_NAMES = ('f.zeta_pos', 'f.zeta_mean', 'f.zeta_var_unc', 'f.variance_unc', 'f.lengthscales_unc')
RECOG_NAMES = ('recog.gate_kernel', 'recog.gate_bias', 'recog.cand_kernel', 'recog.cand_bias', 'recog.dense_kernel',
               'recog.dense_bias')
GRU_UNITS = 16      # cbfssmhalf.py:84


CONV_NAMES = ('recog.conv_kernel', 'recog.conv_bias', 'recog.dense_kernel', 'recog.dense_bias')
PRSSM_GP_NAMES = ('zeta_pos', 'zeta_mean', 'zeta_var_unc', 'variance_unc', 'lengthscales_unc')


def half_param_names(config, variant='half'):
    if variant == 'prssm':
        names = PRSSM_GP_NAMES + ('var_x_unc', 'var_y_unc')
        recog = config['recog_model']
    else:
        names = GP_NAMES + ('var_x_unc', 'var_y_unc')
        recog = config.get('recog_model', 'rnn')
    if recog == 'rnn':
        names = names + RECOG_NAMES
    elif recog == 'conv':
        names = names + CONV_NAMES
    return names


def conv_recognition(recog, u, y, recog_len):
    """prssm.py:143-155: conv1d(5, 3, relu) -> max_pool(2, 2) -> dense, in float32 as the reference casts it."""
    uy = torch.cat((u, y), dim=2)[:, :recog_len, :].to(torch.float32)
    k = recog['recog.conv_kernel'].to(torch.float32)                      # TF layout (width, in, out)
    x = torch.nn.functional.conv1d(uy.permute(0, 2, 1), k.permute(2, 1, 0), recog['recog.conv_bias'].to(torch.float32))
    x = torch.nn.functional.max_pool1d(torch.relu(x), 2, 2)
    x = x.permute(0, 2, 1).reshape(u.shape[0], -1)
    out = x @ recog['recog.dense_kernel'].to(torch.float32) + recog['recog.dense_bias'].to(torch.float32)
    return out.to(torch.float64)


def gru_recognition(recog, u, y, recog_len):
    """TF-1.8 GRUCell(16) over the reversed first recog_len steps of [u, y], then dense -> dim_x (cbfssmhalf.py:82-93)."""
    uy = torch.flip(torch.cat((u, y), dim=2)[:, :recog_len, :], dims=[1])
    h = torch.zeros(u.shape[0], GRU_UNITS, dtype=u.dtype, device=u.device)
    for t in range(uy.shape[1]):
        x = uy[:, t, :]
        gates = torch.sigmoid(torch.cat((x, h), 1) @ recog['recog.gate_kernel'] + recog['recog.gate_bias'])
        r, z = torch.chunk(gates, 2, dim=1)
        c = torch.tanh(torch.cat((x, r * h), 1) @ recog['recog.cand_kernel'] + recog['recog.cand_bias'])
        h = z * h + (1.0 - z) * c
    return h @ recog['recog.dense_kernel'] + recog['recog.dense_bias']


# ---- recognisers: x_0 of every sequence and, from d loss / d x_0, the gradients of the tensors they own.  An engine picks
# one at construction and calls forward(params, p, u, y, keep, want_window) -> x0 (B, dim_x), contiguous and detached, then
# backward(gx0_b, gwin, st) -> {name: gradient}; gwin: the (B, R, dim_u + dim_y) window adjoint to fill, or None.  What
# backward needs stays on the object (one evaluation is in flight per engine, as for ops.TilePool).
class OutputRecogniser:
    """x_0 = [y_0, 0] (recog_model 'output'): no parameters, and the adjoint of x_0 goes to y_0 directly (half_input_grads
    takes gx0 instead of a window adjoint)"""
    names = ()

    def __init__(self, n_hidden):
        self.n_hidden = n_hidden

    def forward(self, params, p, u, y, keep, want_window):
        pad = torch.zeros(u.shape[0], self.n_hidden, dtype=u.dtype, device=u.device)
        return torch.cat((y[:, 0, :], pad), dim=1).contiguous().detach()

    def backward(self, gx0_b, gwin, st):
        return {}


# what tells the two fused recognition models apart: (tensor names, the param_elems symbol and whether it takes recog_len,
# whether an activation buffer (cbfssm_gru_recog_act_elems) goes along, the forward / backward / backward `_in` symbols)
KERNELS = {'gru': (RECOG_NAMES, 'cbfssm_gru_recog_param_elems', False, True,
                   'cbfssm_gru_recog_f64', 'cbfssm_gru_recog_bwd_f64', 'cbfssm_gru_recog_bwd_in_f64'),
           'conv': (CONV_NAMES, 'cbfssm_conv_recog_param_elems', True, False,
                    'cbfssm_conv_recog_f32', 'cbfssm_conv_recog_bwd_f32', 'cbfssm_conv_recog_bwd_in_f32')}


class KernelRecogniser:
    """the GRU (float64) or the conv model (float32) as two launches, cbfssm_{gru,conv}_recog[_bwd[_in]]_*: one wave per
    sequence, per-sequence gradient slabs reduced in fixed order into one vector that the returned gradients view"""

    def __init__(self, kind, dims, recog_len, device):
        self.names, self.elems, self.elems_R, self.has_act, *self.syms = KERNELS[kind]
        self.fns = [getattr(_l.load(), s) for s in self.syms]                   # forward, backward, backward `_in`
        self.dims, self.recog_len, self.device = dims, recog_len, device        # dims: (dim_u, dim_y, dim_x)
        self._bufs = {}
        self._held = None

    def _flat(self, params, p):
        """the recognition tensors (six of the GRU, four of the conv model) as one flat vector: the tail of the optimiser's own
        storage when `params` are its views"""
        names = self.names
        flat = getattr(params, 'flat', None)
        n = sum(p[k].numel() for k in names)
        if flat is not None and flat.device == self.device and tuple(params.keys())[-len(names):] == names:
            return flat[flat.numel() - n:]
        return torch.cat([p[k].reshape(-1) for k in names])

    def forward(self, params, p, u, y, keep, want_window):
        lib = _l.load()
        B, T = u.shape[0], u.shape[1]
        R = min(self.recog_len, T)                           # (the window is the first recog_len steps: all of a shorter sequence)
        rflat = self._flat(params, p)
        if (B, R) not in self._bufs:
            f = dict(dtype=torch.float64, device=self.device)
            P = int(getattr(lib, self.elems)(*self.dims, *((R,) if self.elems_R else ())))
            self._bufs[B, R] = types.SimpleNamespace(
                P=P, x0=torch.zeros(B, self.dims[2], **f),
                act=torch.zeros(int(lib.cbfssm_gru_recog_act_elems(B, R)), **f) if self.has_act else None,
                gpart=torch.zeros((B + 32) * max(P, 0), **f))
        b = self._bufs[B, R]
        a = (B, T, *self.dims, R, _ptr(u), _ptr(y), _ptr(rflat))
        if keep:    # (with the tensors behind the pointers: alive until backward, which lets go of them)
            self._held = (b, a, (u, y, rflat), [(k, p[k].shape) for k in self.names])
        act = (_ptr(b.act) if keep else None,) if self.has_act else ()
        _l.check(self.fns[0](*a, _ptr(b.x0), *act, _stream()), self.syms[0])
        return b.x0

    def backward(self, gx0_b, gwin, st):
        (b, a, _, shapes), self._held = self._held, None
        a = a + ((_ptr(b.act),) if self.has_act else ()) + (_ptr(gx0_b.contiguous()), _ptr(b.gpart))
        if gwin is not None:
            _l.check(self.fns[2](*a, _ptr(gwin), st), self.syms[2])
        else:
            _l.check(self.fns[1](*a, st), self.syms[1])
        rg = torch.zeros(b.P, dtype=torch.float64, device=self.device)
        ops.reduce_partials(b.gpart, b.P, gx0_b.shape[0], rg, st)
        grads, o = {}, 0
        for k, shape in shapes:
            grads[k] = rg[o:o + shape.numel()].view(shape)
            o += shape.numel()
        return grads


class TorchRecogniser:
    """gru_recognition / conv_recognition above through the tensor library's autograd: the cross-check of the kernels
    (CBFSSM_TORCH_GRU=1, CBFSSM_TORCH_CONV=1) and the conv model at a recog_len beyond their limits"""

    def __init__(self, names, recog_len):
        self.names, self.recog_len = names, recog_len

    def _fn(self):      # looked up in this module at every call: a test swaps the two functions to prove who runs them
        return gru_recognition if self.names is RECOG_NAMES else conv_recognition

    def forward(self, params, p, u, y, keep, want_window):
        if not keep:
            return self._fn()(p, u, y, self.recog_len).contiguous()
        self.rp = {k: p[k].detach().clone().requires_grad_(True) for k in self.names}
        self.win = ()
        if want_window:         # the window's adjoint comes from the tensor library's autograd too
            R = min(self.recog_len, u.shape[1])
            self.win = tuple(t[:, :R].detach().clone().requires_grad_(True) for t in (u, y))
        self.x0g = self._fn()(self.rp, *(self.win or (u, y)), self.recog_len)
        return self.x0g.detach().contiguous()

    def backward(self, gx0_b, gwin, st):
        gl = torch.autograd.grad(self.x0g, [self.rp[k] for k in self.names] + list(self.win), grad_outputs=gx0_b)
        self.x0g = self.rp = self.win = None
        if gwin is not None:
            gwin.copy_(torch.cat(gl[len(self.names):], dim=2))
        return dict(zip(self.names, gl))


class HipHalfGrad:
    """loss and gradients of CBFSSMHALF for one mini-batch on one device."""

    def __init__(self, config, device, dist=None, variant='half', dtype='float64'):
        """variant 'half': CBFSSMHALF.  variant 'prssm': the PR-SSM baseline (reference cbfssm/model/prssm.py) -- the same
        pass with the Kalman update switched off everywhere (free run), loss = -(lambda0 * loglik - KL_z) with the KL
        prior factorised WITHOUT jitter (prssm.py:81-82,96) and one shared lengthscale (prssm.py:40).

        dtype 'float32' (the reference's model dtype argument, cbfssmhalf.py:17 / prssm.py:17): the time loop and its adjoint
        compute in float32 (cbfssm_half_forward_pass_f32 / _bwd_f32); K_mm / Cholesky / K^-1, the recognition model, the train
        tail and the optimizer step stay float64, as in HipElboGrad."""
        assert dtype in ('float64', 'float32')
        self.f32 = dtype == 'float32'
        self.config = config
        self.variant = variant
        self.device = torch.device(device)
        self.dist = dist
        self.dim_u, self.dim_y, self.dim_x = config['ds'].dim_u, config['ds'].dim_y, config['dim_x']
        self.M, self.S = config['ind_pnt_num'], config['samples']
        self.D = self.dim_x + self.dim_u
        self.names = half_param_names(config, variant)
        self.rnn = 'recog.gate_kernel' in self.names
        self.conv = 'recog.conv_kernel' in self.names
        self.pre = '' if variant == 'prssm' else 'f.'
        # loss = -(cL * (loglik - kl_x) - KL_z): cL = lambda0 / S for CBFSSMHALF, lambda0 for PR-SSM
        lf0 = float(config['loss_factors'][0])
        self.cL = lf0 if variant == 'prssm' else lf0 / self.S
        self.pack_kl = GPPack(self.M, self.D, self.dim_x, self.device) if variant == 'prssm' else None
        self.pack_f = GPPack(self.M, self.D, self.dim_x, self.device, ops.gp_form_mode_f32(config) if self.f32 else None)
        if self.f32:
            self.pack_f.cond_threshold = min(self.pack_f.cond_threshold, ops.F32_FORM_COND)
            # per-workgroup slabs of the float32 adjoint: the non-stash layout at every tile height (matrix section included)
            self.slab32_f = int(_l.load().cbfssm_rev32_slab_elems(C.byref(self.pack_f.layout)))
        self.stash = bool(self.pack_f.layout.rev_stash)
        self.repack32 = repacks_f32(self.f32, self.pack_f.layout)
        self._tmp32 = None
        self.stash_bytes = int(float(config.get('adjoint_stash_gib', 4.0)) * 2 ** 30)
        self._stash_buf = None
        self.slab_f = int(self.pack_f.layout.rev_slab)
        self._ws = {}
        self.last_ws = None
        # the K_mm / Cholesky / prior-KL adjoint is shared with CBFSSM: cbfssm_train_tail_half_f64 (five launches on flat
        # vectors); CBFSSM_TORCH_TAIL=1 keeps the tensor-library restatement (train._gp_adjoint: same numbers, a cross-check)
        self.fused_tail = self.slab_f > 0 and not os.environ.get('CBFSSM_TORCH_TAIL')
        self.gp_names = self.names[:7]                       # the five GP tensors, var_x_unc, var_y_unc: the tail's flat order
        self.tail_work = None
        # the recogniser: the GRU as two launches instead of ~800 tensor-library launches through autograd (CBFSSM_TORCH_GRU=1
        # keeps the latter: same numbers, a cross-check); the conv model likewise (CBFSSM_TORCH_CONV=1), the tensor library
        # also serving a recog_len beyond the kernels' limits (the library says where they are: param_elems < 0)
        dims, R = (self.dim_u, self.dim_y, self.dim_x), int(config['recog_len'])
        self.fused_gru = self.rnn and not os.environ.get('CBFSSM_TORCH_GRU')
        self.fused_conv = (self.conv and not os.environ.get('CBFSSM_TORCH_CONV') and
                           int(_l.load().cbfssm_conv_recog_param_elems(*dims, R)) >= 0)
        if self.fused_gru or self.fused_conv:
            self.recog = KernelRecogniser('gru' if self.rnn else 'conv', dims, R, self.device)
        elif self.rnn or self.conv:
            self.recog = TorchRecogniser(RECOG_NAMES if self.rnn else CONV_NAMES, R)
        else:
            self.recog = OutputRecogniser(self.dim_x - self.dim_y)

    def _problem(self, B, T, condition):
        c = self.config
        if self.variant == 'prssm':      # never condition: recog_len 1 and condition False make every step a free run
            return _l.make_problem(B, self.S, T, self.dim_x, self.dim_u, self.dim_y, self.M, 1, 1.0, False, half=True)
        return _l.make_problem(B, self.S, T, self.dim_x, self.dim_u, self.dim_y, self.M, c['recog_len'], c['k_factor'],
                               condition, half=True)

    def _forward(self, lp, p, c):
        st = _stream()
        pre = self.pre
        self.pack_f.prepare(p[pre + 'zeta_pos'], c['ls'], c['var'], p[pre + 'zeta_mean'], c['zvar'])
        if self.pack_kl is not None:
            self.pack_kl.prepare(p[pre + 'zeta_pos'], c['ls'], c['var'], p[pre + 'zeta_mean'], c['zvar'], jitter=0.0)
        lp.cast_f32()
        _timed(getattr(self, '_prof', None), 'forward_pass', None, lambda: lp.half_forward_pass(lp.prob, st))
        lp.elbo_tail(self.cL * self.S, 0.0, st, kl_pack=self.pack_kl)

    def _constrained(self, p):
        pre = self.pre
        ls = tf_forward(p[pre + 'lengthscales_unc']).reshape(-1)
        if ls.numel() == 1:                                  # PR-SSM: one lengthscale for all input dims (prssm.py:40)
            ls = ls.expand(self.D)
        return {'ls': ls.contiguous(),
                'var': tf_forward(p[pre + 'variance_unc']).reshape(-1).contiguous(),
                'zvar': tf_forward(p[pre + 'zeta_var_unc']).contiguous(),
                'var_x': tf_forward(p['var_x_unc']).contiguous(), 'var_y': tf_forward(p['var_y_unc']).contiguous()}

    def _workspace(self, prob):
        key = (prob.B, prob.T)
        if key not in self._ws:
            lib = _l.load()
            f = dict(dtype=torch.float64, device=self.device)
            N = prob.B * prob.S
            ws = types.SimpleNamespace()
            ws.n_kl = int(lib.cbfssm_forward_pass_partials(C.byref(prob)))
            ws.n_f = int(lib.cbfssm_rev_workgroups(C.byref(prob), 0))
            ws.x = torch.zeros(prob.T, N, prob.dim_x, **f)
            ws.fmv_f = torch.zeros(max(prob.T - 1, 0), N, prob.dim_x, 2, **f)
            if self.f32:    # every step's [A2 | kernel tile] registers of the float32 pass, float32 (held in a float64 buffer)
                n_a2 = int(lib.cbfssm_saved_a2_f32_elems(C.byref(prob), C.byref(self.pack_f.layout), 0))
                assert n_a2 > 0 or prob.T == 1
                n_a2 = max((n_a2 + 1) // 2, 1)
            else:
                n_a2 = int(lib.cbfssm_saved_a2_elems(C.byref(prob), C.byref(self.pack_f.layout), 0))
            if getattr(self, 'tile_pool', None) is None:
                self.tile_pool = ops.TilePool(self.device)
            ws.a2s_f, _ = self.tile_pool.get(n_a2, 0)
            ws.kl_part = torch.zeros(ws.n_kl, **f)
            ws.ll_part = torch.zeros(int(lib.cbfssm_loglik_partials(C.byref(prob))), **f)   # [block][dim_y]
            ws.pred_mean = torch.zeros(prob.B, prob.T, prob.dim_y, **f)
            ws.pred_var = torch.zeros(prob.B, prob.T, prob.dim_y, **f)
            ws.int_mean = torch.zeros(prob.B, prob.T, prob.dim_x, **f)
            ws.int_var = torch.zeros(prob.B, prob.T, prob.dim_x, **f)
            ws.out = torch.zeros(8, **f)
            ws.y2 = torch.zeros(prob.T, N, max(0, prob.dim_x - prob.dim_y), **f)      # (surface compatibility)
            ws.gx0 = torch.zeros(N, prob.dim_x, **f)
            ws.gx_carry = torch.zeros(N, prob.dim_x, **f)
            ws.gpart_f = torch.zeros((ws.n_f + 32) * (self.slab32_f if self.f32 else self.slab_f), **f)
            ws.red = torch.zeros(self.slab_f + 3 + prob.dim_y, **f)     # [slab | loglik, kl_x, 0, d loss / d var_y]
            self._ws[key] = ws
        return self._ws[key]

    def _terms(self, ws, red2=None):
        out = ws.out
        cL = self.cL
        if red2 is None:
            loglik, kl_x = out[0], out[1]
        else:
            loglik, kl_x = red2[0], red2[1]
        loss = -(loglik * cL - kl_x * cL - out[3])                                 # cbfssmhalf.py:195-199
        z = torch.zeros((), dtype=torch.float64, device=self.device)
        return loss, {'loglik': loglik, 'kl_x': kl_x, 'entropy': z, 'kl_z_f': out[3], 'kl_z_b': z, 'info': out[7]}

    def _evaluate(self, params, u, y, noise, condition, grad=False, input_grads=False):
        """what forward() and loss_and_grads() share: the casts, the problem and its workspace, the constrained parameters, x_0
        from the recogniser and the forward evaluation.  Returns (p, c, lp): lp the time-loop entry points bound to all of it.
        grad: the recogniser and the pass keep what their adjoints need."""
        dev = self.device
        p = {k: _f64(params[k], dev) for k in self.names}
        u, y = _f64(u, dev), _f64(y, dev)
        prob = self._problem(u.shape[0], u.shape[1], condition)
        self.last_ws = ws = self._workspace(prob)
        # (forward() has always evaluated the recogniser ahead of the transforms, loss_and_grads() behind them: kept, so that
        # either issues the launches it always did, in their order)
        if not grad:
            with torch.no_grad():
                x0 = self.recog.forward(params, p, u, y, False, False)
        c = self._constrained(p)
        eps_f = _f64(noise['eps_f'], dev)
        if grad:
            x0 = self.recog.forward(params, p, u, y, True, input_grads)
        lp = ops.TimeLoops(prob, ws, self.pack_f, None, c['var_x'], c['var_y'], u, y, eps_f, x0=x0, cL=self.cL, f32=self.f32)
        if input_grads:
            lp.in_bufs = self._input_buffers(prob, ws)
        self._forward(lp, p, c)
        return p, c, lp

    def forward(self, params, u, y, noise, condition=True, weight=1.0, local=False):
        ws = self._evaluate(params, u, y, noise, condition)[2].ws
        red2 = None
        if self.dist is not None and not local:
            red2 = ws.out[0:2].clone()
            if weight != 1.0:
                red2.mul_(float(weight))
            all_reduce_sum(red2, self.dist)
        loss, terms = self._terms(ws, red2)
        return loss, terms, ws

    def _need_input_grads(self):
        need_input_grads(self.f32, self.dist)

    def _window(self, T):
        """rows of u, y that the recognition model reads"""
        return min(int(self.config['recog_len']), T)

    def _input_buffers(self, prob, ws):
        """per-chain buffers of the `_in` adjoint (gin_f, -, gyo), the window adjoint and the two results, kept with the
        workspace"""
        if getattr(ws, 'in_bufs', None) is None:
            lib = _l.load()
            f = dict(dtype=torch.float64, device=self.device)
            n_f, n_o = (int(fn(C.byref(prob))) for fn in (lib.cbfssm_input_adjoint_fwd_elems, lib.cbfssm_input_adjoint_obs_elems))
            assert min(n_f, n_o) >= 0, (n_f, n_o)
            ws.in_bufs = (torch.zeros(max(n_f, 1), **f), None, torch.zeros(max(n_o, 1), **f))
            ws.gwin = torch.zeros(prob.B, self._window(prob.T), prob.dim_u + prob.dim_y, **f)
            ws.grad_u = torch.zeros(prob.B, prob.T, prob.dim_u, **f)
            ws.grad_y = torch.zeros(prob.B, prob.T, prob.dim_y, **f)
        return ws.in_bufs

    def _adjoint(self, lp, ws, prof, st):
        """the adjoint of the time loop, its per-workgroup slabs reduced into ws.red[:slab_f].  Returns the image of
        d loss / d K^-1 that goes beside the slab (stash tile heights), or None."""
        prob, sf, red, dev = lp.prob, self.slab_f, ws.red, self.device
        if self.stash and not self.f32:
            # float64 at M > 112: time-chunked launches that fit the stash, each followed by its reduction and the GEMM that
            # contracts the stashed A2bar / K tiles into the image (the forward-pass half of HipElboGrad._adjoint_stash)
            groups = (prob.B * self.S + 15) // 16
            Mp = self.pack_f.layout.Mp
            cols_max = max(groups * 16, self.stash_bytes // (2 * Mp * 8))
            f = dict(dtype=torch.float64, device=dev)
            if self._stash_buf is None or self._stash_buf[0].numel() < Mp * cols_max:
                self._stash_buf = (torch.zeros(Mp * cols_max, **f), torch.zeros(Mp * cols_max, **f))
            sa, sk = self._stash_buf
            if getattr(self, '_contract', None) is None:
                self._contract = StashContract(self.pack_f, dev)
            self._contract.image.zero_()
            tmp = torch.zeros(sf, **f)
            red[:sf].zero_()
            per = max(1, cols_max // (groups * 16))
            t_hi = prob.T - 2
            while True:
                t_lo = max(0, t_hi - per + 1)
                cols = groups * max(0, t_hi - t_lo + 1) * 16
                _timed(prof, 'forward_pass_adjoint', None,
                       lambda: lp.half_forward_pass_bwd(prob, st, (t_hi, t_lo, sa, sk, cols)))
                ops.reduce_partials(ws.gpart_f, sf, groups, tmp, st)
                red[:sf] += tmp
                if cols:
                    _timed(prof, 'stash_contraction', None, lambda: self._contract.add(sa, sk, cols, st))
                t_hi = t_lo - 1
                if t_hi < 0:
                    return self._contract.image
        # one launch for the whole time loop (float32: at every tile height, into the non-stash slab)
        _timed(prof, 'forward_pass_adjoint', None, lambda: lp.half_forward_pass_bwd(prob, st))
        if not self.repack32:
            assert not self.f32 or self.slab32_f == sf
            ops.reduce_partials(ws.gpart_f, sf, ws.n_f, red[:sf], st)
            return None
        s32, nb = self.slab32_f, self.pack_f.layout.NBLK
        if self._tmp32 is None:
            self._tmp32 = torch.zeros(s32 + nb * nb * 256, dtype=torch.float64, device=dev)
        t32, gB = self._tmp32[:s32], self._tmp32[s32:]
        ops.reduce_partials(ws.gpart_f, s32, ws.n_f, t32, st)
        repack_f32(t32, red[:sf], gB, nb)
        return gB

    def _all_reduce(self, pieces, weight):
        """the ONE collective of a step, over one flat buffer of the pieces, which take their sums back"""
        flat = torch.cat([t.reshape(-1) for t in pieces])
        if weight != 1.0:
            flat.mul_(float(weight))
        all_reduce_sum(flat, self.dist)
        o = 0
        for t in pieces:
            t.copy_(flat[o:o + t.numel()].view_as(t))
            o += t.numel()

    def _param_grads(self, params, p, c, red, gB, rgrads, st):
        """from the reduced slab (and image) to the gradients of the unconstrained tensors; the recogniser's ride along"""
        lib, dev, pre, sf = _l.load(), self.device, self.pre, self.slab_f
        if self.fused_tail:
            # the K_mm -> Cholesky -> K^-1 adjoint, the prior KL and the chain through the positivity transforms in HIP
            lay = C.byref(self.pack_f.layout)
            gp = [p[k].reshape(-1) for k in self.gp_names]
            pflat = getattr(params, 'flat', None)
            ngp = sum(t.numel() for t in gp)
            if pflat is None or pflat.device != dev or list(params.keys())[:7] != list(self.gp_names):
                pflat = torch.cat(gp)
            lsc = tf_forward(p[pre + 'lengthscales_unc']).reshape(-1)
            cflat = torch.cat([gp[0], gp[1], c['zvar'].reshape(-1), c['var'], lsc, c['var_x'], c['var_y']])
            if self.tail_work is None:
                nw = int(lib.cbfssm_train_tail_half_work_elems(lay))
                self.tail_work = torch.zeros(nw, dtype=torch.float64, device=dev)
            gall = torch.zeros(ngp + sum(g.numel() for g in rgrads.values()), dtype=torch.float64, device=dev)
            rc = lib.cbfssm_train_tail_half_f64(lay, _ptr(self.pack_f.buf), _ptr(self.pack_kl.buf) if self.pack_kl is not None else None,
                                                int(lsc.numel() == 1), _ptr(red), _ptr(gB), 0, g_mode(self.f32, self.pack_f.layout), self.dim_y, _ptr(pflat), _ptr(cflat),
                                                _ptr(self.tail_work), _ptr(gall), st)
            _l.check(rc, 'cbfssm_train_tail_half_f64')
            grads = FlatDict()
            grads.flat = gall
            o = 0
            for k in self.gp_names:
                grads[k] = gall[o:o + p[k].numel()].view(p[k].shape)
                o += p[k].numel()
            for k, g in rgrads.items():
                gall[o:o + g.numel()] = g.reshape(-1)
                grads[k] = gall[o:o + g.numel()].view(g.shape)
                o += g.numel()
            return grads
        grads = dict(rgrads)
        if self.f32:
            gB = kgk_image(self.pack_f, red[:sf], gB)
        gz, gmu, gs2, gvar, gls, small = _gp_adjoint(self.pack_f, red[:sf], p[pre + 'zeta_pos'], c['ls'], c['var'],
                                                     p[pre + 'zeta_mean'], c['zvar'], self.dim_x, not self.stash, gB,
                                                     self.pack_kl)
        grads.update(gp_unc_grads(pre, p, gz, gmu, gs2, gvar, gls, shared_ls=p[pre + 'lengthscales_unc'].numel() == 1))
        grads['var_x_unc'] = small[0:self.dim_x] * torch.sigmoid(p['var_x_unc'])
        grads['var_y_unc'] = (small[16:16 + self.dim_y] + red[sf + 3:]) * torch.sigmoid(p['var_y_unc'])
        return grads

    def loss_and_grads(self, params, u, y, noise, condition=True, weight=1.0, local=False, input_grads=False):
        """input_grads: the grads also hold 'u' (B,T,dim_u) and 'y' (B,T,dim_y), the gradient of the loss with respect to the
        input and output sequences (tf.gradients(loss, sample_in / sample_out)): through the time loop, the log-likelihood
        and the recognition model's window.  float64 engines without a process group only; an eager path (HipHalfTrainStep
        never takes it)."""
        if input_grads:
            self._need_input_grads()
        p, c, lp = self._evaluate(params, u, y, noise, condition, grad=True, input_grads=input_grads)
        prob, ws, st, rec = lp.prob, lp.ws, _stream(), self.recog
        gB = self._adjoint(lp, ws, getattr(self, '_prof', None), st)
        # data scalars and the log-likelihood's pull on var_y (cbfssmhalf.py:181-189): tail = [loglik, kl_x, 0, d/d var_y]
        tail = ws.red[self.slab_f:]
        _l.check(_l.load().cbfssm_data_tail_f64(C.byref(prob), _ptr(c['var_y']), _ptr(ws.ll_part), _ptr(ws.out), self.cL,
                                                _ptr(tail), st), 'cbfssm_data_tail_f64')
        gx0_b = ws.gx0.view(prob.B, self.S, self.dim_x).sum(1)   # d loss / d x_0 per sequence (tiled over S, :87)
        gwin = ws.gwin if input_grads and rec.names else None
        rgrads = rec.backward(gx0_b, gwin, st)
        if input_grads:
            # x_0 = [y_0, 0] without a recognition model: its adjoint goes to y_0 directly
            lp.half_input_grads(None if rec.names else ws.gx0, gwin, self._window(prob.T), ws.grad_u, ws.grad_y, st)
        if self.dist is not None and not local:
            # [slab | data scalars | stash-mode K^-1-adjoint image | recognition-model gradients]
            self._all_reduce([ws.red] + ([gB] if gB is not None else []) + [rgrads[k].reshape(-1) for k in rec.names], weight)
        loss, terms = self._terms(ws, tail[0:2])
        grads = self._param_grads(params, p, c, ws.red, gB, rgrads, st)
        if input_grads:
            grads['u'], grads['y'] = ws.grad_u, ws.grad_y
        return loss, grads, terms


class HipHalfTrainStep:
    """One `sess.run((model.train, model.loss))` of a forward-only variant (training/trainer.py:40) as ONE HIP-graph replay:
    the recognition model forward and backward (two launches; through the tensor library's autograd under CBFSSM_TORCH_GRU /
    CBFSSM_TORCH_CONV: a few hundred tiny launches for the GRU, most of an eager step at the small-scale shapes), K_mm /
    Cholesky / K^-1, the pass, its adjoint, the train tail and the Adam update.  One graph per (shapes, condition, GP form),
    captured at first use; single device (a data-parallel run keeps eager launches around its collective)."""

    def __init__(self, engine, opt, graph=None):
        self.engine, self.opt = engine, opt
        if graph is None:
            graph = engine.config.get('hip_graph', os.environ.get('CBFSSM_HIP_GRAPH', '1') != '0')
        self.use_graph = bool(graph) and engine.dist is None
        self._graphs = {}
        self.last_terms = self.last_ws = None

    def _eager(self, u, y, noise, condition, **kw):
        loss, grads, terms = self.engine.loss_and_grads(self.opt.views, u, y, noise, condition, **kw)
        self.opt.step(grads)
        self.last_terms, self.last_ws = terms, self.engine.last_ws
        return loss

    def step(self, u, y, noise, condition=True, **kw):
        eng = self.engine
        if not self.use_graph or kw:
            return self._eager(u, y, noise, condition, **kw)
        dev = eng.device
        u, y, eps = _f64(u, dev), _f64(y, dev), _f64(noise['eps_f'], dev)
        # (auto form: a completed condition-number read-back may flip the GP form -- other kernels, another graph)
        forms = tuple(pk.update_form() for pk in (eng.pack_f, eng.pack_kl) if pk is not None)
        key = (tuple(u.shape), tuple(y.shape), bool(condition), forms)
        g = self._graphs.get(key)
        if g is None:
            g = {'u': u.clone(), 'y': y.clone(), 'noise': {'eps_f': eps.clone()}}
            cur = torch.cuda.current_stream(dev)
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(cur)
            with torch.cuda.stream(side):                 # warm-up outside the capture (workspaces, autograd state); no update
                for _ in range(2):
                    eng.loss_and_grads(self.opt.views, g['u'], g['y'], g['noise'], condition)
            cur.wait_stream(side)
            torch.cuda.synchronize(dev)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                loss, grads, terms = eng.loss_and_grads(self.opt.views, g['u'], g['y'], g['noise'], condition)
                if getattr(grads, 'flat', None) is not None:
                    self.opt.step(grads)
                else:
                    self.opt.step_device(grads)
                self.opt._t -= 1                          # capture does not execute; every replay counts below
            g.update(graph=graph, loss=loss, terms=terms, ws=eng.last_ws)
            self._graphs[key] = g
        else:
            g['u'].copy_(u)
            g['y'].copy_(y)
            g['noise']['eps_f'].copy_(eps)
        g['graph'].replay()
        self.opt._t += 1
        self.last_terms, self.last_ws = g['terms'], g['ws']
        return g['loss'].clone()
