"""The CBF-SSM loss as a differentiable torch function over the HIP engine.

    loss = elbo_loss(engine, params, u, y, noise, condition=True)

`engine` is a cbfssm.hip.train.HipElboGrad, `params` the dict of its twelve unconstrained tensors (train.PARAM_NAMES),
`u` (B,T,dim_u) and `y` (B,T,dim_y) float64 device tensors, `noise` the dict of standard-normal draws the engine takes.
loss.backward() then fills .grad of every parameter tensor that requires it AND of whatever produced u and y: a learnable
input gain or bias, a sensor calibration, a feature map or an encoder in front of the model trains through the
hand-written time loops.  This is what tf.gradients(model.loss, model.sample_in) / (model.loss, model.sample_out) give
in the reference's graph (base_model.py:22-27; cbfssm/model/voliro.py:106-137 trains a GP through it).

The forward call runs the engine's loss_and_grads once -- forward evaluation and adjoint time loops -- and keeps copies
of the gradients; backward only scales them.  The input gradients (the engine's input_grads=True path: float64, no
process group) are computed only when u or y requires grad, or when `input_grads=True` asks for them; with
`input_grads=False` the call is the engine's default adjoint and u, y receive no gradient.  Nothing here computes on
the host or in the tensor library: a missing kernel is the engine's error.
"""
import torch

from .train import PARAM_NAMES


class _ElboLoss(torch.autograd.Function):

    @staticmethod
    def forward(ctx, engine, condition, noise, input_grads, u, y, *params):
        pd = {k: p.detach() for k, p in zip(PARAM_NAMES, params)}
        want_in = bool(ctx.needs_input_grad[4] or ctx.needs_input_grad[5]) if input_grads is None else bool(input_grads)
        loss, grads, terms = engine.loss_and_grads(pd, u.detach(), y.detach(), noise, condition, input_grads=want_in)
        # (the engine's gradient tensors are views of buffers the next evaluation overwrites)
        ctx.grads = tuple(grads[k].clone() for k in PARAM_NAMES)
        ctx.gu = grads['u'].clone() if want_in else None
        ctx.gy = grads['y'].clone() if want_in else None
        ctx.shapes = tuple(p.shape for p in params)
        return loss.detach().clone()

    @staticmethod
    def backward(ctx, gout):
        need = ctx.needs_input_grad
        gu = ctx.gu * gout if (need[4] and ctx.gu is not None) else None
        gy = ctx.gy * gout if (need[5] and ctx.gy is not None) else None
        gp = tuple((g * gout).reshape(s) if need[6 + i] else None for i, (g, s) in enumerate(zip(ctx.grads, ctx.shapes)))
        return (None, None, None, None, gu, gy) + gp


def elbo_loss(engine, params, u, y, noise, condition=True, input_grads=None):
    """The loss of one mini-batch as a 0-d tensor with a grad_fn (see the module docstring).

    input_grads: None -- d loss / d u and d loss / d y are computed when u or y requires grad; True -- always; False --
    never (u and y get no gradient; loss and parameter gradients are those of engine.loss_and_grads as it always was)."""
    missing = [k for k in PARAM_NAMES if k not in params]
    if missing:
        raise KeyError('elbo_loss: params lacks %s' % ', '.join(missing))
    if input_grads is False and (getattr(u, 'requires_grad', False) or getattr(y, 'requires_grad', False)):
        u, y = u.detach(), y.detach()
    return _ElboLoss.apply(engine, bool(condition), noise, input_grads, u, y, *[params[k] for k in PARAM_NAMES])
