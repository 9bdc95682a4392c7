"""HipHalfGrad under a process group: the branch of forward() and loss_and_grads() that packs one flat buffer
[slab | data scalars | stash-mode K^-1-adjoint image | recognition-model gradients], weights it, all-reduces it and copies the
pieces back (tests/test_distributed_gpu.py covers HipElboGrad only).

No torch.distributed and no second process: the group is a stub of world size 2 whose all_reduce doubles the buffer in place.
With weight = 0.5 the collective is then an exact identity in floating point (a scaling by 2^-1 and one by 2, no entry near
the subnormal range), so every number the engine returns must be BITWISE the one of an engine without a group.  An identity
cannot show a piece that was left out of the buffer, so the size of the buffer is asserted too."""
import pytest
import torch

from cbfssm.hip.train_half import HipHalfGrad, half_param_names

import half_input_grads_cases as hc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SWITCHES = ('CBFSSM_TORCH_GRU', 'CBFSSM_TORCH_CONV', 'CBFSSM_TORCH_TAIL')
# (case of half_input_grads_cases, environment switch or None)
CASES = [('half-rnn', None), ('prssm-conv', None), ('half-output', None),
         ('half-rnn-stash', None),                     # the K^-1-adjoint image rides in the flat buffer
         ('half-rnn', 'CBFSSM_TORCH_GRU'),             # the recogniser gradients come from autograd and ride in it
         ('half-rnn', 'CBFSSM_TORCH_TAIL')]


class StubGroup:
    """what dist_utils.all_reduce_sum asks of a process group: two ranks that hold the same buffer"""

    def __init__(self):
        self.calls = 0
        self.numel = None           # of the last buffer

    def get_world_size(self):
        return 2

    def get_backend(self):
        return 'stub'

    def all_reduce(self, t):
        self.calls += 1
        self.numel = t.numel()
        t.mul_(2.0)


def _same_bits(tag, a, b):
    assert a.shape == b.shape and a.dtype == b.dtype, tag
    assert torch.equal(a, b), tag
    assert bool(torch.isfinite(a).all()), tag


@pytest.mark.parametrize('name,env', CASES, ids=['%s%s' % (n, '-' + e if e else '') for n, e in CASES])
def test_process_group_branch_is_an_exact_identity_at_weight_one_half(monkeypatch, name, env):
    for k in SWITCHES + ('CBFSSM_GP_FORM',):
        monkeypatch.delenv(k, raising=False)
    if env:
        monkeypatch.setenv(env, '1')
    variant, w, cfg, p, u, y, noise = hc.setup(name)
    recog = hc.CASES[name][1]
    params = {k: torch.tensor(v, device=DEV) for k, v in p.items()}
    stub = StubGroup()
    res = {}
    for dist in (None, stub):
        eng = HipHalfGrad(cfg, DEV, dist=dist, variant=variant)
        # the case runs the path it is named after
        assert eng.fused_gru == (recog == 'rnn' and env != 'CBFSSM_TORCH_GRU') and eng.fused_conv == (recog == 'conv')
        assert eng.fused_tail == (env != 'CBFSSM_TORCH_TAIL') and eng.stash == (w.M > 112)
        n0 = stub.calls
        loss, grads, terms = eng.loss_and_grads(params, u, y, noise, weight=0.5)
        if dist is not None:
            assert stub.calls == n0 + 1, 'one collective per loss_and_grads'
            # [slab | loglik, kl_x, 0, d loss / d var_y | stash-mode image of d loss / d K^-1 | recogniser gradients]
            nimg = eng.pack_f.layout.NBLK ** 2 * 256 if eng.stash else 0
            nrec = sum(params[k].numel() for k in half_param_names(cfg, variant)[7:])
            assert (nrec > 0) == (recog != 'output')
            assert stub.numel == eng.slab_f + 3 + w.dim_y + nimg + nrec, 'a piece does not ride in the flat buffer'
        out = {'loss': loss.clone(), 'grads': {k: v.clone() for k, v in grads.items()},
               'terms': {k: v.clone() for k, v in terms.items()}}
        n0 = stub.calls
        loss_f, terms_f, _ = eng.forward(params, u, y, noise, weight=0.5)
        if dist is not None:
            assert stub.calls == n0 + 1 and stub.numel == 2, 'one collective per forward: loglik, kl_x'
        out.update(loss_f=loss_f.clone(), terms_f={k: v.clone() for k, v in terms_f.items()})
        torch.cuda.synchronize()
        res[dist is not None] = out
    ref, got = res[False], res[True]
    assert float(ref['terms']['info']) == 0.0 and float(ref['terms_f']['info']) == 0.0
    assert set(ref['grads']) == set(got['grads']) == set(half_param_names(cfg, variant))
    assert set(ref['terms']) == set(got['terms']) and set(ref['terms_f']) == set(got['terms_f'])
    _same_bits('loss', got['loss'], ref['loss'])
    _same_bits('forward loss', got['loss_f'], ref['loss_f'])
    for k in ref['terms']:
        _same_bits('terms ' + k, got['terms'][k], ref['terms'][k])
        _same_bits('forward terms ' + k, got['terms_f'][k], ref['terms_f'][k])
    for k in ref['grads']:
        _same_bits('gradient ' + k, got['grads'][k], ref['grads'][k])
        assert float(ref['grads'][k].abs().max()) > 0.0, ('a gradient of zeros compares nothing', k)
