"""Two figures for the input gradients of the forward-only variants (profiles/half_input_gradients/README.md):

    python profiles/tools/half_input_grads_cost.py step --variant half  [--workload C2] [--replays 200] [--blocks 3]
    python profiles/tools/half_input_grads_cost.py step --variant prssm
        the DEFAULT train step (HipHalfTrainStep, captured graph; CBFSSMHALF with the GRU recogniser, PR-SSM with the conv
        one): HIP events around `--replays` steps per block after a warm-up, one line of JSON per run.  The recognition
        kernels are shared with the input-gradient path, so this is run alternately on two builds of the library -- this
        tree's and the parent commit's (CBFSSM_TREE for its package, CBFSSM_HIP_LIB for its library), one process per block group -- and the difference of the
        medians is read against the block-to-block spread of the parent itself.

    python profiles/tools/half_input_grads_cost.py cost --variant half|prssm
        loss_and_grads(input_grads=True) against input_grads=False on ONE engine (eager launches, the path the input
        gradients take), alternated in blocks.

The learning rate is 0 (the Adam launch runs, the parameters stay): the time of a step does not depend on their values."""
import argparse
import json
import os
import sys

# CBFSSM_TREE: root of the checkout whose package is imported (the parent commit's, next to CBFSSM_HIP_LIB for its library)
ROOT = os.environ.get('CBFSSM_TREE') or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'cbf-ssm_amd')]
import numpy as np      # noqa: E402
import torch            # noqa: E402
from cbfssm import synthetic as syn                                         # noqa: E402
from cbfssm.hip import lib                                                  # noqa: E402
from cbfssm.hip.train import TFAdam                                         # noqa: E402
from cbfssm.hip.train_half import HipHalfGrad, HipHalfTrainStep             # noqa: E402


def _timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=('step', 'cost'))
    ap.add_argument('--variant', default='half', choices=('half', 'prssm'))
    ap.add_argument('--workload', default='C2', choices=sorted(syn.WORKLOADS))
    ap.add_argument('--replays', type=int, default=200)
    ap.add_argument('--blocks', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--tag', default='')
    args = ap.parse_args()
    dev = 'cuda:0'
    w = syn.WORKLOADS[args.workload]
    cfg, p = syn.make_variant_params(w, args.variant, 'conv' if args.variant == 'prssm' else 'rnn')
    p = syn.perturb_params(p, scale=0.05)
    cfg['learning_rate'] = 0.0
    u, y = (torch.tensor(a, device=dev) for a in syn.make_inputs(w))
    noise = {'eps_f': torch.tensor(syn.make_noise(w)['eps_f'], device=dev)}
    eng = HipHalfGrad(cfg, dev, variant=args.variant)
    assert eng.fused_gru or eng.fused_conv
    opt = TFAdam({k: torch.tensor(v, device=dev) for k, v in p.items()}, cfg['learning_rate'])
    res = {'mode': args.mode, 'variant': args.variant, 'workload': w.name, 'tag': args.tag, 'lib': lib.LIB_PATH,
           'replays': args.replays}
    if args.mode == 'step':
        st = HipHalfTrainStep(eng, opt, graph=True)
        for _ in range(args.warmup):
            loss = float(st.step(u, y, noise, True))
        torch.cuda.synchronize()
        res['loss'] = loss
        res['ms'] = [_timed(lambda: st.step(u, y, noise, True), args.replays) for _ in range(args.blocks)]
    else:
        ms = {False: [], True: []}
        for ig in (False, True):
            for _ in range(args.warmup):
                eng.loss_and_grads(opt.views, u, y, noise, True, input_grads=ig)
        torch.cuda.synchronize()
        for _ in range(args.blocks):
            for ig in (False, True):
                ms[ig].append(_timed(lambda: eng.loss_and_grads(opt.views, u, y, noise, True, input_grads=ig), args.replays))
        res['ms_default'], res['ms_input_grads'] = ms[False], ms[True]
        res['median_default'], res['median_input_grads'] = float(np.median(ms[False])), float(np.median(ms[True]))
        res['extra_ms'] = res['median_input_grads'] - res['median_default']
    print('HALF_IN_COST ' + json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
