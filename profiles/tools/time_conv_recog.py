"""PR-SSM train step with the conv recognition model (prssm.py:146-157) through HipHalfTrainStep, the recogniser as the two
HIP launches (cbfssm_conv_recog[_bwd]_f32) against the tensor-library path (CBFSSM_TORCH_CONV=1), both engines in ONE
process, alternated in blocks: HIP events around `--replays` steps per block after a warm-up of both, `--blocks` blocks
each, median and spread printed.

    python profiles/tools/time_conv_recog.py --workload C2            # Actuator shape (M=50, T=100, B=64, S=50)
    python profiles/tools/time_conv_recog.py --workload C3            # Sarcos shape (M=100, T=250, B=256, S=20)
    rocprofv3 --kernel-trace --stats -- python profiles/tools/time_conv_recog.py --workload C2 --only fused --replays 20 --blocks 1
                                                                      # (launches per step: one path per run, no counters)

The learning rate is 0 (the Adam launch runs, the parameters stay): both engines then see the same parameters in every
block, and the time of a step does not depend on their values."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'cbf-ssm_amd')]
import numpy as np      # noqa: E402
import torch            # noqa: E402
from cbfssm import synthetic as syn                                         # noqa: E402
from cbfssm.hip.train import TFAdam                                         # noqa: E402
from cbfssm.hip.train_half import HipHalfGrad, HipHalfTrainStep             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='C2', choices=sorted(syn.WORKLOADS))
    ap.add_argument('--replays', type=int, default=200)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--only', choices=('fused', 'torch'), default=None)
    ap.add_argument('--eager', action='store_true', help='no HIP graph (every launch of a step shows in a kernel trace)')
    args = ap.parse_args()
    dev = 'cuda:0'
    w = syn.WORKLOADS[args.workload]
    cfg, p = syn.make_variant_params(w, 'prssm', 'conv')
    p = syn.perturb_params(p, scale=0.05)
    cfg['learning_rate'] = 0.0
    u, y = (torch.tensor(a, device=dev) for a in syn.make_inputs(w))
    noise = {'eps_f': torch.tensor(syn.make_noise(w)['eps_f'], device=dev)}
    steppers = {}
    for name in ('fused', 'torch'):
        if args.only not in (None, name):
            continue
        if name == 'torch':
            os.environ['CBFSSM_TORCH_CONV'] = '1'
        else:
            os.environ.pop('CBFSSM_TORCH_CONV', None)
        eng = HipHalfGrad(cfg, dev, variant='prssm')
        os.environ.pop('CBFSSM_TORCH_CONV', None)
        assert eng.fused_conv == (name == 'fused')
        opt = TFAdam({k: torch.tensor(v, device=dev) for k, v in p.items()}, cfg['learning_rate'])
        steppers[name] = HipHalfTrainStep(eng, opt, graph=not args.eager)
    print('workload %s: M=%d T=%d B=%d S=%d recog_len=%d dim_u=%d dim_y=%d dim_x=%d, graph %s, %d steps per block, %d blocks'
          % (w.name, w.M, w.T, w.B, w.S, w.recog_len, w.dim_u, w.dim_y, w.dim_x, 'off' if args.eager else 'on', args.replays,
             args.blocks), flush=True)
    loss = {}
    for name, st in steppers.items():
        for _ in range(args.warmup):
            loss[name] = float(st.step(u, y, noise, True))
        torch.cuda.synchronize()
        print('%-5s loss after warm-up %.12g' % (name, loss[name]), flush=True)
    ms = {name: [] for name in steppers}
    for blk in range(args.blocks):
        for name, st in steppers.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.replays):
                st.step(u, y, noise, True)
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.replays)
            print('block %d %-5s %.4f ms/step' % (blk, name, ms[name][-1]), flush=True)
    for name, v in ms.items():
        print('%-5s median %.4f ms/step, min %.4f, max %.4f (spread %.4f) over %d blocks'
              % (name, float(np.median(v)), min(v), max(v), max(v) - min(v), len(v)))
    if len(ms) == 2:
        f, t = float(np.median(ms['fused'])), float(np.median(ms['torch']))
        print('fused / torch = %.4f (%.4f ms/step %s)' % (f / t, abs(t - f), 'saved' if f <= t else 'lost'))


if __name__ == '__main__':
    main()
