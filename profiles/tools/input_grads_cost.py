"""Cost of a train step that also asks for d loss / d u and d loss / d y (HipElboGrad.loss_and_grads(..., input_grads=True))
against the plain eager step of the same engine, interleaved rounds in one process:

    python profiles/tools/input_grads_cost.py C3 [rounds] [steps]

Prints one JSON line: median and min ms per step of both, and their ratio."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'cbf-ssm_amd')]

import numpy as np
import torch

from cbfssm import synthetic as syn
from cbfssm.hip import ops
from cbfssm.hip.train import HipElboGrad, TFAdam, PARAM_NAMES, _f64


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else 'C3'
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    dev = torch.device('cuda:0')
    w = syn.WORKLOADS[name]
    cfg = w.model_config()
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    u = torch.randn(w.B, w.T, w.dim_u, dtype=torch.float64, device=dev, generator=g)
    y = torch.randn(w.B, w.T, w.dim_y, dtype=torch.float64, device=dev, generator=g)
    p_np = syn.make_params(w, seed=1)
    eng = HipElboGrad(cfg, dev)
    opt = TFAdam({k: _f64(torch.tensor(p_np[k]), dev).clone() for k in PARAM_NAMES}, cfg['learning_rate'])
    pipe = ops.NoisePipeline(dev, g)

    def step(ig):
        loss, grads, _ = eng.loss_and_grads(opt.views, u, y, pipe.next(w.T, w.N), condition=True, input_grads=ig)
        opt.step(grads)
        return loss

    def timed(ig):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = step(ig)
        torch.cuda.synchronize()
        assert np.isfinite(float(loss))
        return (time.perf_counter() - t0) / steps * 1e3

    for ig in (False, True, False, True):
        step(ig)
    res = {False: [], True: []}
    for _ in range(rounds):
        for ig in (False, True):
            res[ig].append(timed(ig))
    plain, with_in = res[False], res[True]
    print(json.dumps({'workload': name, 'rounds': rounds, 'steps_per_round': steps,
                      'plain_eager_ms': {'median': float(np.median(plain)), 'min': min(plain), 'all': plain},
                      'input_grads_ms': {'median': float(np.median(with_in)), 'min': min(with_in), 'all': with_in},
                      'ratio_of_medians': float(np.median(with_in) / np.median(plain))}))


if __name__ == '__main__':
    main()
