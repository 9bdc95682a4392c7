"""ELBO-step throughput of the MI355X CBF-SSM hot path (BASELINE.json metric) -- prints ONE JSON line on rank 0.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload C3] [--mode eval|train] [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps, writes the last step's outputs (--dump-outputs) and prints the line.
Everything else the line can carry is measured only with --full: the per-kernel roofline, the CPU baseline and, at N>1,
the single-rank baseline, the C4 config and the collective (below).

A "step" is one pass of the hot path over one synthetic mini-batch already resident in HBM: noise draw, positivity
transforms, K_mm/Cholesky/K^-1 + operand packing for both GPs, both backward (recognition) runs, the forward
(filter) pass, log-likelihood + moments, ELBO combination (mode=eval: what Trainer's test pass runs,
reference training/trainer.py:46) and, for mode=train, the adjoint pass + Adam update (trainer.py:40).

N>1: one process per GPU (torch.distributed, backend nccl = RCCL), every rank holds the same per-GPU workload
(weak scaling: the global batch is N x B sequences) and the ranks exchange ONE all-reduce per step.  The default
workload is C3 (Sarcos M=100, the config the metric is quoted on) AT EVERY N, so that a 1 -> 2 -> 4 -> 8 series of
`value` is one workload; --workload overrides.  A line printed at N>1 carries its own baseline: `single_rank` = the
same steps on the same ranks in the same run with the collective off, `scaling_efficiency` = value / (N x that), and
`eight_gpu_config` = the same pair of measurements for C4 (Sarcos M=200, 256 sequences per GPU = BASELINE.json's
8-GPU config).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, 'cbf-ssm_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np   # noqa: E402
import torch         # noqa: E402

F64_MFMA_PEAK_TFLOPS = 78.6   # MI355X FP64 matrix (spec); csrc/probe/mfma_f64_probe measures 77.7 on the box
F32_MFMA_PEAK_TFLOPS = 157.3  # MI355X FP32 matrix, v_mfma_f32_16x16x4_f32 at 32 cycles per SIMD (MI355X_MICROARCH.md: 155 measured;
                              # csrc/probe/mfma_f64_probe prints the rate it measures on the box)
HBM_PEAK_GBS = 8000.0
DUMP_BYTES = 60 * 10 ** 6     # --dump-outputs writes at most this much in all


def dump_outputs(outdir, arrays):
    """--dump-outputs: what the timed path computed in its last step, one float64 `<outdir>/<name>.npy` per array.  An array
    larger than its share of DUMP_BYTES is written as an evenly strided sample of its elements (flattened; the same elements
    in every run)."""
    os.makedirs(outdir, exist_ok=True)
    share = DUMP_BYTES // max(1, len(arrays)) // 8
    for name, t in arrays.items():
        a = t.detach().to('cpu', torch.float64).numpy()
        if a.size > share:
            a = a.reshape(-1)[::-(-a.size // share)]
        np.save(os.path.join(outdir, name + '.npy'), a)


def _cpu_model():
    try:
        for line in open('/proc/cpuinfo'):
            if line.startswith('model name'):
                return line.split(':', 1)[1].strip()
    except OSError:
        pass
    return 'unknown'


def _usable_cores():
    """CPUs this process may actually run on: affinity mask and cgroup quota (a GPU box hands one GPU's share of the
    host's cores to the job; asking the thread pools for every core the host shows would oversubscribe it)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:
        quota, period = open('/sys/fs/cgroup/cpu.max').read().split()
        if quota != 'max':
            n = min(n, max(1, int(float(quota) / float(period))))
    except (OSError, ValueError):
        try:
            quota = int(open('/sys/fs/cgroup/cpu/cpu.cfs_quota_us').read())
            period = int(open('/sys/fs/cgroup/cpu/cpu.cfs_period_us').read())
            if quota > 0:
                n = min(n, max(1, quota // period))
        except (OSError, ValueError):
            pass
    return n


def cpu_baseline(w, mode='eval', policy='auto'):
    """The op-for-op PyTorch-CPU float64 restatement (oracle/cbfssm_torch_ref.py) of the reference's TF-1.8 graph, timed
    on this box's host cores (BASELINE.md section 2 / SURVEY.md section 8d), every size as configured (recog_len too).
    Two thread settings: the reference's own session config (5 intra-op / 10 inter-op threads, training/trainer.py:22-26)
    and all cores the job may use.

    policy 'auto' (default): samples at T = 8 and T = 64 first (they show how the time per GP call converges); when the
    T = 64 sample predicts at most CBFSSM_CPU_FULL_LIMIT (90) seconds per full step the FULL-T step is timed and
    `extrapolated` is false -- with BASELINE.md section 2's statistic, the median of five after two warm-ups, when seven
    full steps fit CBFSSM_CPU_BUDGET (240) seconds (C3: 7 x 18 s on 16 cores + one step with the reference session
    config), the median of three otherwise (the autograd state of a full C3 train step is about 30 GB of host memory).
    Above the limit a T = 128 sample is added and the largest sample is scaled linearly in the number of GP calls.
    'sample': the T = 64 sample only, scaled.  'full': full T whatever it costs, median of five after two warm-ups.
    mode=train times loss + reverse-mode gradient (what minimize() executes)."""
    from cbfssm import synthetic as syn
    from oracle import cbfssm_torch_ref as tref
    import dataclasses
    host_cores = os.cpu_count() or 1
    usable = _usable_cores()
    # "all cores" = what the job can use, at most CBFSSM_BENCH_THREADS (16 = one GPU's CPU share on the MI355X boxes)
    ncores = max(1, min(usable, int(os.environ.get('CBFSSM_BENCH_THREADS', '16'))))
    try:
        torch.set_num_interop_threads(10)                    # trainer.py:25 (can only be set once per process)
    except RuntimeError:
        pass

    def timed(T_s, threads, reps):
        torch.set_num_threads(threads)
        ws = dataclasses.replace(w, T=T_s)
        cfg = ws.model_config()
        p = {k: torch.tensor(v) for k, v in syn.make_params(ws).items()}
        u, y = (torch.tensor(a) for a in syn.make_inputs(ws))
        noise = {k: torch.tensor(v) for k, v in syn.make_noise(ws).items()}
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            if mode == 'train':
                pg = {k: v.clone().requires_grad_(True) for k, v in p.items()}
                tref.elbo_step(cfg, pg, u, y, noise, True)['loss'].backward()
            else:
                with torch.no_grad():
                    tref.elbo_step(cfg, p, u, y, noise, True)
            ts.append(time.perf_counter() - t0)
        return ts

    calls = lambda T: 3 * T - 1
    per_call = {}                                            # seconds per GP call on all cores, by sample length
    T_0 = min(w.T, 8)
    per_call[T_0] = float(np.median(timed(T_0, ncores, 3)[1:])) / calls(T_0)
    T_1 = min(w.T, 64)
    t64_all = float(min(timed(T_1, ncores, 2)))              # (the first run of a size pays the allocator's first touch)
    per_call[T_1] = t64_all / calls(T_1)
    predicted = per_call[T_1] * calls(w.T)
    limit = float(os.environ.get('CBFSSM_CPU_FULL_LIMIT', '90'))
    if policy == 'full' or (policy == 'auto' and predicted <= limit):
        T_s = w.T
        budget = float(os.environ.get('CBFSSM_CPU_BUDGET', '240'))
        if policy == 'full' or 7.0 * predicted <= budget:
            reps_all, stat = 7, 'median of 5 after 2 warm-ups'
            ts = timed(T_s, ncores, reps_all)[2:]
        else:
            reps_all, stat = 3, 'median of 3 (the T = 8 and T = 64 samples ran before as warm-ups)'
            ts = timed(T_s, ncores, reps_all)
        t_all = float(np.median(ts))
        t_ref = float(min(timed(T_s, 5, 3 if policy == 'full' else 1)))
    elif policy == 'sample' or T_1 == w.T:
        T_s, stat = T_1, 'faster of 2'
        t_all = t64_all
        t_ref = float(min(timed(T_s, 5, 2)))
    else:
        T_s, stat = min(w.T, 128), 'faster of 2'
        t_all = float(min(timed(T_s, ncores, 2)))
        t_ref = float(min(timed(T_s, 5, 1)))
    per_call[T_s] = t_all / calls(T_s)
    scale = calls(w.T) / calls(T_s)
    best = min(t_all, t_ref) * scale
    conv = {('T%d' % k): v for k, v in sorted(per_call.items())}
    # `cores`: the threads the quoted value actually ran on (the faster of the two settings); the host's count beside it
    used = ncores if t_all <= t_ref else 5
    return {'value': 1.0 / best, 'unit': 'steps/s', 'cores': used, 'host_cores': host_cores, 'cores_usable': usable, 'cpu_model': _cpu_model(),
            'kind': 'port',
            'threads': {'all_cores': {'intra_op': ncores, 'seconds_per_step': t_all * scale},
                        'reference_session_config': {'intra_op': 5, 'inter_op': 10, 'seconds_per_step': t_ref * scale}},
            'sample_T': T_s, 'sample_gp_calls': calls(T_s), 'full_gp_calls': calls(w.T), 'extrapolated': T_s != w.T,
            'seconds_per_gp_call_all_cores': conv, 'statistic': stat,
            'sample': '%s step of %s, every size as configured (M=%d B=%d S=%d recog_len=%d), T = %d of %d (%d of %d GP '
                      'calls): %.2f s on %d threads (the job\'s share of the host\'s cores; %s), %.2f s with the reference '
                      'session config (5 intra-op / 10 inter-op threads)%s; seconds per GP call on all cores at T = %s: %s; '
                      'PyTorch-CPU float64 restatement of the TF-1.8 op sequence%s; value = the faster of the two settings'
                      % (mode, w.name, w.M, w.B, w.S, w.recog_len, T_s, w.T, calls(T_s), calls(w.T), t_all, ncores, stat, t_ref,
                         '' if T_s == w.T else ', scaled linearly to T=%d' % w.T,
                         ' / '.join(str(k) for k in sorted(per_call)), ' / '.join('%.4f' % per_call[k] for k in sorted(per_call)),
                         ' + reverse-mode autodiff' if mode == 'train' else '')}


def bench_variant(args, dev):
    """ELBO-step throughput of the forward-only variants: CBFSSMHALF
    (cbfssm/model/cbfssmhalf.py:117-196) and the PR-SSM baseline (cbfssm/model/prssm.py:96,117-118) on a BASELINE workload
    shape.  A step = recognition model, K_mm / Cholesky / K^-1 + packing, the forward pass, log-likelihood + moments, and for
    mode=train the adjoint pass, the K_mm adjoint + prior KL and the TF-1.8 Adam update."""
    from cbfssm import synthetic as syn
    from cbfssm.hip.train_half import HipHalfGrad, HipHalfTrainStep
    from cbfssm.hip.train import TFAdam
    from cbfssm.hip import ops
    w = syn.WORKLOADS[args.workload or 'C3']
    mode = 'train' if args.mode == 'auto' else args.mode
    cfg, p_np = syn.make_variant_params(w, args.model, 'rnn')
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    u = torch.randn(w.B, w.T, w.dim_u, dtype=torch.float64, device=dev, generator=g)
    y = torch.randn(w.B, w.T, w.dim_y, dtype=torch.float64, device=dev, generator=g)
    f32 = args.dtype == 'float32'
    eng = HipHalfGrad(cfg, dev, variant=args.model, dtype=args.dtype)
    opt = TFAdam({k: torch.tensor(v, device=dev) for k, v in p_np.items()}, cfg['learning_rate'])
    params = opt.views
    noise_pipe = ops.NoisePipeline(dev, g, with_backward=False)
    stepper = HipHalfTrainStep(eng, opt)                  # one HIP-graph replay per train step (CBFSSM_HIP_GRAPH=0: eager)

    last_terms = {}

    def step():
        noise = noise_pipe.next(w.T, w.N)
        if mode == 'train':
            return stepper.step(u, y, noise, True)
        loss_t, terms, _ = eng.forward(params, u, y, noise, True)
        last_terms.update(terms)
        return loss_t

    for _ in range(args.warmup):
        out = step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    loss = float(out)
    assert np.isfinite(loss), 'non-finite loss'
    if args.dump_outputs:
        arrays = {'loss': out}
        if mode == 'train':
            arrays.update(('elbo_' + k, v) for k, v in stepper.last_terms.items())
            arrays.update(('param_' + k.replace('.', '_'), v) for k, v in stepper.opt.views.items())
        else:
            arrays.update(('elbo_' + k, v) for k, v in last_terms.items())
            arrays.update(pred_mean=eng.last_ws.pred_mean, pred_var=eng.last_ws.pred_var)
        dump_outputs(args.dump_outputs, arrays)

    roof = None
    if args.full:
        # ---- the time-loop kernels by themselves: every launch of a step bracketed by HIP events (eng._prof)
        ms, n = {}, {}
        stepper.use_graph = False                             # (eager launches, each bracketed by events)
        for _ in range(3):
            eng._prof = []
            step()
            torch.cuda.synchronize()
            ms, n = {}, {}
            for kind, e0, e1 in eng._prof:
                ms[kind] = ms.get(kind, 0.0) + e0.elapsed_time(e1)
                n[kind] = n.get(kind, 0) + 1
        eng._prof = None

        def F(M, D, Do):   # algorithmic FLOPs of one GP point evaluation
            return 2 * M * M + M * (2 * D + 5 * Do + 5)
        pts = 1.0 * (w.T - 1) * w.N
        fl = {'forward_pass': pts * F(w.M, w.D, w.dim_x)}
        if mode == 'train':
            stash = eng.stash and not f32                                  # (the float32 adjoint is one launch at every height)
            fa = 2.0 if eng.last_ws.a2s_f is not None else 3.0            # saved A2 tiles: the reverse sweep costs 2 F
            outer = 2.0 * w.M * w.M if stash else 0.0                      # stash mode: A2bar K^T runs in the contraction
            fl['forward_pass_adjoint'] = pts * (fa * F(w.M, w.D, w.dim_x) - outer)
            if stash:
                fl['stash_contraction'] = pts * outer
        name = max(ms, key=lambda k: ms[k])
        ach = fl[name] / (ms[name] * 1e-3) / 1e12
        peak = F32_MFMA_PEAK_TFLOPS if f32 else F64_MFMA_PEAK_TFLOPS
        roof = {'bound': 'mfma', 'achieved': ach, 'peak': peak, 'unit': 'TFLOP/s',
                'frac': ach / peak, 'traffic': None, 'kernel': name,
                'kernel_ms': ms, 'kernel_tflops': {k: fl[k] / (ms[k] * 1e-3) / 1e12 for k in ms}, 'launches': n,
                'note': 'one GP (gp_f), no backward runs: one workgroup per 16-chain group walks the T - 1 steps (%d groups on '
                        'the chip\'s CUs); full launches, HIP events on the launch stream' % ((w.N + 15) // 16)}
    steps_per_s = args.steps / dt
    rec = {
        'metric': 'ELBO steps/sec', 'value': steps_per_s, 'unit': 'steps/s (one step = one %d-sequence mini-batch per GPU)' % w.B,
        'n_gpus': 1, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': dt / args.steps * 1e3,
        'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32' if f32 else 'f64', 'data': 'synthetic',
        'states_per_sec': steps_per_s * w.B * w.T,
        'config': {'workload': '%s shape, %s %s step: M=%d T=%d B=%d/GPU S=%d dim_x=%d dim_u=%d dim_y=%d recog_len=%d, GRU(16) '
                               'recognition model' % (w.name, {'half': 'CBFSSMHALF', 'prssm': 'PRSSM'}[args.model], mode, w.M, w.T,
                                                      w.B, w.S, w.dim_x, w.dim_u, w.dim_y, w.recog_len),
                   'model': args.model, 'mode': mode, 'global_batch': w.B, 'seq_len': w.T, 'particles': w.S, 'parallelism': 'dp1'},
        'loss': loss,
        'roofline': roof,
        'cpu_baseline': None,
    }
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--workload', default=None,
                    help='C1..C5 (default: C3 -- the config the metric is quoted on -- at every N; at N > 1 the line also '
                         'carries C4, the 8-GPU config of BASELINE.json, 256 sequences per GPU, as `eight_gpu_config`)')
    ap.add_argument('--mode', default='auto', choices=['auto', 'eval', 'train'])
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--cpu-baseline', default='auto', choices=['auto', 'sample', 'full'])
    ap.add_argument('--params', default='init', choices=['init', 'trained'],
                    help='init: run-script initial values (cond(K_mm) 1..700, dense GP form).  trained: the trained-like '
                         'family of the parity sweep (cbfssm.synthetic.trained_like_params, lengthscales x 64, inducing means '
                         '0.1: cond 3e7, above the automatic switch to the two-triangular GP form)')
    ap.add_argument('--model', default='cbfssm', choices=['cbfssm', 'half', 'prssm'],
                    help='cbfssm: the headline path.  half / prssm: the forward-only variants (CBFSSMHALF, cbfssmhalf.py; the PR-SSM '
                         'baseline, prssm.py) on the same workload shapes: one GP, no backward runs, GRU(16) recognition model')
    ap.add_argument('--dtype', default='float64', choices=['float64', 'float32'],
                    help='float32: the float32-arithmetic passes and adjoint (NOT the headline: the reference computes in '
                         'float64)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write what the last one computed as DIR/<name>.npy (float64)')
    ap.add_argument('--full', action='store_true',
                    help='also measure what the headline figure does not need: the per-kernel roofline, the CPU baseline '
                         '(unless --no-cpu-baseline) and, at N > 1, the single-rank baseline, the C4 config and the collective')
    args = ap.parse_args()

    from cbfssm import synthetic as syn
    from cbfssm.hip import ops, lib
    lib.load()   # fail loudly if the HIP extension is missing

    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        # rehearsal on a one-GPU box: CBFSSM_BENCH_ONE_DEVICE=1 puts every rank on cuda:0 with the gloo backend (the
        # collective then goes through the host, cbfssm/hip/dist_utils.py); the real run is one rank per GPU over RCCL
        if os.environ.get('CBFSSM_BENCH_ONE_DEVICE'):
            local_rank = 0
            dist.init_process_group('gloo')
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group('nccl', device_id=torch.device('cuda', local_rank))
    assert world == args.gpus, 'launch with torch.distributed.run --nproc-per-node %d' % args.gpus
    dev = torch.device('cuda', local_rank)
    torch.cuda.set_device(dev)

    if args.model != 'cbfssm':
        assert world == 1, '--model half|prssm: one GPU'
        return bench_variant(args, dev)
    default_workload = args.workload is None
    if default_workload:
        args.workload = 'C3'          # the same workload at every N: a 1 -> N series of `value` is one workload
    w = syn.WORKLOADS[args.workload]
    cfg = w.model_config()
    mode = args.mode
    try:
        from cbfssm.hip.train import HipTrainStep
        have_train = True
    except ImportError:
        have_train = False
    if mode == 'auto':
        mode = 'train' if have_train else 'eval'
    if args.dtype == 'float32':
        assert world == 1, 'float32 arithmetic: measured on one GPU'

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def build(w, cfg):
        """synthetic inputs of workload `w`, resident in HBM before the timed region, and its step: `step()` as the job
        runs it (N > 1: with the step's one all-reduce), `step_local()` the same launches on this rank alone"""
        g = torch.Generator(device=dev)
        g.manual_seed(1234 + rank)
        u = torch.randn(w.B, w.T, w.dim_u, dtype=torch.float64, device=dev, generator=g)
        y = torch.randn(w.B, w.T, w.dim_y, dtype=torch.float64, device=dev, generator=g)
        if args.params == 'trained':
            p_np = syn.trained_like_params(w, ls_mult=64.0, zeta_mean=0.1)
        else:
            p_np = syn.make_params(w, seed=1)
        params = {k: torch.tensor(v, device=dev) for k, v in p_np.items()}
        # fresh noise every step (the reference draws it inside the graph); the draw for step k+1 runs on a side stream
        # while step k computes
        noise_pipe = ops.NoisePipeline(dev, g)

        def draw_noise():
            return noise_pipe.next(w.T, w.N)

        b = dict(w=w, cfg=cfg, u=u, y=y, params=params, draw_noise=draw_noise, stepper=None)
        if mode == 'train':
            # N > 1: the data-parallel step can replay two HIP graphs around the eager all-reduce
            # (tests/test_distributed_gpu.py); at this workload the launches are hidden behind the kernels anyway, so the
            # bench keeps plain launches there unless asked (CBFSSM_DP_GRAPH=1)
            use_graph = None if world == 1 else (os.environ.get('CBFSSM_DP_GRAPH') == '1')
            stepper = HipTrainStep(cfg, params, dev, dist if world > 1 else None, graph=use_graph, dtype=args.dtype)
            b['stepper'] = stepper
            b['step'] = lambda: stepper.step(u, y, draw_noise(), condition=True)
            b['step_local'] = lambda: stepper.step(u, y, draw_noise(), condition=True, local=True)

            def outputs(loss):
                # the step's loss and ELBO terms, and the parameters after its Adam update
                d = {'loss': loss}
                d.update(('elbo_' + k, v) for k, v in stepper.last_terms.items())
                d.update(('param_' + k.replace('.', '_'), v) for k, v in stepper.params.items())
                return d
            b['outputs'] = outputs
        else:
            from cbfssm.hip.train import HipElboGrad
            eng = HipElboGrad(cfg, dev, dist if world > 1 else None, require_adjoint=False, dtype=args.dtype)
            out8 = torch.zeros(8, dtype=torch.float64, device=dev)

            def step(local=False):
                # what Trainer's test pass fetches (loss only); N>1: the three data terms are all-reduced inside
                loss_t, _, ws = eng.forward(params, u, y, draw_noise(), condition=True, local=local)
                out8.copy_(ws.out)
                out8[6] = loss_t
                return out8
            b['step'] = step
            b['step_local'] = lambda: step(local=True)
            # out[0..7] of cbfssm_elbo_combine_f64 (loss = out[6]) and the predictive moments of the same evaluation
            b['outputs'] = lambda out: {'elbo_out': out, 'pred_mean': eng.last_ws.pred_mean, 'pred_var': eng.last_ws.pred_var}
        return b

    def timed(stepfn, steps, warmup):
        """`warmup` untimed steps, then EXACTLY `steps` steps between barrier + synchronize on both sides; max over ranks.
        Returns (seconds, loss, what the last step returned)."""
        out = None
        for _ in range(warmup):
            out = stepfn()
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = stepfn()
        sync()
        dt = time.perf_counter() - t0
        if world > 1:
            tmax = torch.tensor([dt], dtype=torch.float64, device=dev if dist.get_backend() == 'nccl' else 'cpu')
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            dt = float(tmax.item())
        loss = float(out[6]) if mode == 'eval' else float(out)
        assert np.isfinite(loss), 'non-finite loss'
        return dt, loss, out

    def with_baseline(b, steps, warmup):
        """N > 1: the single-rank baseline of the SAME workload in the SAME run -- the same launches on every rank with the
        collective off (each rank evaluates its own mini-batch as a single device would; max over ranks like `value`)"""
        dt1, _, _ = timed(b['step_local'], steps, max(1, min(warmup, 2)))
        return {'ms_per_step': dt1 / steps * 1e3, 'steps_per_s': steps / dt1, 'steps': steps,
                'how': 'the same step on every rank with the all-reduce off, same process, right after the timed region'}

    bld = build(w, cfg)
    u, y, params, draw_noise, stepper = bld['u'], bld['y'], bld['params'], bld['draw_noise'], bld['stepper']
    N = w.N
    dt, loss, out = timed(bld['step'], args.steps, args.warmup)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, bld['outputs'](out))
    single = eff = c4 = None
    if world > 1 and args.full:
        single = with_baseline(bld, args.steps, args.warmup)
        eff = (args.steps / dt) / single['steps_per_s']
        if default_workload and mode == 'train' and not os.environ.get('CBFSSM_BENCH_NO_C4'):
            # BASELINE.json's 8-GPU config (Sarcos M = 200, 256 sequences per GPU) beside the headline workload, with its
            # own single-rank baseline: one SCALE record holds both
            w4 = syn.WORKLOADS['C4']
            k4 = max(3, min(args.steps, 10))
            b4 = build(w4, w4.model_config())
            dt4, loss4, _ = timed(b4['step'], k4, 2)
            s4 = with_baseline(b4, k4, 2)
            c4 = {'workload': '%s %s step: M=%d T=%d B=%d/GPU S=%d' % (w4.name, mode, w4.M, w4.T, w4.B, w4.S),
                  'value': k4 / dt4 * world, 'unit': 'steps/s', 'steps': k4, 'ms_per_step': dt4 / k4 * 1e3,
                  'global_batch': w4.B * world, 'loss': loss4, 'single_rank': s4,
                  'scaling_efficiency': (k4 / dt4) / s4['steps_per_s'],
                  'collective_bytes': int(b4['stepper'].engine.red.numel()) * 8}
            del b4
            torch.cuda.empty_cache()

    # ---- the step's ONE collective, timed by itself on every rank (all ranks take part; rank 0 reports): HIP events on
    # the launch stream for RCCL, wall clock around a synchronised call for the gloo rehearsal
    coll = None
    if world > 1 and args.full:
        from cbfssm.hip.dist_utils import all_reduce_sum
        nel = int(stepper.engine.red.numel()) if mode == 'train' else 3
        buf = torch.ones(nel, dtype=torch.float64, device=dev)
        reps = 20
        for _ in range(3):
            all_reduce_sum(buf, dist)
            buf.fill_(1.0)
        sync()
        if dist.get_backend() == 'nccl':
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                all_reduce_sum(buf, dist)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1) / reps
        else:
            t0c = time.perf_counter()
            for _ in range(reps):
                all_reduce_sum(buf, dist)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0c) * 1e3 / reps
        # 1.0 summed over `world` ranks, `reps` + 0 times since the last fill: world ** reps (exact in float64 up to 2^53)
        expect = float(world) ** reps
        ok = bool(abs(float(buf[0]) / expect - 1.0) < 1e-12) if expect < 2.0 ** 53 else None
        coll = {'op': 'all_reduce(sum)', 'backend': dist.get_backend() + (' (RCCL)' if dist.get_backend() == 'nccl' else ''),
                'ranks': dist.get_world_size(), 'bytes': nel * 8, 'ms': ms, 'per_step': 1, 'sum_checked': ok,
                'timing': 'HIP events, %d back-to-back calls' % reps if dist.get_backend() == 'nccl' else 'wall clock'}
        sync()

    # ---- per-kernel timing of the time-loop kernels with HIP events on the launch stream
    roof = None
    if rank == 0 and args.full and args.dtype == 'float32':
        # the float32-arithmetic time loops (cbfssm_*_pass_f32, cbfssm_*_pass_bwd_f32), each timed by itself with HIP events on
        # the launch stream and priced against the float32 matrix peak (v_mfma_f32_16x16x4_f32)
        import ctypes as C
        l = lib.load()
        st = ops._stream()
        noise = draw_noise()
        prob = lib.make_problem(w.B, w.S, w.T, w.dim_x, w.dim_u, w.dim_y, w.M, cfg['recog_len'], cfg['k_factor'], True)
        if mode == 'train':
            eng2 = stepper.engine
            eng2.loss_and_grads(stepper.params, u, y, noise)          # fills the trajectories, (fmean, fvar) and the packs
            ws = eng2.last_ws
            cst = eng2._constrained({k: v for k, v in stepper.params.items()})
            var_x, var_y, pack_f, pack_b = cst['var_x'], cst['var_y'], eng2.pack_f, eng2.pack_b
        else:
            eng2 = ops.HipElbo(cfg, dev, dtype='float32')
            eng2.prepare(params)
            ws = eng2.run(u, y, noise, condition=True, keep_h=True)
            var_x, var_y, pack_f, pack_b = eng2.var_x, eng2.var_y, eng2.pack_f, eng2.pack_b
        b32f, b32b = (C.c_void_p(pk.pack_f32().data_ptr()) for pk in (pack_f, pack_b))
        lf_, lb_ = C.byref(pack_f.layout), C.byref(pack_b.layout)
        P = ops._ptr

        def time32(fn, reps):
            fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3 / reps

        def F(M, D, Do):   # algorithmic FLOPs of one GP point evaluation
            return 2 * M * M + M * (2 * D + 5 * Do + 5)
        pts_f, pts_b = 1.0 * (w.T - 1) * N, 2.0 * w.T * N
        reps = 10 if w.M <= 200 else 2
        kern = {
            'backward_pass_f32': (time32(lambda: lib.check(l.cbfssm_backward_pass_f32(
                C.byref(prob), lb_, b32b, P(var_x), P(u), P(y), P(noise['hid_b']), P(noise['eps_b']), P(ws.y2), P(ws.h_all),
                P(ws.fmv_b), P(ws.a2s_b), P(ws.ent_part), st), 'bwd32'), reps), pts_b * F(w.M, w.D, w.dim_out_b)),
            'forward_pass_f32': (time32(lambda: lib.check(l.cbfssm_forward_pass_f32(
                C.byref(prob), lf_, b32f, P(var_x), P(var_y), P(u), P(y), P(ws.y2), P(noise['eps_f']), P(ws.x), P(ws.fmv_f),
                P(ws.a2s_f), P(ws.kl_part), st), 'fwd32'), reps), pts_f * F(w.M, w.D, w.dim_x))}
        if mode == 'train':
            cL, cE = float(cfg['loss_factors'][0]) / w.S, float(cfg['loss_factors'][1]) / w.S
            # with the tiles the passes kept the reverse sweep costs 2 F per GP evaluation (K^-1 A2bar and the accumulation),
            # 3 F when it recomputes the kernel tile and A2
            fa32 = 2.0 if ws.a2s_b is not None else 3.0
            kern['forward_pass_adjoint_f32'] = (time32(lambda: lib.check(l.cbfssm_forward_pass_bwd_f32(
                C.byref(prob), lf_, b32f, P(var_x), P(var_y), P(u), P(y), P(ws.y2), P(noise['eps_f']), P(ws.x), P(ws.fmv_f),
                P(ws.a2s_f), cL, P(ws.gy2), P(ws.gpart_f), st), 'rev fwd32'), max(1, reps // 2)), fa32 * pts_f * F(w.M, w.D, w.dim_x))
            kern['backward_pass_adjoint_f32'] = (time32(lambda: lib.check(l.cbfssm_backward_pass_bwd_f32(
                C.byref(prob), lb_, b32b, P(var_x), P(u), P(y), P(noise['hid_b']), P(noise['eps_b']), P(ws.h_all), P(ws.fmv_b),
                P(ws.a2s_b), P(ws.gy2), cE, P(ws.gpart_b), st), 'rev bwd32'), max(1, reps // 2)), fa32 * pts_b * F(w.M, w.D, w.dim_out_b))
        name = max(kern, key=lambda k: kern[k][0])
        ach = kern[name][1] / kern[name][0] / 1e12
        roof = {'bound': 'mfma', 'achieved': ach, 'peak': F32_MFMA_PEAK_TFLOPS, 'unit': 'TFLOP/s',
                'frac': ach / F32_MFMA_PEAK_TFLOPS, 'traffic': None, 'kernel': name,
                'kernel_ms': {k: v[0] * 1e3 for k, v in kern.items()},
                'kernel_tflops': {k: v[1] / v[0] / 1e12 for k, v in kern.items()},
                'note': 'float32 arithmetic (v_mfma_f32_16x16x4_f32, 32 cycles per SIMD: 157.3 TFLOP/s); full launches; the adjoint is '
                        'priced at 2 F per GP evaluation when it reads the kept [A2 | kernel tile] records, 3 F when it recomputes them'}
    elif rank == 0 and args.full:
        import ctypes as C
        l = lib.load()
        st = ops._stream()
        noise = draw_noise()
        prob = lib.make_problem(w.B, w.S, w.T, w.dim_x, w.dim_u, w.dim_y, w.M, cfg['recog_len'], cfg['k_factor'], True)

        def time_kernel(fn, reps=10):
            fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3 / reps

        stash = (mode == 'train') and stepper.engine.stash
        stash_ms = None
        if mode == 'train':
            eng2 = stepper.engine
            group, eng2.dist = eng2.dist, None     # rank-local from here on: the other ranks do not take part
            try:
                eng2.loss_and_grads(stepper.params, u, y, noise)      # fills the saved trajectories
                if stash:
                    # stash mode (M > 112): the adjoint is a schedule of time-chunked launches + contractions
                    # (hip/train.py:_adjoint_stash).  Run it with every launch bracketed by HIP events on ONE stream and
                    # sum per kind: each kernel's own time, nothing overlapping it
                    for _ in range(3):
                        eng2._prof = []
                        eng2.loss_and_grads(stepper.params, u, y, noise)
                        torch.cuda.synchronize()
                        stash_ms, stash_n = {}, {}
                        for kind, e0, e1 in eng2._prof:
                            stash_ms[kind] = stash_ms.get(kind, 0.0) + e0.elapsed_time(e1)
                            stash_n[kind] = stash_n.get(kind, 0) + 1
            finally:
                eng2.dist = group
                eng2._prof = None
            ws = eng2.last_ws
            cst = eng2._constrained({k: v for k, v in stepper.params.items()})
            var_x, var_y = cst['var_x'], cst['var_y']
            pack_f, pack_b = eng2.pack_f, eng2.pack_b
        else:
            eng2 = ops.HipElbo(cfg, dev)
            eng2.prepare(params if mode == 'eval' else stepper.params)
            ws = ops.ElboWorkspace(prob, dev, keep_h=False)
            var_x, var_y, pack_f, pack_b = eng2.var_x, eng2.var_y, eng2.pack_f, eng2.pack_b

        def k_bwd():
            lib.check(l.cbfssm_backward_pass_f64(C.byref(prob), C.byref(pack_b.layout), ops._ptr(pack_b.buf),
                                                 ops._ptr(var_x), ops._ptr(u), ops._ptr(y), ops._ptr(noise['hid_b']),
                                                 ops._ptr(noise['eps_b']), ops._ptr(ws.y2), ops._ptr(ws.h_all),
                                                 ops._ptr(ws.fmv_b), ops._ptr(ws.a2s_b), ops._ptr(ws.ent_part), st),
                      'bwd')

        def k_fwd():
            lib.check(l.cbfssm_forward_pass_f64(C.byref(prob), C.byref(pack_f.layout), ops._ptr(pack_f.buf),
                                                ops._ptr(var_x), ops._ptr(var_y), ops._ptr(u), ops._ptr(y),
                                                ops._ptr(ws.y2), ops._ptr(noise['eps_f']), ops._ptr(ws.x),
                                                ops._ptr(ws.fmv_f), ops._ptr(ws.a2s_f), ops._ptr(ws.kl_part), st), 'fwd')

        def F(M, D, Do):   # algorithmic FLOPs of one GP point evaluation
            return 2 * M * M + M * (2 * D + 5 * Do + 5)
        kern = {}
        k_bwd(); k_fwd()
        kern['backward_pass'] = (time_kernel(k_bwd), 2.0 * w.T * N * F(w.M, w.D, w.dim_out_b))
        kern['forward_pass'] = (time_kernel(k_fwd), 1.0 * (w.T - 1) * N * F(w.M, w.D, w.dim_x))
        # adjoint of one GP evaluation: the reverse sweep costs 2F (K^-1 A2bar and the A2bar K^T outer product);
        # without the saved A2 tiles the kernel also recomputes the evaluation itself (+F)  
        fa = 2.0 if (mode == 'train' and ws.a2s_b is not None) else 3.0
        pts_f, pts_b = 1.0 * (w.T - 1) * N, 2.0 * w.T * N          # GP point evaluations per launch
        launches = None
        if stash:
            # the outer product A2bar K^T (2 M^2 flops per GP point) is not in the adjoint kernels here: they write its
            # operand images and cbfssm_stash_contract_f64 does it -- priced where it runs
            outer = 2.0 * w.M * w.M
            kern['forward_pass_adjoint'] = (stash_ms['forward_pass_adjoint'] * 1e-3, pts_f * (fa * F(w.M, w.D, w.dim_x) - outer))
            kern['backward_pass_adjoint'] = (stash_ms['backward_pass_adjoint'] * 1e-3, pts_b * (fa * F(w.M, w.D, w.dim_out_b) - outer))
            kern['stash_contraction'] = (stash_ms['stash_contraction'] * 1e-3, (pts_f + pts_b) * outer)
            launches = dict(stash_n)
        if mode == 'train' and not stash:
            cL, cE = float(cfg['loss_factors'][0]) / w.S, float(cfg['loss_factors'][1]) / w.S

            def k_rfwd():
                lib.check(l.cbfssm_forward_pass_bwd_f64(C.byref(prob), C.byref(pack_f.layout), ops._ptr(pack_f.buf),
                                                        ops._ptr(var_x), ops._ptr(var_y), ops._ptr(u), ops._ptr(y),
                                                        ops._ptr(ws.y2), ops._ptr(noise['eps_f']), ops._ptr(ws.x),
                                                        ops._ptr(ws.fmv_f), ops._ptr(ws.a2s_f), cL, ops._ptr(ws.gy2), ops._ptr(ws.gpart_f), st), 'rev fwd')

            def k_rbwd():
                lib.check(l.cbfssm_backward_pass_bwd_f64(C.byref(prob), C.byref(pack_b.layout), ops._ptr(pack_b.buf),
                                                         ops._ptr(var_x), ops._ptr(u), ops._ptr(y),
                                                         ops._ptr(noise['hid_b']), ops._ptr(noise['eps_b']),
                                                         ops._ptr(ws.h_all), ops._ptr(ws.fmv_b), ops._ptr(ws.a2s_b),
                                                         ops._ptr(ws.gy2), cE,
                                                         ops._ptr(ws.gpart_b), st), 'rev bwd')
            kern['forward_pass_adjoint'] = (time_kernel(k_rfwd, 5), fa * pts_f * F(w.M, w.D, w.dim_x))
            kern['backward_pass_adjoint'] = (time_kernel(k_rbwd, 5), fa * pts_b * F(w.M, w.D, w.dim_out_b))
        # The forward-direction kernels run one workgroup per 16-chain group: 320 groups on 256 CUs make the full launch
        # two rounds at 62.5 % occupancy.  The step does not run them that way (hip/train.py:_split: a main piece of whole
        # rounds, the remainder overlapped with the many-workgroup backward-run kernels on a second stream), so the
        # main-piece launch is timed too: what these kernels achieve as scheduled.
        main_piece = None
        if mode == 'train' and not stash:
            split = stepper.engine._split(prob)
            if split is not None:
                groups = (N + 15) // 16
                p_main = stepper.engine._sub_problem(prob, 0, split[0])
                full = prob
                prob = p_main
                try:
                    t_f, t_rf = time_kernel(k_fwd), time_kernel(k_rfwd, 5)
                finally:
                    prob = full
                share = split[0] / groups
                main_piece = {'groups': [split[0], groups],
                              'kernel_ms': {'forward_pass': t_f * 1e3, 'forward_pass_adjoint': t_rf * 1e3},
                              'kernel_tflops': {'forward_pass': kern['forward_pass'][1] * share / t_f / 1e12,
                                                'forward_pass_adjoint': kern['forward_pass_adjoint'][1] * share / t_rf / 1e12}}
        # the HBM-bound kernel of the path: log-likelihood + predictive moments, one pass
        # over the filtered trajectories.  Algorithmic bytes: x and y read once, the four (B,T,.) outputs written once.
        # Timed on a ROTATION of trajectory buffers larger than the 256 MB Infinity Cache (a back-to-back loop over one
        # 143 MB buffer is served from that cache and reads as 5 TB/s; in the step the kernel follows 7 GB of tile traffic
        # and sees HBM): every call reads a buffer that has been evicted since its last use.
        x_bytes = ws.x.numel() * 8
        n_rot = max(2, int(3 * 256 * 2 ** 20 // max(x_bytes, 1)) + 1) if x_bytes < 3 * 256 * 2 ** 20 else 1
        n_rot = min(n_rot, 64)
        x_rot = [ws.x] + [ws.x.clone() for _ in range(n_rot - 1)]
        ll_calls = [0]

        def k_ll():
            xb = x_rot[ll_calls[0] % n_rot]
            ll_calls[0] += 1
            lib.check(l.cbfssm_loglik_moments_f64(C.byref(prob), ops._ptr(var_y), ops._ptr(y), ops._ptr(xb),
                                                  ops._ptr(ws.ll_part), ops._ptr(ws.pred_mean), ops._ptr(ws.pred_var),
                                                  ops._ptr(ws.int_mean), ops._ptr(ws.int_var), st), 'loglik')
        t_ll = time_kernel(k_ll, max(20, 2 * n_rot))
        del x_rot
        ll_bytes = 8.0 * (w.T * N * w.dim_x + w.B * w.T * (3 * w.dim_y + 2 * w.dim_x) + ws.ll_part.numel())
        name = max(kern, key=lambda k: kern[k][0])
        tk, fl = kern[name]
        ach = fl / tk / 1e12
        # HBM bytes per launch of that kernel: NOT measured in this run -- rocprofv3 PMC passes of this same command
        # (profiles/tools/collect_traffic.sh) are committed per round; the newest file that has the entry is quoted and
        # named in `traffic_source`
        traffic, traffic_source = None, None
        for rnd in ('r04', 'r03', 'r02', 'r01'):
            tpath = os.path.join(ROOT, 'profiles', rnd, 'traffic.json')
            if os.path.exists(tpath):
                val = json.load(open(tpath)).get('%s:%s' % (args.workload, mode), {}).get(name)
                if val is not None:
                    traffic, traffic_source = val, 'profiles/%s/traffic.json (rocprofv3 --pmc, static)' % rnd
                    break
        roof = {'bound': 'mfma', 'achieved': ach, 'peak': F64_MFMA_PEAK_TFLOPS, 'unit': 'TFLOP/s',
                'frac': ach / F64_MFMA_PEAK_TFLOPS, 'traffic': traffic, 'traffic_source': traffic_source,
                'kernel': name,
                'kernel_ms': {k: v[0] * 1e3 for k, v in kern.items()},
                'kernel_tflops': {k: v[1] / v[0] / 1e12 for k, v in kern.items()},
                'main_piece': main_piece,
                'stash_mode': None if not stash else {
                    'launches': launches, 'bookkeeping_ms': stash_ms.get('reductions'),
                    'adjoint_with_contraction': {
                        'ms': sum(stash_ms[k] for k in ('forward_pass_adjoint', 'backward_pass_adjoint', 'stash_contraction')),
                        'tflops': fa * (pts_f * F(w.M, w.D, w.dim_x) + pts_b * F(w.M, w.D, w.dim_out_b)) / 1e9 /
                        sum(stash_ms[k] for k in ('forward_pass_adjoint', 'backward_pass_adjoint', 'stash_contraction'))},
                    'note': 'M > 112: each adjoint is a series of time-chunked launches (their times are summed); the A2bar K^T '
                            'outer product runs in cbfssm_stash_contract_f64 and is priced there (2 M^2 flops per GP point)'},
                'hbm_kernel': {'kernel': 'loglik_moments', 'bound': 'hbm', 'ms': t_ll * 1e3,
                               'achieved': ll_bytes / t_ll / 1e9, 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                               'frac': ll_bytes / t_ll / 1e9 / HBM_PEAK_GBS,
                               'timing': 'HIP events over calls that rotate through %d trajectory buffers (%.0f MB in all: '
                                         'larger than the 256 MB Infinity Cache, so every read comes from HBM)'
                                         % (n_rot, n_rot * x_bytes / 1e6)},
                'hbm_algorithmic_GBs': w.bytes_per_state() * w.B * w.T / (dt / args.steps) / 1e9,
                'hbm_frac_of_8TBs': w.bytes_per_state() * w.B * w.T / (dt / args.steps) / 1e9 / HBM_PEAK_GBS}

    if rank == 0:
        steps_per_s = args.steps / dt
        rec = {
            'metric': 'ELBO steps/sec', 'value': steps_per_s * world, 'unit': 'steps/s (one step = one %d-sequence '
                      'mini-batch per GPU)' % w.B,
            'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': dt / args.steps * 1e3,
            'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f64' if args.dtype == 'float64' else 'f32',
            'data': 'synthetic',
            'states_per_sec': steps_per_s * world * w.B * w.T,
            'config': {'workload': '%s %s step: M=%d T=%d B=%d/GPU S=%d dim_x=%d dim_u=%d dim_y=%d recog_len=%d'
                                   % (w.name, mode, w.M, w.T, w.B, w.S, w.dim_x, w.dim_u, w.dim_y, w.recog_len),
                       'mode': mode, 'global_batch': w.B * world, 'seq_len': w.T, 'particles': w.S,
                       'parallelism': 'dp%d' % world},
            'loss': loss,
            'single_rank': single,
            'scaling_efficiency': eff,
            'eight_gpu_config': c4,
            'collective': coll,
            'params': args.params,
            'roofline': roof,
        }
        if args.full and not args.no_cpu_baseline and world == 1 and args.dtype == 'float64':
            rec['cpu_baseline'] = cpu_baseline(w, mode, policy=args.cpu_baseline)
            rec['speedup_vs_cpu_baseline'] = rec['value'] / rec['cpu_baseline']['value']
        else:
            rec['cpu_baseline'] = None
        print(json.dumps(rec))
    if world > 1:
        dist.barrier()           # rank 0 times its kernels and the CPU baseline alone; leave together
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
