#!/usr/bin/env python3
"""Times of one AMPC step on the GPU, one process, medians of REGIONS timed regions of REPS steps after a warm-up (device events around
the region, a synchronise at its end), the candidates alternating region by region:

  (a) the native step (SingleProcessOffPolicyOptimizer(native_ampc=True): learner_version 8 of mpg_step_begin / mpg_step_end);
  (b) the method-by-method path as a default-built stack takes it (worker.sample()'s loop of launches, replay(), compute_gradient,
      apply_gradients) - the behaviour without the keyword;
  (c) the method-by-method path with args.one_launch_sample = True (the worker's sample as one launch, everything else as (b));
  (d) one native NADP step on the same env and sizes: the neighbour, no bar attached.

Sizes: PathTracking-v0 at the reference's worker defaults (8 agents, batch_size 512: 64 iterations per sample, sampling every 10th
step), n = 25, M = 1, B = 256 and 4096; InvertedPendulumConti-v0 at built_AMPC_parser's defaults (1 agent x 512 iterations), B = 256.
The rule: (a)'s median at or below (b)'s at every size, no margin beyond the regions' own range; a size where it is not is written
down as such.  tools/bench_ampc.py stays as the record of the entry point and of the method path against NADP's.

    python tools/bench_ampc_native.py [--json out.json]          prints the markdown table of DESIGN.md 7, f8"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REGIONS, REPS, WARMUP = 7, 200, 40
PT, PD = 'PathTracking-v0', 'InvertedPendulumConti-v0'
SIZES = [(PT, 256), (PT, 4096), (PD, 256)]
NAMES = ('ampc_native', 'ampc_method', 'ampc_method_one_launch_sample', 'nadp_native')


def timed(fn, reps=REPS):
    """ms per call of one region"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def stack(alg, env, B, native, one_launch_sample=False):
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import AMPCLearner, NADPLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    more = dict(one_launch_sample=True) if one_launch_sample else {}
    args = default_args(alg, env_id=env, replay_batch_size=B, replay_starts=max(3000, B), nan_check_interval=10 ** 9, **more)
    assert (args.num_agent, args.batch_size) == ((8, 512) if env == PT else (1, 512))
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    learner = (AMPCLearner if alg == 'AMPC' else NADPLearner)(PolicyWithQs, args)
    more = dict(native_ampc=True) if (alg == 'AMPC' and native) else {}
    opt = SingleProcessOffPolicyOptimizer(worker, learner, ReplayBuffer(args, 0), None, args, sampling_interval=10, **more)
    assert (opt._fused is not None) == native
    return opt


def case(env, B):
    from mpg_amd.optimizer import quiesce_gc
    opts = [stack('AMPC', env, B, True), stack('AMPC', env, B, False), stack('AMPC', env, B, False, one_launch_sample=True),
            stack('NADP', env, B, True)]
    quiesce_gc()
    for _ in range(WARMUP):
        for o in opts:
            o.step()
    torch.cuda.synchronize()
    t = [[] for _ in opts]
    for _ in range(REGIONS):                                  # alternating: all four see the same machine
        for k, o in enumerate(opts):
            t[k].append(timed(o.step))
    torch.cuda.synchronize()
    # the three AMPC stacks did the same work from the same seed: bit-identical parameters at the end
    p = [o.worker.policy_with_value.params.view(torch.int32) for o in opts[:3]]
    assert torch.equal(p[0], p[1]) and torch.equal(p[0], p[2]), 'the AMPC candidates diverged'
    return [(statistics.median(x), min(x), max(x)) for x in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_ampc_native.py needs a GPU: nothing here is measured without one'
    fmt = lambda r: '%.4f (%.4f .. %.4f)' % r
    out = {'regions': REGIONS, 'reps': REPS, 'warmup': WARMUP, 'step': []}
    print('| env | agents x iterations | B | (a) AMPC native, ms | (b) AMPC method path, ms | (c) method path, one_launch_sample, ms | '
          '(d) NADP native, ms | (b) / (a) | (c) / (a) | (a) within the rule |\n|---|---|---|---|---|---|---|---|---|---|', flush=True)
    for env, B in SIZES:
        r = case(env, B)
        # the rule: the native median at or below the method path's; "above" only if it also lies beyond the method path's own range
        verdict = 'yes' if r[0][0] <= r[1][0] else ('within the range' if r[0][0] <= r[1][2] else 'NO: above the range')
        out['step'].append(dict(env=env, B=B, sample='8 x 64' if env == PT else '1 x 512', verdict=verdict,
                                **{k: dict(median_ms=x[0], range_ms=(x[1], x[2])) for k, x in zip(NAMES, r)}))
        print('| %s | %s | %d | %s | %s | %s | %s | %.2f | %.2f | %s |' % (env, '8 x 64' if env == PT else '1 x 512', B, fmt(r[0]), fmt(r[1]),
                                                                          fmt(r[2]), fmt(r[3]), r[1][0] / r[0][0], r[2][0] / r[0][0], verdict),
              flush=True)
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
