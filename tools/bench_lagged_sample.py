#!/usr/bin/env python3
"""Times of one native step with and without the lagged worker sample (SingleProcessOffPolicyOptimizer(sample_lag=L); include/mpg_hip.h,
mpg_lagged_sample_t) on the GPU, one process, medians of REGIONS timed regions of REPS steps after a warm-up (device events around the
region on the step's stream; a lagged form drains inside its region, so that every sample it started is paid for there), the forms
alternating region by region:

  (a)  the plain native step: the sample and its add on the step's stream, every 10th step;
  (b)  lagged, ONE stream (side = NULL): the same calls in the lagged order - what the reordering alone costs or gains;
  (c)  lagged, TWO streams: the sample beside the steps,
each lagged form at L = 1 and L = sampling_interval = 10.

(a) against (c) is the result; (b) against (c) isolates the overlap from the reordering.  Stacks: TD3 and SAC on PathTracking-v0 (8 agents
x 64 iterations per sample) and NADP on InvertedPendulumConti-v0 (1 agent x 512 iterations) at their parsers' worker defaults, B = 256, and
TD3 at B = 4096.  No threshold is attached: the table says what was measured.

    python tools/bench_lagged_sample.py [--json out.json]          prints the markdown table of DESIGN.md 7, f18"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REGIONS, REPS, WARMUP, INTERVAL = 7, 200, 40, 10
PT, PD = 'PathTracking-v0', 'InvertedPendulumConti-v0'
CASES = [('TD3', PT, 256), ('SAC', PT, 256), ('NADP', PD, 256), ('TD3', PT, 4096)]
# name -> (lag, streams)
FORMS = [('a_plain', (None, 0)), ('b_one_stream_L1', (1, 1)), ('c_two_streams_L1', (1, 2)), ('b_one_stream_L10', (INTERVAL, 1)),
         ('c_two_streams_L10', (INTERVAL, 2))]


def stack(alg, env, B, lag, streams):
    from mpg_amd import learners
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    args = default_args(alg, env_id=env, replay_batch_size=B, replay_starts=max(3000, B), nan_check_interval=10 ** 9)
    assert (args.num_agent, args.batch_size) == ((8, 512) if env == PT else (1, 512))
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    learner = getattr(learners, alg + 'Learner')(PolicyWithQs, args)
    more = dict(native_sac=True) if alg == 'SAC' else {}
    opt = SingleProcessOffPolicyOptimizer(worker, learner, ReplayBuffer(args, 0), None, args, sampling_interval=INTERVAL, sample_lag=lag, **more)
    assert opt._fused is not None
    if streams == 1:
        opt._fused.lagged.side = None
    return opt


def timed(opt, reps=REPS):
    """ms per step of one region"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        opt.step()
    opt.drain()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def case(alg, env, B):
    from mpg_amd.optimizer import quiesce_gc
    opts = [stack(alg, env, B, *form) for _, form in FORMS]
    quiesce_gc()
    for _ in range(WARMUP):
        for o in opts:
            o.step()
    torch.cuda.synchronize()
    t = [[] for _ in opts]
    for _ in range(REGIONS):                                  # alternating: every form sees the same machine
        for k, o in enumerate(opts):
            t[k].append(timed(o))
    torch.cuda.synchronize()
    # one lag, one result: the stream count changes no bit
    p = [o.worker.policy_with_value.params.view(torch.int32) for o in opts]
    assert torch.equal(p[1], p[2]) and torch.equal(p[3], p[4]), 'forms of one lag diverged'
    for o in opts:
        o.worker.policy_with_value.check_status()
    return [(statistics.median(x), min(x), max(x)) for x in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_lagged_sample.py needs a GPU: nothing here is measured without one'
    fmt = lambda r: '%.4f (%.4f .. %.4f)' % r
    out = {'regions': REGIONS, 'reps': REPS, 'warmup': WARMUP, 'sampling_interval': INTERVAL, 'step': []}
    print('| stack | B | (a) plain, ms | (b) one stream L=1 | (c) two streams L=1 | (b) one stream L=10 | (c) two streams L=10 | '
          '(c) / (a), L=1 | (c) / (a), L=10 |\n|---|---|---|---|---|---|---|---|---|', flush=True)
    for alg, env, B in CASES:
        r = case(alg, env, B)
        out['step'].append(dict(alg=alg, env=env, B=B, **{k: dict(median_ms=x[0], range_ms=(x[1], x[2])) for (k, _), x in zip(FORMS, r)}))
        print('| %s, %s | %d | %s | %.2f | %.2f |' % (alg, env, B, ' | '.join(fmt(x) for x in r), r[2][0] / r[0][0], r[4][0] / r[0][0]), flush=True)
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
