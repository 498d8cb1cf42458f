#!/usr/bin/env python3
"""Times of the AMPC path on the GPU, one process, medians of REGIONS timed regions of REPS steps after a warm-up (device events
around the region, a synchronise at its end), the candidates alternating region by region; PathTracking-v0, n = 25, B = 256 and 4096:

  (a) mpg_ampc_pg (the composed form: forward sweep at the single slice n, k_ampc_returns, reverse sweep, weight gradients over
      n + 1 steps) beside mpg_rollout_pg(all_steps_param_grad = 1, select = [n]) - the same sweeps with the critic's three launches,
      i.e. what leaving the critic out is worth.  A critic-free instantiation of the sweeps, once one exists, is the third column's
      place: it ships only if its median is at or below the composed form's at both sizes;
  (b) one AMPC step against one NADP step, both through SingleProcessOffPolicyOptimizer's method-by-method path (fused=False) on
      PathTracking-v0.  No bar: NADP is the comparison because AMPC has no earlier number.

    python tools/bench_ampc.py [--json out.json]          prints the markdown tables of DESIGN.md 7, f8"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpg_amd import ops                                      # noqa: E402
from tests.golden_inputs import mlp_weights_flat, reset_law_obs   # noqa: E402

REGIONS, REPS, WARMUP, N = 7, 200, 40, 25


def timed(fn, reps=REPS):
    """ms per call of one region"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(fns):
    """medians and ranges of the candidates, one region each in turn"""
    for f in fns:
        for _ in range(WARMUP):
            f()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(REGIONS):
        for k, f in enumerate(fns):
            t[k].append(timed(f))
    return [(statistics.median(x), min(x), max(x)) for x in t]


def entry_point_case(B):
    rng = np.random.Generator(np.random.PCG64(B))
    dev = 'cuda'
    cfg = ops.make_cfg()
    flat = torch.as_tensor(np.concatenate([mlp_weights_flat(rng, 8, 1), mlp_weights_flat(rng, 6, 4)])).to(dev)
    q1, pol = flat[:ops.q_size(cfg)], flat[ops.q_size(cfg):]
    wc = ops.WeightCache(flat, [(8, 1), (6, 4)])            # the learners' form: packed images, the THIN reverse sweep
    cfg.wcache[0] = wc.pointer
    obs = torch.as_tensor(reset_law_obs(rng, B)).to(dev)
    grad, stats = torch.empty(ops.policy_size(cfg), device=dev), torch.empty(2, device=dev)

    def composed():
        ops.ampc_pg(cfg, pol, obs, None, n=N, grad_out=grad, stats_out=stats, noise_seed=1, noise_ctr=2)

    def with_critic():
        ops.rollout_pg(cfg, pol, q1, obs, None, [N], [1.0], all_steps_param_grad=True, grad_out=grad, stats_out=stats, n=N, noise_seed=1,
                       noise_ctr=2)
    out = alternate([composed, with_critic])
    del wc
    return out


def stack(alg, B):
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import AMPCLearner, NADPLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    args = default_args(alg, env_id='PathTracking-v0', replay_batch_size=B, replay_starts=max(3000, B), nan_check_interval=10 ** 9,
                        num_agent=512)
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    learner = (AMPCLearner if alg == 'AMPC' else NADPLearner)(PolicyWithQs, args)
    opt = SingleProcessOffPolicyOptimizer(worker, learner, ReplayBuffer(args, 0), None, args, fused=False)
    assert opt._fused is None
    return opt


def step_case(B):
    from mpg_amd.optimizer import quiesce_gc
    a, b = stack('AMPC', B), stack('NADP', B)
    quiesce_gc()
    return alternate([a.step, b.step])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 4096])
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_ampc.py needs a GPU: nothing here is measured without one'
    fmt = lambda r: '%.4f (%.4f .. %.4f)' % r
    out = {'entry_point': [], 'step': []}
    print('| B | (a) mpg_ampc_pg, composed, ms | mpg_rollout_pg all steps, one slice (with the critic), ms | ratio |\n|---|---|---|---|')
    for B in a.sizes:
        c, q = entry_point_case(B)
        out['entry_point'].append(dict(B=B, composed_ms=c, with_critic_ms=q))
        print('| %d | %s | %s | %.3f |' % (B, fmt(c), fmt(q), c[0] / q[0]))
    print('\n| B | (b) AMPC step, method path, ms | NADP step, method path, ms | ratio |\n|---|---|---|---|')
    for B in a.sizes:
        x, y = step_case(B)
        out['step'].append(dict(B=B, ampc_ms=x, nadp_ms=y))
        print('| %d | %s | %s | %.3f |' % (B, fmt(x), fmt(y), x[0] / y[0]))
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
