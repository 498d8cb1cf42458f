#!/usr/bin/env python3
"""Gradient-step time of NADP on the InvertedDoublePendulum-v2 model at config 3's batch (B = 8192), with config 3 itself (NADP on
the single-pendulum model) timed in the same process for context - timed as tools/bench_configs.py times C3: warm-up, then a host
clock around a window that ends in a device synchronise.  One JSON line each.

    python tools/bench_double_pendulum.py [--iters 300] [--only dp|c3]     (--only dp: the run to put under a kernel trace)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
DEV = 'cuda'


def timed(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def nadp_step(env_id, B, obs, act):
    from mpg_amd.config import default_args
    from mpg_amd.learners import NADPLearner
    from mpg_amd.policy import PolicyWithQs
    learner = NADPLearner(PolicyWithQs, default_args('NADP', env_id=env_id, replay_batch_size=B))
    pw = learner.policy_with_value
    batch = [obs, act, torch.zeros(B, device=DEV), obs, torch.zeros(B, device=DEV)]
    it = [0]

    def step():
        learner.compute_gradient(batch, None, None, it[0])
        pw.apply_gradients(it[0], learner.flat_grad)
        it[0] += 1
    return step, pw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=300)
    ap.add_argument('--only', choices=['dp', 'c3'], default=None)
    a = ap.parse_args()
    B = 8192
    if a.only != 'c3':
        # gym's reset law for the start observations (tests/golden/make_golden_dp.py:start_obs), actions in [-1, 1]
        rng = np.random.Generator(np.random.PCG64(0))
        th = rng.uniform(-0.1, 0.1, (B, 2))
        obs = np.concatenate([rng.uniform(-0.1, 0.1, (B, 1)), np.sin(th), np.cos(th), 0.1 * rng.standard_normal((B, 3)),
                              0.1 * rng.standard_normal((B, 3))], 1).astype(np.float32)
        act = rng.uniform(-1, 1, (B, 1)).astype(np.float32)
        step, pw = nadp_step('InvertedDoublePendulum-v2', B, torch.as_tensor(obs).to(DEV), torch.as_tensor(act).to(DEV))
        t = timed(step, a.iters)
        print(json.dumps(dict(what='NADP InvertedDoublePendulum-v2 model B=8192 (compute_gradient + apply_gradients)', iters=a.iters,
                              ms_per_grad_step=t * 1e3, grad_steps_per_s=1 / t, status_word=int(pw.status.item()))), flush=True)
    if a.only != 'dp':
        g = torch.Generator(device='cpu').manual_seed(0)
        obs = (torch.randn(B, 4, generator=g) * torch.tensor([0.5, 0.1, 0.5, 0.5])).to(DEV)
        act = ((torch.rand(B, 1, generator=g) * 6) - 3).to(DEV)
        step, pw = nadp_step('InvertedPendulumConti-v0', B, obs, act)
        t = timed(step, a.iters)
        print(json.dumps(dict(what='C3 NADP pendulum model B=8192 (compute_gradient + apply_gradients)', iters=a.iters,
                              ms_per_grad_step=t * 1e3, grad_steps_per_s=1 / t)), flush=True)


if __name__ == '__main__':
    main()
