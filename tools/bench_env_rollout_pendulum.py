#!/usr/bin/env python3
"""Times of MPG-v1's real-env sampler on the inverted pendulum, one process, medians of REGIONS timed regions after a warm-up (device
events around REPS back-to-back calls, a synchronise at the end of every region):

  (a) the chain of stand-alone launches - mpg_env_reset_from_obs, then per step mpg_policy_action (from the second step on) and
      mpg_env_step: 2 n launches, enqueued by the C loop of tools/bench_ndpg_chain.c (compiled on first use), REPS chains per call;
  (b) mpg_env_rollout_pendulum, the same computation as ONE launch (bit-identical: tests/test_env_rollout_pendulum_gpu.py; asserted
      here on the timed buffers too);
      both at rows 256 (the parser's replay_batch_size) and 4096, n = 25, both weight forms (packed image / strided), the two
      alternating region by region;
  (c) one native MPG-v1 step (learner_version 1) at the pendulum defaults, B = 256, num_batch_reuse 10 and 1 (the worst case: a fresh
      batch, its rollout and its clipped target on every step), with the launch and with the chain kept (sample_iters < 0).  The worker
      does not sample inside the timed regions (sampling_interval beyond them), so the pair differs in the learner's sampler alone.

    python tools/bench_env_rollout_pendulum.py [--json out.json]          prints markdown tables"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mpg_amd import _lib as L                                # noqa: E402
from mpg_amd import ops                                      # noqa: E402
from bench_ndpg import host_loops, timed                     # noqa: E402  (the C loops and the region timer of the PathTracking tool)
from tests.golden_inputs import mlp_weights_flat             # noqa: E402

REGIONS, REPS, WARMUP = 5, 200, 5
ENV_ID = 'InvertedPendulumConti-v0'
I = ctypes.c_int


def sampler_case(rows, cache, n=25):
    rng = np.random.Generator(np.random.PCG64(rows + int(cache)))
    dev = 'cuda'
    cfg = ops.make_cfg(ENV_ID)
    pol = torch.as_tensor(mlp_weights_flat(rng, 4, 2)).to(dev)
    wc = None
    if cache:
        wc = ops.WeightCache(pol, [(4, 2)])
        cfg.wcache[0] = wc.pointer
    obs0 = torch.as_tensor((rng.uniform(-1, 1, (rows, 4)) * np.array([1.9, 0.2, 1.0, 1.0])).astype(np.float32)).to(dev)
    act0 = torch.as_tensor(rng.uniform(-3, 3, (rows, 1)).astype(np.float32)).to(dev)
    state, obs, act = torch.zeros(8, rows, device=dev), torch.empty(rows, 4, device=dev), torch.empty(rows, 1, device=dev)
    rew_a, rew_b, last_b = torch.empty(n, rows, device=dev), torch.empty(n, rows, device=dev), torch.empty(rows, 4, device=dev)
    done, done_i = torch.empty(rows, dtype=torch.uint8, device=dev), torch.empty(rows, dtype=torch.uint8, device=dev)
    lib, s, c = L.lib(), L.stream(), ctypes.byref(cfg)
    p = L.ptr
    fp = lambda f: ctypes.cast(f, ctypes.c_void_p)
    host = host_loops()

    def chain(reps):
        assert host.bench_chain(fp(lib.mpg_env_reset_from_obs), fp(lib.mpg_policy_action), fp(lib.mpg_env_step), c, p(pol), I(rows), I(n),
                                p(obs0), p(act0), p(state), p(obs), p(act), p(rew_a), p(done), p(done_i), s, I(reps)) == 0

    def launch(reps):
        assert host.bench_launch(fp(lib.mpg_env_rollout_pendulum), c, p(pol), I(rows), I(n), p(obs0), p(act0), p(rew_b), p(last_b), s,
                                 I(reps)) == 0
    chain(WARMUP), launch(WARMUP)
    torch.cuda.synchronize()
    assert torch.equal(rew_a.view(torch.int32), rew_b.view(torch.int32)) and torch.equal(obs.view(torch.int32), last_b.view(torch.int32))
    ta, tb = [], []
    for _ in range(REGIONS):                                  # alternating: both see the same machine
        ta.append(timed(chain, REPS, batched=True))
        tb.append(timed(launch, REPS, batched=True))
    keep = (wc, state, done, done_i)                          # (alive until here)
    del keep
    return statistics.median(ta), statistics.median(tb), (min(ta), max(ta)), (min(tb), max(tb))


def step_case(reuse, chain, iters=100):
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import MPGLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer, quiesce_gc
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    args = default_args('MPG-v1', env_id=ENV_ID, num_batch_reuse=reuse, nan_check_interval=10 ** 9, one_launch_sample=True)
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    opt = SingleProcessOffPolicyOptimizer(worker, MPGLearner(PolicyWithQs, args), ReplayBuffer(args, 0), None, args, sampling_interval=10 ** 9)
    assert opt._fused is not None and args.replay_batch_size == 256 and opt._fused.c.learner_version == 1
    if chain:
        opt._fused.c.sample_iters = -opt._fused.c.sample_iters
    quiesce_gc()
    for _ in range(40):                                       # (iteration 0 samples; none of the timed ones does)
        opt.step()
    torch.cuda.synchronize()
    t = [timed(opt.step, iters) for _ in range(REGIONS)]      # (iters a multiple of the reuse count)
    return statistics.median(t), (min(t), max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_env_rollout_pendulum.py needs a GPU: nothing here is measured without one'
    out = {'sampler': [], 'step': []}
    print('| rows | W2 | (a) chain, 50 launches, ms | (b) mpg_env_rollout_pendulum, ms | (a) / (b) |\n|---|---|---|---|---|', flush=True)
    for rows in (256, 4096):
        for cache in (True, False):
            ma, mb, ra, rb = sampler_case(rows, cache)
            form = 'packed' if cache else 'strided'
            out['sampler'].append(dict(rows=rows, weights=form, chain_ms=ma, chain_range=ra, rollout_ms=mb, rollout_range=rb))
            print('| %d | %s | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) | %.2f |' % (rows, form, ma, ra[0], ra[1], mb, rb[0], rb[1], ma / mb),
                  flush=True)
    print('\n| native MPG-v1 step on the pendulum, B = 256 | the launch, ms per step | the chain kept, ms per step |\n|---|---|---|', flush=True)
    for reuse in (10, 1):
        (ml, rl), (mc, rc) = step_case(reuse, False), step_case(reuse, True)
        out['step'].append(dict(num_batch_reuse=reuse, launch_ms=ml, launch_range=rl, chain_ms=mc, chain_range=rc))
        print('| num_batch_reuse %d | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) |' % (reuse, ml, rl[0], rl[1], mc, rc[0], rc[1]), flush=True)
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
