#!/usr/bin/env python3
"""Times of the n-step DPG path on the GPU, one process, medians of REGIONS timed regions after a warm-up (device events around
REPS back-to-back calls, a synchronise at the end of every region):

  (a) the real-env n-step sampler as the chain of stand-alone launches - mpg_env_reset_from_obs, then per step mpg_policy_action
      (from the second step on) and mpg_env_step: what train_step.cpp enqueues for MPG-v1, enqueued by the same C loop
      (tools/bench_ndpg_chain.c, compiled on first use), REPS chains per call into it;
  (b) mpg_env_rollout, the same computation as ONE launch (bit-identical: tests/test_ndpg_gpu.py);
      both at rows 256 and 4096, n = 25, obs_dim 6 and 9, the two alternating region by region;
  (c) one native NDPG step (learner_version 5) at B = 256 with num_batch_reuse 1 and 10.

    python tools/bench_ndpg.py [--json out.json]          prints a markdown table (EXPERIMENTS.md)"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpg_amd import _lib as L                                # noqa: E402
from mpg_amd import ops                                      # noqa: E402
from tests.golden_inputs import mlp_weights_flat, reset_law_obs   # noqa: E402

REGIONS, REPS, WARMUP = 7, 200, 5
I, F, U64 = ctypes.c_int, ctypes.c_float, ctypes.c_uint64


def host_loops():
    """tools/bench_ndpg_chain.c as a shared object beside it (rebuilt when the source is newer)"""
    here = os.path.dirname(os.path.abspath(__file__))
    src, so = os.path.join(here, 'bench_ndpg_chain.c'), os.path.join(here, 'bench_ndpg_chain.so')
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call([os.environ.get('CC', 'cc'), '-O2', '-shared', '-fPIC', '-I' + os.path.join(here, '..', 'include'), src, '-o', so])
    return ctypes.CDLL(so)


def timed(fn, reps=REPS, batched=False):
    """ms per call of one region: device events around `reps` calls (batched: fn(reps) issues them itself)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    if batched:
        fn(reps)
    else:
        for _ in range(reps):
            fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def sampler_case(rows, od, n=25):
    rng = np.random.Generator(np.random.PCG64(rows + od))
    dev = 'cuda'
    cfg = ops.make_cfg(obs_dim=od)
    pol = torch.as_tensor(mlp_weights_flat(rng, od, 4)).to(dev)
    wc = ops.WeightCache(pol, [(od, 4)])
    cfg.wcache[0] = wc.pointer
    obs0 = torch.as_tensor(np.concatenate([reset_law_obs(rng, rows), np.zeros((rows, od - 6), np.float32)], 1)).to(dev)
    act0 = torch.as_tensor(rng.uniform(-1, 1, (rows, 2)).astype(np.float32)).to(dev)
    state, obs, act = torch.zeros(8, rows, device=dev), torch.empty(rows, od, device=dev), torch.empty(rows, 2, device=dev)
    rew_a, rew_b, last_b = torch.empty(n, rows, device=dev), torch.empty(n, rows, device=dev), torch.empty(rows, od, device=dev)
    done, done_i = torch.empty(rows, dtype=torch.uint8, device=dev), torch.empty(rows, dtype=torch.uint8, device=dev)
    lib, s, c = L.lib(), L.stream(), ctypes.byref(cfg)
    p = L.ptr
    fp = lambda f: ctypes.cast(f, ctypes.c_void_p)
    host = host_loops()

    def chain(reps):
        assert host.bench_chain(fp(lib.mpg_env_reset_from_obs), fp(lib.mpg_policy_action), fp(lib.mpg_env_step), c, p(pol), I(rows), I(n),
                                p(obs0), p(act0), p(state), p(obs), p(act), p(rew_a), p(done), p(done_i), s, I(reps)) == 0

    def launch(reps):
        assert host.bench_launch(fp(lib.mpg_env_rollout), c, p(pol), I(rows), I(n), p(obs0), p(act0), p(rew_b), p(last_b), s, I(reps)) == 0
    chain(WARMUP), launch(WARMUP)
    torch.cuda.synchronize()
    assert torch.equal(rew_a.view(torch.int32), rew_b.view(torch.int32)) and torch.equal(obs.view(torch.int32), last_b.view(torch.int32))
    ta, tb = [], []
    for _ in range(REGIONS):                                  # alternating: both see the same machine
        ta.append(timed(chain, batched=True))
        tb.append(timed(launch, batched=True))
    keep = (wc, state, done, done_i)                          # (alive until here)
    del keep
    return statistics.median(ta), statistics.median(tb), (min(ta), max(ta)), (min(tb), max(tb))


def step_case(reuse, iters=200):
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import NDPGLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer, quiesce_gc
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    args = default_args('NDPG', num_batch_reuse=reuse, nan_check_interval=10 ** 9)
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    opt = SingleProcessOffPolicyOptimizer(worker, NDPGLearner(PolicyWithQs, args), ReplayBuffer(args, 0), None, args)
    assert opt._fused is not None and args.replay_batch_size == 256
    quiesce_gc()
    for _ in range(40):
        opt.step()
    torch.cuda.synchronize()
    t = [timed(opt.step, iters) for _ in range(REGIONS)]      # (iters a multiple of the sampling interval and of the reuse count)
    return statistics.median(t), (min(t), max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_ndpg.py needs a GPU: nothing here is measured without one'
    out = {'sampler': [], 'step': []}
    print('| rows | obs_dim | (a) chain, 50 launches, ms | (b) mpg_env_rollout, ms | (a) / (b) |\n|---|---|---|---|---|')
    for rows in (256, 4096):
        for od in (6, 9):
            ma, mb, ra, rb = sampler_case(rows, od)
            out['sampler'].append(dict(rows=rows, obs_dim=od, chain_ms=ma, chain_range=ra, rollout_ms=mb, rollout_range=rb))
            print('| %d | %d | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) | %.2f |' % (rows, od, ma, ra[0], ra[1], mb, rb[0], rb[1], ma / mb))
    print('\n| native NDPG step, B = 256 | ms per step |\n|---|---|')
    for reuse in (1, 10):
        m, r = step_case(reuse)
        out['step'].append(dict(num_batch_reuse=reuse, step_ms=m, step_range=r))
        print('| num_batch_reuse %d | %.4f (%.4f .. %.4f) |' % (reuse, m, r[0], r[1]))
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
