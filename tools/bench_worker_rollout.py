#!/usr/bin/env python3
"""Times of one worker sample on the GPU, one process, medians of REGIONS timed regions after a warm-up (device events around REPS
back-to-back samples, a synchronise at the end of every region):

  (a) the sample as the chain of `iters` mpg_worker_step launches - what sample of train_step.cpp enqueues without the
      one-launch form - enqueued by a C loop (tools/bench_worker_rollout_chain.c, compiled on first use), REPS samples per call into it;
  (b) mpg_worker_rollout, the same sample as ONE launch (bit-identical: tests/test_worker_rollout_gpu.py; asserted here at the end);
      cases (agents, iters, obs_dim) = (8, 64, 6), (256, 16, 6), (8, 64, 9), (256, 16, 9), explore_sigma 0.1, the packed weight
      image, the two alternating region by region;
  (c) one native step at the reference's worker defaults (num_agent 8, batch_size 512, sampling every 10th step), B = 256, for TD3
      and MPG-v2: the driver as it decides, and the same driver with the chain kept (mpg_train_ctx_t.sample_iters < 0), alternating.

The rule for the driver: it calls (b) for a width only if (b)'s median is at or below (a)'s at both sizes of that width.

    python tools/bench_worker_rollout.py [--json out.json]          prints markdown tables (EXPERIMENTS.md)
    python tools/bench_worker_rollout.py --steps-only [--tree DIR]  (c) alone; --tree: time another checkout's build (a parent commit)
    python tools/bench_worker_rollout.py --env pendulum [...]       the same for InvertedPendulumConti-v0: (a) the chain of `iters` pairs
        mpg_policy_action + mpg_env_step_store_reset against (b) mpg_worker_rollout_pendulum at (agents, iters, explore_sigma) =
        (1, 512, 0.1), (1, 512, 0), (64, 8, 0.1), and (c) one native NADP step at the pendulum parser's defaults (1 agent, 512
        iterations per sample, B = 256)
    python tools/bench_worker_rollout.py --env pendulum --stochastic [--json out.json]   the tanh-squashed Gaussian policy on the pendulum:
        (a) the chain of `iters` triples mpg_normal_fill + mpg_policy_sample_squashed + mpg_env_step_store_reset (four launches per
        iteration) against (b) mpg_worker_sample_rollout_pendulum at (agents, iters) = (1, 512) - the reference's SAC defaults - and
        (64, 8), and (d) OffPolicyWorker.sample() of the squashed SAC stack at 1 x 512 on its loop and with one_launch_sample, alternating
    python tools/bench_worker_rollout.py --stochastic [--steps-only] [--json out.json]   a stochastic policy on PathTracking-v0 (SAC):
        (a) the chain - the plain Gaussian head: `iters` mpg_worker_sample_step launches, what sample of train_step.cpp
        enqueues without the one-launch form; the tanh-squashed head (action_range 1.5): `iters` triples mpg_normal_fill +
        mpg_policy_sample_squashed + mpg_env_step_store_reset - against (b) mpg_worker_sample_rollout at the four cases of the
        deterministic measurement, (d) OffPolicyWorker.sample() of both SAC stacks at 8 x 64 on the loop and with one_launch_sample, and
        (c) one native SAC step (fixed and learned temperature) as the driver decides against the chain kept (sample_iters = -64);
        --steps-only: (c) alone.  The driver's rule per width is the one above, on the plain head's rows.
    python tools/bench_worker_rollout.py --env model [--json out.json]   the model-backed InvertedDoublePendulum-v2 env: (a) the chain of
        `iters` pairs mpg_policy_action + mpg_model_env_step_store_reset against (b) mpg_worker_rollout_model at (agents, iters,
        explore_sigma) = (1, 512, 0) - the reference-shaped defaults -, (1, 512, 0.1) and (64, 8, 0).  The launch is taken on request
        (args.one_launch_sample) and the native step driver does not serve this env: no rule, no step times."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

REGIONS, REPS, WARMUP = 7, 200, 5
I, F, U64 = ctypes.c_int, ctypes.c_float, ctypes.c_uint64
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ((8, 64, 6), (256, 16, 6), (8, 64, 9), (256, 16, 9))


class Side(ctypes.Structure):               # worker_side_t, tools/bench_worker_rollout_chain.c
    _fields_ = [(k, ctypes.c_void_p) for k in ('state', 'obs', 'act', 'ring_obs', 'ring_act', 'ring_rew', 'ring_obs2', 'ring_done', 'done')] + \
               [('capacity', I), ('next_idx', I), ('ctr', U64)]


def host_loops():
    """tools/bench_worker_rollout_chain.c as a shared object beside it (rebuilt when the source is newer)"""
    src, so = os.path.join(HERE, 'bench_worker_rollout_chain.c'), os.path.join(HERE, 'bench_worker_rollout_chain.so')
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call([os.environ.get('CC', 'cc'), '-O2', '-shared', '-fPIC', '-I' + os.path.join(HERE, '..', 'include'), src, '-o', so])
    return ctypes.CDLL(so)


def timed(fn, reps=REPS, batched=False):
    """ms per call of one region: device events around `reps` calls (batched: fn(reps) issues them itself)"""
    import torch
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


def sample_case(n, iters, od, sigma=0.1):
    import numpy as np
    import torch
    from mpg_amd import _lib as L
    from mpg_amd import ops
    from mpg_amd.envs import PathTrackingEnv
    from tests.golden_inputs import mlp_weights_flat
    rng = np.random.Generator(np.random.PCG64(n + od))
    dev = 'cuda'
    cfg = ops.make_cfg(obs_dim=od)
    pol = torch.as_tensor(mlp_weights_flat(rng, od, 4)).to(dev)
    wc = ops.WeightCache(pol, [(od, 4)])
    cfg.wcache[0] = wc.pointer
    cap = 4 * iters * n + 3 * n                   # (the ring position wraps inside a sample now and then)
    sides, keep = [], []
    for _ in range(2):
        env = PathTrackingEnv(num_agent=n, num_future_data=od - 6, seed=4)
        t = dict(state=env._state, obs=env.reset().clone(), act=torch.empty(n, 2, device=dev), ring_obs=torch.zeros(cap, od, device=dev),
                 ring_act=torch.zeros(cap, 2, device=dev), ring_rew=torch.zeros(cap, device=dev), ring_obs2=torch.zeros(cap, od, device=dev),
                 ring_done=torch.zeros(cap, dtype=torch.uint8, device=dev), done=torch.zeros(n, dtype=torch.uint8, device=dev))
        sd = Side(capacity=cap, next_idx=0, ctr=1)
        for k, v in t.items():
            setattr(sd, k, v.data_ptr())
        sides.append((t, sd))
        keep.append(env)
    lib, s, c = L.lib(), L.stream(), ctypes.byref(cfg)
    fp = lambda f: ctypes.cast(f, ctypes.c_void_p)
    host = host_loops()

    def chain(reps):
        assert host.bench_chain(fp(lib.mpg_worker_step), c, L.ptr(pol), I(n), I(iters), F(sigma), ctypes.byref(sides[0][1]), s, I(reps)) == 0

    def launch(reps):
        assert host.bench_launch(fp(lib.mpg_worker_rollout), c, L.ptr(pol), I(n), I(iters), F(sigma), ctypes.byref(sides[1][1]), s, I(reps)) == 0
    chain(WARMUP), launch(WARMUP)
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(REGIONS):                                      # alternating: both see the same machine
        ta.append(timed(chain, batched=True))
        tb.append(timed(launch, batched=True))
    torch.cuda.synchronize()
    for k in sides[0][0]:                                         # the two did the same work: bit-identical at the end
        a, b = sides[0][0][k], sides[1][0][k]
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), k
    del keep, wc
    return statistics.median(ta), statistics.median(tb), (min(ta), max(ta)), (min(tb), max(tb))


PENDULUM_CASES = ((1, 512, 0.1), (1, 512, 0.), (64, 8, 0.1))       # (agents, iters, explore_sigma); 1 x 512: the reference's defaults


def sample_case_pendulum(n, iters, sigma):
    """--env pendulum: (a) the chain of `iters` pairs mpg_policy_action + mpg_env_step_store_reset (two launches per iteration, what
    sample's loop enqueues on this env) against (b) mpg_worker_rollout_pendulum, as sample_case does it"""
    import numpy as np
    import torch
    from mpg_amd import _lib as L
    from mpg_amd import ops
    from mpg_amd.envs import InvertedPendulumContiEnv
    from tests.golden_inputs import mlp_weights_flat
    rng = np.random.Generator(np.random.PCG64(n + 4))
    dev = 'cuda'
    cfg = ops.make_cfg('InvertedPendulumConti-v0')
    pol = torch.as_tensor(mlp_weights_flat(rng, 4, 2)).to(dev)
    wc = ops.WeightCache(pol, [(4, 2)])
    cfg.wcache[0] = wc.pointer
    cap = 4 * iters * n + 3 * n                   # (the ring position wraps inside a sample now and then)
    sides, keep = [], []
    for _ in range(2):
        env = InvertedPendulumContiEnv(num_agent=n, seed=4)
        t = dict(state=env._state, obs=env.reset().clone(), act=torch.empty(n, 1, device=dev), ring_obs=torch.zeros(cap, 4, device=dev),
                 ring_act=torch.zeros(cap, 1, device=dev), ring_rew=torch.zeros(cap, device=dev), ring_obs2=torch.zeros(cap, 4, device=dev),
                 ring_done=torch.zeros(cap, dtype=torch.uint8, device=dev), done=torch.zeros(n, dtype=torch.uint8, device=dev))
        sd = Side(capacity=cap, next_idx=0, ctr=1)
        for k, v in t.items():
            setattr(sd, k, v.data_ptr())
        sides.append((t, sd))
        keep.append(env)
    lib, s, c = L.lib(), L.stream(), ctypes.byref(cfg)
    fp = lambda f: ctypes.cast(f, ctypes.c_void_p)
    host = host_loops()

    def chain(reps):
        assert host.bench_chain_pendulum(fp(lib.mpg_policy_action), fp(lib.mpg_env_step_store_reset), c, L.ptr(pol), I(n), I(iters), F(sigma),
                                         ctypes.byref(sides[0][1]), s, I(reps)) == 0

    def launch(reps):
        assert host.bench_launch(fp(lib.mpg_worker_rollout_pendulum), c, L.ptr(pol), I(n), I(iters), F(sigma), ctypes.byref(sides[1][1]), s,
                                 I(reps)) == 0
    chain(WARMUP), launch(WARMUP)
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(REGIONS):                                      # alternating: both see the same machine
        ta.append(timed(chain, batched=True))
        tb.append(timed(launch, batched=True))
    torch.cuda.synchronize()
    for k in sides[0][0]:                                         # the two did the same work: bit-identical at the end
        a, b = sides[0][0][k], sides[1][0][k]
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), k
    fell = int(sides[1][0]['ring_done'].sum().item())             # (this env's done is real: how many of the ring's rows ended an episode)
    del keep, wc
    return statistics.median(ta), statistics.median(tb), (min(ta), max(ta)), (min(tb), max(tb)), fell, cap


MODEL_CASES = ((1, 512, 0.), (1, 512, 0.1), (64, 8, 0.))             # (agents, iters, explore_sigma); 1 x 512: the reference-shaped defaults


def sample_case_model(n, iters, sigma, max_steps=1000):
    """--env model: (a) the chain of `iters` pairs mpg_policy_action + mpg_model_env_step_store_reset (two launches per iteration, what
    sample's loop enqueues on the model-backed InvertedDoublePendulum-v2 env) against (b) mpg_worker_rollout_model, as sample_case does it"""
    import numpy as np
    import torch
    from mpg_amd import _lib as L
    from mpg_amd import ops
    from mpg_amd.envs import InvertedDoublePendulumModelEnv
    from tests.golden_inputs import mlp_weights_flat
    rng = np.random.Generator(np.random.PCG64(n + 11))
    dev = 'cuda'
    cfg = ops.make_cfg('InvertedDoublePendulum-v2')
    pol = torch.as_tensor(mlp_weights_flat(rng, 11, 2)).to(dev)
    wc = ops.WeightCache(pol, [(11, 2)])
    cfg.wcache[0] = wc.pointer
    cap = 4 * iters * n + 3 * n                   # (the ring position wraps inside a sample now and then)
    sides, keep = [], []
    for _ in range(2):
        env = InvertedDoublePendulumModelEnv(num_agent=n, seed=4, max_episode_steps=max_steps)
        t = dict(state=env._state, obs=env.reset().clone(), act=torch.empty(n, 1, device=dev), ring_obs=torch.zeros(cap, 11, device=dev),
                 ring_act=torch.zeros(cap, 1, device=dev), ring_rew=torch.zeros(cap, device=dev), ring_obs2=torch.zeros(cap, 11, device=dev),
                 ring_done=torch.zeros(cap, dtype=torch.uint8, device=dev), done=torch.zeros(n, dtype=torch.uint8, device=dev))
        sd = Side(capacity=cap, next_idx=0, ctr=1)
        for k, v in t.items():
            setattr(sd, k, v.data_ptr())
        sides.append((t, sd))
        keep.append(env)
    lib, s, c = L.lib(), L.stream(), ctypes.byref(cfg)
    fp = lambda f: ctypes.cast(f, ctypes.c_void_p)
    host = host_loops()

    def chain(reps):
        assert host.bench_chain_model(fp(lib.mpg_policy_action), fp(lib.mpg_model_env_step_store_reset), c, L.ptr(pol), I(n), I(iters),
                                      I(max_steps), F(sigma), ctypes.byref(sides[0][1]), s, I(reps)) == 0

    def launch(reps):
        assert host.bench_launch_model(fp(lib.mpg_worker_rollout_model), c, L.ptr(pol), I(n), I(iters), I(max_steps), F(sigma),
                                       ctypes.byref(sides[1][1]), s, I(reps)) == 0
    chain(WARMUP), launch(WARMUP)
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(REGIONS):                                      # alternating: both see the same machine
        ta.append(timed(chain, batched=True))
        tb.append(timed(launch, batched=True))
    torch.cuda.synchronize()
    for k in sides[0][0]:                                         # the two did the same work: bit-identical at the end
        a, b = sides[0][0][k], sides[1][0][k]
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), k
    fell = int(sides[1][0]['ring_done'].sum().item())             # (how many of the ring's rows ended an episode: a fall or the limit)
    del keep, wc
    return statistics.median(ta), statistics.median(tb), (min(ta), max(ta)), (min(tb), max(tb)), fell, cap


STOCHASTIC_CASES = ((1, 512), (64, 8))                              # (agents, iters); 1 x 512: built_SAC_parser's defaults
SAMPLE_REPS = 20                                                    # worker.sample() calls per region (the loop form is 512 x 5 launches)


def sample_case_stochastic_pendulum(n, iters):
    """--env pendulum --stochastic: (a) the three entry points per iteration against (b) mpg_worker_sample_rollout_pendulum, as
    sample_case_pendulum does it"""
    import numpy as np
    import torch
    from mpg_amd import _lib as L
    from mpg_amd import ops
    from mpg_amd.envs import InvertedPendulumContiEnv
    from tests.golden_inputs import mlp_weights_flat
    rng = np.random.Generator(np.random.PCG64(n + 4))
    dev = 'cuda'
    cfg = ops.make_cfg('InvertedPendulumConti-v0')
    pol = torch.as_tensor(mlp_weights_flat(rng, 4, 2)).to(dev)
    wc = ops.WeightCache(pol, [(4, 2)])
    cfg.wcache[0] = wc.pointer
    cap = 4 * iters * n + 3 * n                   # (the ring position wraps inside a sample now and then)
    sides, keep = [], []
    for _ in range(2):
        env = InvertedPendulumContiEnv(num_agent=n, seed=4)
        t = dict(state=env._state, obs=env.reset().clone(), act=torch.empty(n, 1, device=dev), ring_obs=torch.zeros(cap, 4, device=dev),
                 ring_act=torch.zeros(cap, 1, device=dev), ring_rew=torch.zeros(cap, device=dev), ring_obs2=torch.zeros(cap, 4, device=dev),
                 ring_done=torch.zeros(cap, dtype=torch.uint8, device=dev), done=torch.zeros(n, dtype=torch.uint8, device=dev))
        sd = Side(capacity=cap, next_idx=0, ctr=1)
        for k, v in t.items():
            setattr(sd, k, v.data_ptr())
        sides.append((t, sd))
        keep.append(env)
    eps, logp = torch.empty(n, device=dev), torch.empty(n, device=dev)
    ws = ops._ws(dev, 0, 'mpg_policy_sample_squashed_workspace_bytes', cfg, n)
    lib, s, c = L.lib(), L.stream(), ctypes.byref(cfg)
    fp = lambda f: ctypes.cast(f, ctypes.c_void_p)
    host = host_loops()

    def chain(reps):
        assert host.bench_chain_sample_pendulum(fp(lib.mpg_normal_fill), fp(lib.mpg_policy_sample_squashed), fp(lib.mpg_env_step_store_reset), c,
                                                L.ptr(pol), I(n), I(iters), L.ptr(eps), L.ptr(logp), *ws, ctypes.byref(sides[0][1]), s,
                                                I(reps)) == 0

    def launch(reps):
        assert host.bench_launch_sample(fp(lib.mpg_worker_sample_rollout_pendulum), c, L.ptr(pol), I(n), I(iters), ctypes.byref(sides[1][1]), s,
                                        I(reps)) == 0
    chain(WARMUP), launch(WARMUP)
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(REGIONS):                                      # alternating: both see the same machine
        ta.append(timed(chain, batched=True))
        tb.append(timed(launch, batched=True))
    torch.cuda.synchronize()
    for k in sides[0][0]:                                         # the two did the same work: bit-identical at the end
        a, b = sides[0][0][k], sides[1][0][k]
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), k
    fell = int(sides[1][0]['ring_done'].sum().item())
    del keep, wc
    return statistics.median(ta), statistics.median(tb), (min(ta), max(ta)), (min(tb), max(tb)), fell, cap


def worker_sample_stochastic_pendulum(out):
    """(d): OffPolicyWorker.sample() of the squashed SAC stack at the reference's defaults (one agent, 512 iterations) on its loop and
    with one_launch_sample - host time included: the loop's launches are enqueued from Python, as a training run enqueues them"""
    import torch
    from mpg_amd.config import default_args
    from mpg_amd.optimizer import quiesce_gc
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    workers = []
    for one in (False, True):
        args = default_args('SAC', env_id='InvertedPendulumConti-v0', squashed_head=True, nan_check_interval=10 ** 9,
                            **(dict(one_launch_sample=True) if one else {}))
        assert (args.num_agent, args.batch_size, args.action_range) == (1, 512, 3.0)
        workers.append(OffPolicyWorker(PolicyWithQs, args.env_id, args, 0))
    quiesce_gc()
    for w in workers:
        for _ in range(WARMUP):
            w.sample()
    torch.cuda.synchronize()
    t = [[], []]
    for _ in range(REGIONS):
        for k, w in enumerate(workers):
            t[k].append(timed(w.sample, SAMPLE_REPS))
    for a, b in zip(workers[0].sample(), workers[1].sample()):    # the two did the same work: bit-identical at the end
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    print('\n| OffPolicyWorker.sample(), squashed SAC, InvertedPendulumConti-v0, num_agent 1, batch_size 512 | ms per sample |\n|---|---|', flush=True)
    for form, x in zip(('the loop (five launches per iteration)', 'one_launch_sample'), t):
        out['worker_sample'].append(dict(form=form, sample_ms=statistics.median(x), sample_range=(min(x), max(x))))
        print('| %s | %.4f (%.4f .. %.4f) |' % (form, statistics.median(x), min(x), max(x)), flush=True)


STOCHASTIC_RANGE = 1.5                                              # the squashed head's action range on PathTracking-v0


def sample_case_stochastic(n, iters, od, squashed):
    """--stochastic on PathTracking-v0: (a) the chain - `iters` mpg_worker_sample_step launches (plain head), or `iters` triples
    mpg_normal_fill + mpg_policy_sample_squashed + mpg_env_step_store_reset (squashed head) - against (b) mpg_worker_sample_rollout,
    as sample_case does it"""
    import numpy as np
    import torch
    from mpg_amd import _lib as L
    from mpg_amd import ops
    from mpg_amd.envs import PathTrackingEnv
    from tests.golden_inputs import mlp_weights_flat
    rng = np.random.Generator(np.random.PCG64(n + od))
    dev = 'cuda'
    cfg = ops.make_cfg(obs_dim=od, policy_out_activation='linear', action_range=STOCHASTIC_RANGE if squashed else None)
    pol = torch.as_tensor(mlp_weights_flat(rng, od, 4)).to(dev)
    wc = ops.WeightCache(pol, [(od, 4)])
    cfg.wcache[0] = wc.pointer
    cap = 4 * iters * n + 3 * n                   # (the ring position wraps inside a sample now and then)
    sides, keep = [], []
    for _ in range(2):
        env = PathTrackingEnv(num_agent=n, num_future_data=od - 6, seed=4)
        t = dict(state=env._state, obs=env.reset().clone(), act=torch.empty(n, 2, device=dev), ring_obs=torch.zeros(cap, od, device=dev),
                 ring_act=torch.zeros(cap, 2, device=dev), ring_rew=torch.zeros(cap, device=dev), ring_obs2=torch.zeros(cap, od, device=dev),
                 ring_done=torch.zeros(cap, dtype=torch.uint8, device=dev), done=torch.zeros(n, dtype=torch.uint8, device=dev))
        sd = Side(capacity=cap, next_idx=0, ctr=1)
        for k, v in t.items():
            setattr(sd, k, v.data_ptr())
        sides.append((t, sd))
        keep.append(env)
    eps, logp = torch.empty(2 * n, device=dev), torch.empty(n, device=dev)
    ws = ops._ws(dev, 0, 'mpg_policy_sample_squashed_workspace_bytes', cfg, n) if squashed else None
    lib, s, c = L.lib(), L.stream(), ctypes.byref(cfg)
    fp = lambda f: ctypes.cast(f, ctypes.c_void_p)
    host = host_loops()

    def chain(reps):
        if squashed:
            assert host.bench_chain_sample(fp(lib.mpg_normal_fill), fp(lib.mpg_policy_sample_squashed), fp(lib.mpg_env_step_store_reset), c,
                                           L.ptr(pol), I(n), I(iters), L.ptr(eps), L.ptr(logp), *ws, ctypes.byref(sides[0][1]), s, I(reps)) == 0
        else:
            assert host.bench_chain_sample_step(fp(lib.mpg_worker_sample_step), c, L.ptr(pol), I(n), I(iters), ctypes.byref(sides[0][1]), s,
                                                I(reps)) == 0

    def launch(reps):
        assert host.bench_launch_sample(fp(lib.mpg_worker_sample_rollout), c, L.ptr(pol), I(n), I(iters), ctypes.byref(sides[1][1]), s,
                                        I(reps)) == 0
    chain(WARMUP), launch(WARMUP)
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(REGIONS):                                      # alternating: both see the same machine
        ta.append(timed(chain, batched=True))
        tb.append(timed(launch, batched=True))
    torch.cuda.synchronize()
    for k in sides[0][0]:                                         # the two did the same work: bit-identical at the end
        a, b = sides[0][0][k], sides[1][0][k]
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), k
    del keep, wc
    return statistics.median(ta), statistics.median(tb), (min(ta), max(ta)), (min(tb), max(tb))


def worker_sample_stochastic(out):
    """(d): OffPolicyWorker.sample() of the SAC stacks on PathTracking-v0 at the reference's worker defaults (8 agents, 64 iterations) on
    the loop and with one_launch_sample - host time included: the loop's launches are enqueued from Python, as a training run that
    does not take the native step enqueues them"""
    import torch
    from mpg_amd.config import default_args
    from mpg_amd.optimizer import quiesce_gc
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    print('\n| OffPolicyWorker.sample(), SAC, PathTracking-v0, num_agent 8, batch_size 512 | ms per sample |\n|---|---|', flush=True)
    for head, kw in (('Gaussian head', {}), ('squashed head', dict(squashed_head=True, action_range=STOCHASTIC_RANGE))):
        workers = []
        for one in (False, True):
            args = default_args('SAC', nan_check_interval=10 ** 9, **kw, **(dict(one_launch_sample=True) if one else {}))
            assert (args.env_id, args.num_agent, args.batch_size) == ('PathTracking-v0', 8, 512)
            workers.append(OffPolicyWorker(PolicyWithQs, args.env_id, args, 0))
        quiesce_gc()
        for w in workers:
            for _ in range(WARMUP):
                w.sample()
        torch.cuda.synchronize()
        t = [[], []]
        for _ in range(REGIONS):
            for k, w in enumerate(workers):
                t[k].append(timed(w.sample, SAMPLE_REPS))
        for a, b in zip(workers[0].sample(), workers[1].sample()):    # the two did the same work: bit-identical at the end
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
        for form, x in zip(('the loop (four launches per iteration)', 'one_launch_sample'), t):
            out['worker_sample'].append(dict(head=head, form=form, sample_ms=statistics.median(x), sample_range=(min(x), max(x))))
            print('| %s, %s | %.4f (%.4f .. %.4f) |' % (head, form, statistics.median(x), min(x), max(x)), flush=True)


def stack_sac(auto, chain=False):
    """SAC at the reference's worker defaults under the native step (fixed temperature, or the learned one)"""
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import SACLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    args = default_args('SAC', nan_check_interval=10 ** 9, **(dict(alpha='auto', target_entropy=-2.) if auto else {}))
    assert (args.num_agent, args.batch_size, args.replay_batch_size) == (8, 512, 256)
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    opt = SingleProcessOffPolicyOptimizer(worker, SACLearner(PolicyWithQs, args), ReplayBuffer(args, 0), None, args, sampling_interval=10,
                                          native_sac=True)
    assert opt._fused is not None and opt._fused.c.sample_iters == 64
    if chain:
        opt._fused.c.sample_iters = -64           # include/mpg_hip.h: the same iterations, one mpg_worker_sample_step each
    return opt


def step_cases_sac(out):
    import torch
    from mpg_amd.optimizer import quiesce_gc
    cases = [(auto, chain) for auto in (False, True) for chain in (True, False)]
    opts = [stack_sac(auto, chain) for auto, chain in cases]
    quiesce_gc()
    for _ in range(40):
        for o in opts:
            o.step()
    torch.cuda.synchronize()
    t = [[] for _ in opts]
    for _ in range(REGIONS):                                      # alternating; REPS a multiple of the sampling interval
        for k, o in enumerate(opts):
            t[k].append(timed(o.step, REPS))
    print('\n| native SAC step, num_agent 8, batch_size 512, sampling_interval 10, B = 256 | ms per step |\n|---|---|', flush=True)
    for (auto, chain), x in zip(cases, t):
        alg = "SAC, alpha = 'auto'" if auto else 'SAC, fixed alpha'
        form = 'chain kept (sample_iters = -64)' if chain else "the driver's own choice"
        out['step'].append(dict(alg=alg, form=form, step_ms=statistics.median(x), step_range=(min(x), max(x))))
        print('| %s, %s | %.4f (%.4f .. %.4f) |' % (alg, form, statistics.median(x), min(x), max(x)), flush=True)


def stack_pendulum(chain=False):
    """NADP at the pendulum parser's defaults: one agent, 512 iterations per sample, B = 256"""
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import NADPLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    args = default_args('NADP', nan_check_interval=10 ** 9)
    assert (args.env_id, args.num_agent, args.batch_size, args.replay_batch_size) == ('InvertedPendulumConti-v0', 1, 512, 256)
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    opt = SingleProcessOffPolicyOptimizer(worker, NADPLearner(PolicyWithQs, args), ReplayBuffer(args, 0), None, args, sampling_interval=10)
    assert opt._fused is not None and opt._fused.c.sample_iters == 512
    if chain:
        opt._fused.c.sample_iters = -512          # include/mpg_hip.h: the same iterations, two launches each
    return opt


def step_cases_pendulum(out, ab):
    import torch
    from mpg_amd.optimizer import quiesce_gc
    cases = (True, False) if ab else (False,)
    opts = [stack_pendulum(chain) for chain in cases]
    quiesce_gc()
    for _ in range(40):
        for o in opts:
            o.step()
    torch.cuda.synchronize()
    t = [[] for _ in opts]
    for _ in range(REGIONS):                                      # alternating; REPS a multiple of the sampling interval
        for k, o in enumerate(opts):
            t[k].append(timed(o.step, REPS))
    print('\n| native NADP step, InvertedPendulumConti-v0, num_agent 1, batch_size 512, sampling_interval 10, B = 256 | ms per step |\n|---|---|',
          flush=True)
    for chain, x in zip(cases, t):
        form = ('chain kept (sample_iters < 0)' if chain else "the driver's own choice") if ab else 'as built'
        out['step'].append(dict(alg='NADP', form=form, step_ms=statistics.median(x), step_range=(min(x), max(x))))
        print('| NADP, %s | %.4f (%.4f .. %.4f) |' % (form, statistics.median(x), min(x), max(x)), flush=True)


def stack(alg, chain=False):
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import MPGLearner, TD3Learner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    args = default_args(alg, nan_check_interval=10 ** 9)
    assert (args.num_agent, args.batch_size, args.replay_batch_size) == (8, 512, 256)
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    learner = (TD3Learner if alg == 'TD3' else MPGLearner)(PolicyWithQs, args)
    opt = SingleProcessOffPolicyOptimizer(worker, learner, ReplayBuffer(args, 0), None, args, sampling_interval=10)
    assert opt._fused is not None and opt._fused.c.sample_iters == 64
    if chain:
        opt._fused.c.sample_iters = -64           # include/mpg_hip.h: the same iterations, one mpg_worker_step each
    return opt


def step_cases(out, ab):
    import torch
    from mpg_amd.optimizer import quiesce_gc
    cases = [(a, chain) for a in ('TD3', 'MPG-v2') for chain in ((True, False) if ab else (False,))]
    opts = [stack(a, chain) for a, chain in cases]
    quiesce_gc()
    for _ in range(40):
        for o in opts:
            o.step()
    torch.cuda.synchronize()
    t = [[] for _ in opts]
    for _ in range(REGIONS):                                      # alternating; REPS a multiple of the sampling interval
        for k, o in enumerate(opts):
            t[k].append(timed(o.step, REPS))
    print('\n| native step, num_agent 8, batch_size 512, sampling_interval 10, B = 256 | ms per step |\n|---|---|', flush=True)
    for (a, chain), x in zip(cases, t):
        form = ('chain kept (sample_iters < 0)' if chain else "the driver's own choice") if ab else 'as built'
        out['step'].append(dict(alg=a, form=form, step_ms=statistics.median(x), step_range=(min(x), max(x))))
        print('| %s, %s | %.4f (%.4f .. %.4f) |' % (a, form, statistics.median(x), min(x), max(x)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--steps-only', action='store_true', help='the native step times alone')
    ap.add_argument('--env', default='path_tracking', choices=('path_tracking', 'pendulum', 'model'),
                    help='pendulum: mpg_worker_rollout_pendulum against its chain, and the native NADP step at the pendulum defaults; '
                         'model: mpg_worker_rollout_model against its chain on the model-backed InvertedDoublePendulum-v2 env')
    ap.add_argument('--stochastic', action='store_true',
                    help='the stochastic (SAC) policy: mpg_worker_sample_rollout on PathTracking-v0 (both heads; with --steps-only the native '
                         'SAC step alone), or with --env pendulum mpg_worker_sample_rollout_pendulum (the tanh-squashed Gaussian policy), '
                         'each against its chain, and OffPolicyWorker.sample() both ways')
    ap.add_argument('--tree', default=None, help="another checkout of this project whose build is timed (with --steps-only)")
    a = ap.parse_args()
    assert not a.tree or a.steps_only, '--tree times the native steps of another checkout: pass --steps-only'
    assert not (a.stochastic and a.env == 'pendulum' and a.steps_only), '--stochastic --env pendulum has no native step to time'
    assert not (a.stochastic and a.tree), '--tree times the deterministic learners\' native steps'
    assert not (a.env == 'model' and (a.stochastic or a.steps_only or a.tree)), \
        '--env model times the deterministic sample alone: the launch is taken on request and the native step does not serve this env'
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else os.path.dirname(HERE))
    import torch
    assert torch.cuda.is_available(), 'bench_worker_rollout.py needs a GPU: nothing here is measured without one'
    out = {'sample': [], 'step': []}
    if a.env == 'model':
        print('| agents | iters | explore_sigma | (a) chain of mpg_policy_action + mpg_model_env_step_store_reset, ms | '
              '(b) mpg_worker_rollout_model, ms | (a) / (b) | done rows in the ring |\n|---|---|---|---|---|---|---|', flush=True)
        for n, iters, sigma in MODEL_CASES:
            ma, mb, ra, rb, fell, cap = sample_case_model(n, iters, sigma)
            out['sample'].append(dict(agents=n, iters=iters, explore_sigma=sigma, chain_ms=ma, chain_range=ra, launch_ms=mb,
                                      launch_range=rb, done_rows=fell, ring_rows=cap))
            print('| %d | %d | %g | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) | %.2f | %d of %d |'
                  % (n, iters, sigma, ma, ra[0], ra[1], mb, rb[0], rb[1], ma / mb, fell, cap), flush=True)
    elif a.stochastic and a.env != 'pendulum':
        if not a.steps_only:
            out['worker_sample'] = []
            print('| head | agents | iters | obs_dim | (a) chain, ms | (b) mpg_worker_sample_rollout, ms | (a) / (b) |\n|---|---|---|---|---|---|---|',
                  flush=True)
            for squashed in (False, True):
                head = 'squashed: mpg_normal_fill + mpg_policy_sample_squashed + mpg_env_step_store_reset' if squashed else \
                    'Gaussian: mpg_worker_sample_step'
                for n, iters, od in CASES:
                    ma, mb, ra, rb = sample_case_stochastic(n, iters, od, squashed)
                    out['sample'].append(dict(head=head, agents=n, iters=iters, obs_dim=od, chain_ms=ma, chain_range=ra, launch_ms=mb,
                                              launch_range=rb))
                    print('| %s | %d | %d | %d | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) | %.2f |'
                          % (head, n, iters, od, ma, ra[0], ra[1], mb, rb[0], rb[1], ma / mb), flush=True)
            worker_sample_stochastic(out)
        step_cases_sac(out)
    elif a.stochastic:
        out['worker_sample'] = []
        print('| agents | iters | (a) chain of mpg_normal_fill + mpg_policy_sample_squashed + mpg_env_step_store_reset, ms | '
              '(b) mpg_worker_sample_rollout_pendulum, ms | (a) / (b) | done rows in the ring |\n|---|---|---|---|---|---|', flush=True)
        for n, iters in STOCHASTIC_CASES:
            ma, mb, ra, rb, fell, cap = sample_case_stochastic_pendulum(n, iters)
            out['sample'].append(dict(agents=n, iters=iters, chain_ms=ma, chain_range=ra, launch_ms=mb, launch_range=rb, done_rows=fell,
                                      ring_rows=cap))
            print('| %d | %d | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) | %.2f | %d of %d |'
                  % (n, iters, ma, ra[0], ra[1], mb, rb[0], rb[1], ma / mb, fell, cap), flush=True)
        worker_sample_stochastic_pendulum(out)
    elif a.env == 'pendulum':
        if not a.steps_only:
            print('| agents | iters | explore_sigma | (a) chain of mpg_policy_action + mpg_env_step_store_reset, ms | '
                  '(b) mpg_worker_rollout_pendulum, ms | (a) / (b) | done rows in the ring |\n|---|---|---|---|---|---|---|', flush=True)
            for n, iters, sigma in PENDULUM_CASES:
                ma, mb, ra, rb, fell, cap = sample_case_pendulum(n, iters, sigma)
                out['sample'].append(dict(agents=n, iters=iters, explore_sigma=sigma, chain_ms=ma, chain_range=ra, launch_ms=mb,
                                          launch_range=rb, done_rows=fell, ring_rows=cap))
                print('| %d | %d | %g | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) | %.2f | %d of %d |'
                      % (n, iters, sigma, ma, ra[0], ra[1], mb, rb[0], rb[1], ma / mb, fell, cap), flush=True)
        step_cases_pendulum(out, ab=not a.tree)
    elif not a.steps_only:
        print('| agents | iters | obs_dim | (a) chain of mpg_worker_step, ms | (b) mpg_worker_rollout, ms | (a) / (b) |\n|---|---|---|---|---|---|', flush=True)
        for n, iters, od in CASES:
            ma, mb, ra, rb = sample_case(n, iters, od)
            out['sample'].append(dict(agents=n, iters=iters, obs_dim=od, chain_ms=ma, chain_range=ra, launch_ms=mb, launch_range=rb))
            print('| %d | %d | %d | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) | %.2f |' % (n, iters, od, ma, ra[0], ra[1], mb, rb[0], rb[1], ma / mb),
                  flush=True)
    if a.env == 'path_tracking' and not a.stochastic:
        step_cases(out, ab=not a.tree)       # (another checkout may not know the chain-kept form)
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
