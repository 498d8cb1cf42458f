#!/usr/bin/env python3
"""Times of an evaluation's episodes, one process, medians of REGIONS timed regions after a warm-up, the two forms alternating region
by region:

  (a) device events around REPS back-to-back evaluations, a synchronise at the end of every region:
      the chain of stand-alone launches - per step mpg_policy_action (sigma 0) and mpg_env_step, 2 * steps launches, enqueued from
      Python through ctypes with every argument prepared beforehand (the evaluator's own loop also allocates three tensors per step) -
      against mpg_eval_rollout / mpg_eval_rollout_pendulum, the same computation as ONE launch (bit-identical:
      tests/test_eval_rollout_gpu.py; asserted here too, on the timed buffers after the last region, both done flags included).  Both start every evaluation from the same state (two
      small device copies in front of each, in both forms).  PathTracking 5 x 200 and 50 x 200 (the two num_eval_agent values the
      parsers use), the pendulum 1 x 100, 5 x 100 and 1 x 500; both weight forms (packed image / strided).
  (b) wall time of one Evaluator.run_evaluation, host-inclusive (a synchronise at its end), with and without args.one_launch_eval, at
      the MPG-v2 PathTracking defaults (5 agents x 200 steps) and at the pendulum NADP defaults (num_eval_agent 1, num_eval_episode 5,
      fixed_steps 100).  Without the flag run_evaluation is the parent commit's method path, which on the pendulum runs ONE episode
      where the flag runs the reference's five.

    python tools/bench_eval.py [--json out.json]          prints markdown tables"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpg_amd import _lib as L                                # noqa: E402
from mpg_amd import ops                                      # noqa: E402
from tests.golden_inputs import mlp_weights_flat             # noqa: E402

REGIONS, REPS, WARMUP = 5, 5, 2
PT, PEND = 'PathTracking-v0', 'InvertedPendulumConti-v0'
I = ctypes.c_int


def timed(fn, reps):
    """ms per call of one region: device events around `reps` calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def rollout_case(env_id, n, steps, cache):
    rng = np.random.Generator(np.random.PCG64(n + steps + int(cache)))
    dev = 'cuda'
    cfg = ops.make_cfg(env_id)
    od, ad, kind = cfg.obs_dim, cfg.act_dim, cfg.env_kind
    pol = torch.as_tensor(mlp_weights_flat(rng, od, 2 * ad)).to(dev)
    wc = None
    if cache:
        wc = ops.WeightCache(pol, [(od, 2 * ad)])
        cfg.wcache[0] = wc.pointer
    state0, obs0 = torch.zeros(8, n, device=dev), torch.empty(n, od, device=dev)
    L.call('mpg_env_reset', I(kind), I(n), I(od), L.ptr(state0), L.ptr(None), L.c_u64(424242), L.c_u64(0), L.ptr(obs0), L.stream())
    f = dict(dtype=torch.float32, device=dev)
    u8 = dict(dtype=torch.uint8, device=dev)
    # the chain: policy reads obs_a[t], the env writes obs_a[t + 1] - the trajectory needs no copy
    state_a, obs_a, act_a, rew_a = torch.empty(8, n, **f), torch.empty(steps + 1, n, od, **f), torch.empty(steps, n, ad, **f), torch.empty(steps, n, **f)
    done_a, di_a = torch.empty(n, **u8), torch.empty(n, **u8)
    state_b, obs_b, obst_b, act_b, rew_b = torch.empty(8, n, **f), torch.empty(n, od, **f), torch.empty(steps, n, od, **f), torch.empty(steps, n, ad, **f), torch.empty(steps, n, **f)
    done_b, di_b = torch.empty(n, **u8), torch.empty(n, **u8)
    lib, s, c, p = L.lib(), L.stream(), ctypes.byref(cfg), L.ptr
    zero, z64 = ctypes.c_float(0.), ctypes.c_uint64(0)
    pa = [(c, p(pol), I(n), p(obs_a[t]), zero, z64, z64, p(act_a[t]), s) for t in range(steps)]
    ea = [(I(kind), I(n), I(od), p(state_a), p(act_a[t]), p(obs_a[t + 1]), p(rew_a[t]), p(done_a), p(di_a), s) for t in range(steps)]
    policy_action, env_step = lib.mpg_policy_action, lib.mpg_env_step
    if kind == 0:
        entry, tail = lib.mpg_eval_rollout, (p(done_b), p(di_b), s)
    else:
        entry, tail = lib.mpg_eval_rollout_pendulum, (p(done_b), s)
    la = (c, p(pol), I(n), I(steps), p(state_b), p(obs_b), p(obst_b), p(act_b), p(rew_b)) + tail

    def chain():
        state_a.copy_(state0)
        obs_a[0].copy_(obs0)
        for t in range(steps):
            assert policy_action(*pa[t]) == 0 and env_step(*ea[t]) == 0

    def launch():
        state_b.copy_(state0)
        obs_b.copy_(obs0)
        assert entry(*la) == 0

    for _ in range(WARMUP):
        chain(), launch()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(REGIONS):                                  # alternating: both see the same machine
        ta.append(timed(chain, REPS))
        tb.append(timed(launch, REPS))
    # what the last timed evaluation of each form left: bit-identical
    b32 = lambda x: x.contiguous().view(torch.int32)
    for x, y in ((obs_a[:steps], obst_b), (act_a, act_b), (rew_a, rew_b), (obs_a[steps], obs_b), (state_a, state_b)):
        assert torch.equal(b32(x), b32(y))
    assert torch.equal(done_a, done_b)
    if kind == 0:                                             # (the pendulum's launch has no second flag: its step writes `done` into both)
        assert torch.equal(di_a, di_b)
    else:
        assert torch.equal(di_a, done_b)
    del wc
    return statistics.median(ta), statistics.median(tb), (min(ta), max(ta)), (min(tb), max(tb))


def evaluation_case(alg, **kw):
    """(median, range) of the wall time of one run_evaluation in ms, without and with the flag, alternating"""
    from mpg_amd.config import default_args
    from mpg_amd.evaluator import Evaluator
    from mpg_amd.policy import PolicyWithQs
    evs = []
    for flag in (False, True):
        args = default_args(alg, one_launch_eval=flag, **kw)
        evs.append(Evaluator(PolicyWithQs, args.env_id, args))

    def wall(ev):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.run_evaluation(0)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    for _ in range(WARMUP):
        [wall(ev) for ev in evs]
    t = [[], []]
    for _ in range(REGIONS):
        for k, ev in enumerate(evs):
            t[k].append(wall(ev))
    return [(statistics.median(x), (min(x), max(x))) for x in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_eval.py needs a GPU: nothing here is measured without one'
    out = {'rollout': [], 'evaluation': []}
    print('| env | agents x steps | W2 | (a) chain, launches | chain, ms | one launch, ms | chain / launch |\n|---|---|---|---|---|---|---|', flush=True)
    for env_id, n, steps in ((PT, 5, 200), (PT, 50, 200), (PEND, 1, 100), (PEND, 5, 100), (PEND, 1, 500)):
        for cache in (True, False):
            ma, mb, ra, rb = rollout_case(env_id, n, steps, cache)
            form = 'packed' if cache else 'strided'
            out['rollout'].append(dict(env=env_id, n=n, steps=steps, weights=form, chain_ms=ma, chain_range=ra, launch_ms=mb, launch_range=rb))
            print('| %s | %d x %d | %s | %d | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) | %.1f |'
                  % (env_id, n, steps, form, 2 * steps, ma, ra[0], ra[1], mb, rb[0], rb[1], ma / mb), flush=True)
    print('\n| run_evaluation, wall ms | method path (2 * fixed_steps launches, ~20 torch ops, a sync per metric) | one_launch_eval (1 + 1 launches, one copy) |'
          '\n|---|---|---|', flush=True)
    for name, alg, kw in (('MPG-v2 PathTracking defaults: 5 agents x 200 steps', 'MPG-v2', dict(num_eval_agent=5, fixed_steps=200)),
                          ('pendulum NADP defaults: 1 agent, 5 episodes x 100 steps (the method path runs ONE episode)', 'NADP',
                           dict(num_eval_agent=1, num_eval_episode=5, fixed_steps=100))):
        (m0, r0), (m1, r1) = evaluation_case(alg, **kw)
        out['evaluation'].append(dict(case=name, method_ms=m0, method_range=r0, one_launch_ms=m1, one_launch_range=r1))
        print('| %s | %.2f (%.2f .. %.2f) | %.2f (%.2f .. %.2f) |' % (name, m0, r0[0], r0[1], m1, r1[0], r1[1]), flush=True)
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
