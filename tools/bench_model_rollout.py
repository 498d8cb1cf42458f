#!/usr/bin/env python3
"""Times of a policy's closed loop on the differentiable model, one process: the chain of stand-alone launches - per step
mpg_policy_action (sigma 0) and mpg_model_step, 2 * steps launches, enqueued through ctypes with every argument prepared beforehand -
against mpg_model_rollout, the same computation as ONE launch (bit-identical: tests/test_model_rollout_gpu.py; asserted here too, on
the timed buffers after the last region).  Medians of REGIONS timed regions of REPS calls after WARMUP warm-up calls, device events
around a region, the two forms alternating region by region, the range in brackets.  The feature has no earlier number: the chain in
the same run is the comparison, and no bar is fixed in advance.

Cases: 5 trajectories x 200 steps (PathTracking, the evaluator's defaults), 1 x 500 (pendulum), 50 x 200 (PathTracking) and 256 x 25
(double pendulum: a batch's rollouts); both weight forms (packed image / strided).

    python tools/bench_model_rollout.py [--json out.json]       prints a markdown table
    python tools/bench_model_rollout.py --gap [--env ENV] [--checkpoint DIR --iteration N]
        prints ModelEvaluator.gap_to_env - per step the mean absolute difference of every observation column and of the reward between
        the env's closed loop and the model's, and the two mean returns - for a fresh policy or a saved one"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpg_amd import _lib as L                                # noqa: E402
from mpg_amd import ops                                      # noqa: E402
from tests.golden_inputs import mlp_weights_flat, reset_law_obs   # noqa: E402

REGIONS, REPS, WARMUP = 7, 200, 40
PT, PEND, DPEND = 'PathTracking-v0', 'InvertedPendulumConti-v0', 'InvertedDoublePendulum-v2'
CASES = ((PT, 5, 200), (PEND, 1, 500), (PT, 50, 200), (DPEND, 256, 25))
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


def start_rows(rng, env_id, n):
    if env_id == PT:
        return reset_law_obs(rng, n)
    if env_id == PEND:
        return (rng.uniform(-0.1, 0.1, (n, 4))).astype(np.float32)
    th = rng.uniform(-0.1, 0.1, (n, 2))
    return np.concatenate([rng.uniform(-0.1, 0.1, (n, 1)), np.sin(th), np.cos(th), 0.1 * rng.standard_normal((n, 6))], 1).astype(np.float32)


def rollout_case(env_id, n, steps, cache):
    rng = np.random.Generator(np.random.PCG64(n + steps + int(cache)))
    dev = 'cuda'
    cfg = ops.make_cfg(env_id)
    od, ad = cfg.obs_dim, cfg.act_dim
    pol = torch.as_tensor(mlp_weights_flat(rng, od, 2 * ad)).to(dev)
    wc = None
    if cache:
        wc = ops.WeightCache(pol, [(od, 2 * ad)])
        cfg.wcache[0] = wc.pointer
    f = dict(dtype=torch.float32, device=dev)
    obs0 = torch.as_tensor(start_rows(rng, env_id, n)).to(dev)
    eps = torch.as_tensor(rng.standard_normal((steps, n)).astype(np.float32)).to(dev)
    # the chain: the policy reads obs_a[t], the model writes obs_a[t + 1] - the trajectory needs no copy
    obs_a, act_a, rew_a = torch.empty(steps + 1, n, od, **f), torch.empty(steps, n, ad, **f), torch.empty(steps, n, **f)
    obs_a[0].copy_(obs0)
    obst_b, act_b, rew_b, last_b = torch.empty(steps, n, od, **f), torch.empty(steps, n, ad, **f), torch.empty(steps, n, **f), torch.empty(n, od, **f)
    lib, s, c, p = L.lib(), L.stream(), ctypes.byref(cfg), L.ptr
    zero, z64 = ctypes.c_float(0.), ctypes.c_uint64(0)
    pa = [(c, p(pol), I(n), p(obs_a[t]), zero, z64, z64, p(act_a[t]), s) for t in range(steps)]
    ma = [(c, I(n), p(obs_a[t]), p(act_a[t]), p(eps[t]), p(obs_a[t + 1]), p(rew_a[t]), s) for t in range(steps)]
    policy_action, model_step, model_rollout = lib.mpg_policy_action, lib.mpg_model_step, lib.mpg_model_rollout
    la = (c, p(pol), I(n), I(steps), p(obs0), p(eps), p(obst_b), p(act_b), p(rew_b), p(last_b), s)

    def chain():
        for t in range(steps):
            assert policy_action(*pa[t]) == 0 and model_step(*ma[t]) == 0

    def launch():
        assert model_rollout(*la) == 0

    for k in range(WARMUP):
        (chain if k % 2 == 0 else launch)()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(REGIONS):                                  # alternating: both see the same machine
        ta.append(timed(chain, REPS))
        tb.append(timed(launch, REPS))
    b32 = lambda x: x.contiguous().view(torch.int32)
    for x, y in ((obs_a[:steps], obst_b), (act_a, act_b), (rew_a, rew_b), (obs_a[steps], last_b)):
        assert torch.equal(b32(x), b32(y))
    del wc
    return statistics.median(ta), statistics.median(tb), (min(ta), max(ta)), (min(tb), max(tb))


def print_gap(env_id, checkpoint, iteration, steps):
    from mpg_amd.config import default_args
    from mpg_amd.evaluator import ModelEvaluator
    from mpg_amd.policy import PolicyWithQs
    args = default_args('MPG-v2', env_id=env_id, fixed_steps=steps)
    ev = ModelEvaluator(PolicyWithQs, env_id, args)
    if checkpoint:
        ev.policy_with_value.load_weights(checkpoint, iteration)
    gap = ev.gap_to_env()
    cols = ('v_x', 'v_y', 'r', 'delta_y', 'delta_phi', 'x') if env_id == PT else ('p', 'theta', 'pdot', 'thetadot')
    print('%s, %s policy, %d episodes x %d steps, model noise at its mean' % (env_id, 'saved' if checkpoint else 'fresh', ev.num_eval_agent, steps))
    print('| step | ' + ' | '.join(cols) + ' | reward |\n|---|' + '---|' * (len(cols) + 1))
    for t in sorted(set([0, 1, 2, 5, 10, 25, 50, 100, steps - 1])):
        if t < steps:
            print('| %d | %s | %.4g |' % (t, ' | '.join('%.4g' % v for v in gap['obs_gap'][t].tolist()), float(gap['rew_gap'][t])))
    print('mean return: env %.4f, model %.4f' % (gap['env_return'], gap['model_return']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--gap', action='store_true')
    ap.add_argument('--env', default=PT, choices=(PT, PEND))
    ap.add_argument('--checkpoint', default=None)
    ap.add_argument('--iteration', type=int, default=0)
    ap.add_argument('--steps', type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_model_rollout.py needs a GPU: nothing here is measured without one'
    if a.gap:
        return print_gap(a.env, a.checkpoint, a.iteration, a.steps)
    out = []
    print('| model | trajectories x steps | W2 | chain, launches | chain, ms | one launch, ms | chain / launch |\n|---|---|---|---|---|---|---|', flush=True)
    for env_id, n, steps in CASES:
        for cache in (True, False):
            ma, mb, ra, rb = rollout_case(env_id, n, steps, cache)
            form = 'packed' if cache else 'strided'
            out.append(dict(env=env_id, n=n, steps=steps, weights=form, chain_ms=ma, chain_range=ra, launch_ms=mb, launch_range=rb))
            print('| %s | %d x %d | %s | %d | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) | %.1f |'
                  % (env_id, n, steps, form, 2 * steps, ma, ra[0], ra[1], mb, rb[0], rb[1], ma / mb), flush=True)
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
