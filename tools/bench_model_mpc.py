#!/usr/bin/env python3
"""Times of MPC on the learners' own models (mpg_model_mpc_solve) on the device, one process, medians of REGIONS timed regions after a
warm-up, with the range - tools/bench_mpc.py's form:

  (a) one solve per model at horizon 25 and 200 iterations from zeros, tol 0, for 1, 256 and 64 x (CU count) rows of the model's start law:
      device events around REPS back-to-back solves, a synchronise at the end of every region;
  --caps: (b) one solve per model at horizon 31 with every CU busy (rows = 64 x CU count), tol 0, CAP_ITERS iterations: ms per iteration
      and the largest round iteration count whose launch stays under 0.35 s - what MPG_MODEL_MPC_MAX_ITERS_* in include/mpg_hip.h are
      set from (at most MPG_MPC_MAX_ITERS);
  --gap: (c) ModelEvaluator.gap_to_mpc on the double pendulum's model, 64 reset-law rows, horizon 25, for a fresh AMPC policy and for
      the same stack after --iters optimizer steps of tools/train_model_env.py's loop (its objects, its settings).  A measurement: no
      threshold is attached.

    python tools/bench_model_mpc.py [--caps | --gap [--iters 3000]] [--json out.json]      prints markdown tables"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpg_amd import mpc as M                                 # noqa: E402
from mpg_amd import ops                                      # noqa: E402

REGIONS, WARMUP = 7, 2
HORIZON, ITERS = 25, 200
CAP_HORIZON, CAP_ITERS, CAP_SECONDS = 31, 100, 0.35
MODELS = (('PathTracking-v0', 0), ('InvertedPendulumConti-v0', 1), ('InvertedDoublePendulum-v2', 2))


def start_rows(env_id, n):
    """the models' start laws (PathTrackingEnv.reset's; the pendulum's wide law; the double pendulum's U(-0.1, 0.1) and 0.1 N(0, 1))"""
    rng = np.random.default_rng(0)
    if env_id == MODELS[0][0]:
        vx = rng.uniform(15, 25, n)
        x = np.stack([vx - 20., vx * np.tan(rng.normal(0, 0.15, n)), rng.normal(0, 0.3, n), rng.normal(0, 1, n), rng.normal(0, np.pi / 9, n),
                      rng.uniform(0, 600, n)], 1)
    elif env_id == MODELS[1][0]:
        x = np.stack([rng.uniform(-1, 1, n), rng.uniform(-np.pi, np.pi, n), rng.uniform(-1, 1, n), rng.uniform(-3, 3, n)], 1)
    else:
        th = rng.uniform(-0.1, 0.1, (n, 2))
        x = np.concatenate([rng.uniform(-0.1, 0.1, (n, 1)), np.sin(th), np.cos(th), 0.1 * rng.standard_normal((n, 3)), np.zeros((n, 3))], 1)
    return torch.as_tensor(x, dtype=torch.float32).to('cuda')


def solve_case(env_id, rows, horizon, iters, reps):
    cfg = ops.make_cfg(env_id)
    obs0 = start_rows(env_id, rows)
    zeros = torch.zeros(rows, horizon, cfg.act_dim, device='cuda')
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(WARMUP):
        out = M.model_mpc_solve(cfg, obs0, zeros, iters)
    torch.cuda.synchronize()
    t = []
    for _ in range(REGIONS):
        e0.record()
        for _ in range(reps):
            out = M.model_mpc_solve(cfg, obs0, zeros, iters)
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1) / reps)
    info = out[3]
    return statistics.median(t), (min(t), max(t)), float(info.abs().float().mean()), int((info < 0).sum())


def round_down(n):
    """the largest 'round' number <= n: one or two leading digits of 1, 1.5, 2, 2.5, 3, 4, 5, 6, 8"""
    if n < 10:
        return max(int(n), 1)
    mag = 10 ** (len(str(int(n))) - 1)
    return max(int(c * mag) for c in (1, 1.5, 2, 2.5, 3, 4, 5, 6, 8) if c * mag <= n)


def caps(a):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = 64 * cus
    out = {'caps': []}
    print('| model | rows (64 x %d CUs) | one solve, horizon %d, %d iterations, tol 0: ms | ms per iteration | iterations in %.2f s | cap |\n'
          '|---|---|---|---|---|---|' % (cus, CAP_HORIZON, CAP_ITERS, CAP_SECONDS), flush=True)
    for env_id, _ in MODELS:
        m, r, it, failed = solve_case(env_id, rows, CAP_HORIZON, CAP_ITERS, reps=1)
        # (rows whose search failed early ran fewer iterations: the launch's time is the slowest wave's, which ran them all unless
        # every row of every wave failed)
        per = m / CAP_ITERS
        fit = int(1e3 * CAP_SECONDS / per)
        cap = min(round_down(fit), M.MAX_ITERS)
        out['caps'].append(dict(env=env_id, rows=rows, ms=m, range=r, ms_per_iteration=per, fits=fit, cap=cap, mean_abs_info=it, failed=failed))
        print('| %s | %d | %.2f (%.2f .. %.2f) | %.4f | %d | %d |' % (env_id, rows, m, r[0], r[1], per, fit, cap), flush=True)
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


def gap(a):
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.envs import make_model_env
    from mpg_amd.evaluator import ModelEvaluator
    from mpg_amd.learners import AMPCLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    env_id = MODELS[2][0]
    # tools/train_model_env.py's objects for --alg AMPC
    args = default_args('AMPC', env_id=env_id, env_on_model=True, one_launch_sample=True, seed=0, init_seed=0, fixed_steps=200,
                        num_rollout_list_for_policy_update=[25])
    worker = OffPolicyWorker(PolicyWithQs, env_id, args, 0)
    learner = AMPCLearner(PolicyWithQs, args)
    evaluator = ModelEvaluator(PolicyWithQs, env_id, args)
    opt = SingleProcessOffPolicyOptimizer(worker, learner, ReplayBuffer(args, 0), evaluator, args, sampling_interval=10)
    evaluator.share_policy(worker.policy_with_value)
    starts = make_model_env(env_id, num_agent=64, seed=424242).reset()
    out = {'gap': []}
    print('| policy | rows | horizon | mean policy cost | mean MPC cost | mean gap | largest gap | rows the solve from the policy\'s actions won |\n'
          '|---|---|---|---|---|---|---|---|', flush=True)
    for name, steps in (('fresh', 0), ('after %d AMPC iterations' % a.iters, a.iters)):
        for _ in range(steps):
            opt.step()
        g = evaluator.gap_to_mpc(starts, horizon=HORIZON, iters=ITERS)
        row = dict(policy=name, rows=64, horizon=HORIZON, policy_cost=g['mean_policy_cost'], mpc_cost=g['mean_mpc_cost'], gap=g['mean_gap'],
                   max_gap=float(g['gap'].max()), from_policy_won=int(g['from_policy_won'].sum()))
        out['gap'].append(row)
        print('| %s | 64 | %d | %.4f | %.4f | %.4f | %.4f | %d |' % (name, HORIZON, row['policy_cost'], row['mpc_cost'], row['gap'], row['max_gap'],
                                                                  row['from_policy_won']), flush=True)
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--caps', action='store_true')
    ap.add_argument('--gap', action='store_true')
    ap.add_argument('--iters', type=int, default=3000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_model_mpc.py needs a GPU: nothing here is measured without one'
    if a.caps:
        return caps(a)
    if a.gap:
        return gap(a)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = {'solve': []}
    print('| model | rows | one solve (horizon %d, %d iterations), ms | per row, us | mean |info| | failed searches |\n|---|---|---|---|---|---|'
          % (HORIZON, ITERS), flush=True)
    for env_id, _ in MODELS:
        for rows in (1, 256, 64 * cus):
            m, r, it, failed = solve_case(env_id, rows, HORIZON, ITERS, reps=2)
            out['solve'].append(dict(env=env_id, rows=rows, ms=m, range=r, mean_abs_info=it, failed=failed))
            print('| %s | %d | %.3f (%.3f .. %.3f) | %.2f | %.1f | %d |' % (env_id, rows, m, r[0], r[1], 1e3 * m / rows, it, failed), flush=True)
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
