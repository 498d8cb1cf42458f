#!/usr/bin/env python3
"""Times of MPC on the learners' own models (mpg_model_mpc_solve) on the device, one process, medians of REGIONS timed regions after a
warm-up, with the range - tools/bench_mpc.py's form:

  (a) one solve per model at horizon 25 and 200 iterations from zeros, tol 0, for 1, 256 and 64 x (CU count) rows of the model's start law:
      device events around REPS back-to-back solves, a synchronise at the end of every region;
  --caps: (b) one solve per model at horizon 31 with every CU busy (rows = 64 x CU count), tol 0, CAP_ITERS iterations: ms per iteration
      and the largest round iteration count whose launch stays under 0.35 s - what MPG_MODEL_MPC_MAX_ITERS_* in include/mpg_hip.h are
      set from (at most MPG_MPC_MAX_ITERS);
      and (b') one mpg_model_mpc_rollout launch per model AT its work cap MPG_MODEL_MPC_ROLLOUT_MAX_WORK_* (steps * iters = the cap,
      at most CAP_ROLLOUT_ITERS iterations per solve), horizon 31, rows = 64 x CU count, tol 0, cold start: seconds of the entry point
      alone (buffers allocated before) against the 0.35 s; and the corner the cap does not count, as many steps as pass with 0, 1 and 2
      iterations per solve;
  --closed-loop: (d) run_model_mpc per model for 64 and 256 agents x 90 steps at horizon 25, 200 iterations, warm with tol = 1e-3 and cold
      with tol = 0: the loop form (two launches per step - the parent commit's run_model_mpc, which the default path still is bit for
      bit) against one_launch=True, wall time of the whole call between synchronisations; the accepted iterations per solve and the mean
      reward sum in both settings.  No ratio is fixed in advance;
  --gap: (c) ModelEvaluator.gap_to_mpc on the double pendulum's model, 64 reset-law rows, horizon 25, for a fresh AMPC policy and for
      the same stack after --iters optimizer steps of tools/train_model_env.py's loop (its objects, its settings).  A measurement: no
      threshold is attached.

    python tools/bench_model_mpc.py [--caps | --closed-loop | --gap [--iters 3000]] [--json out.json]
prints markdown tables"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpg_amd import mpc as M                                 # noqa: E402
from mpg_amd import ops                                      # noqa: E402

REGIONS, WARMUP = 7, 2
HORIZON, ITERS = 25, 200
CAP_HORIZON, CAP_ITERS, CAP_SECONDS = 31, 100, 0.35
CAP_ROLLOUT_ITERS = 128          # at most: the largest divisor of the work cap up to it (128 x 16 steps = 2048, 100 x 4 = 400)
LOOP_STEPS, LOOP_AGENTS = 90, (64, 256)
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


def rollout_launch_seconds(cfg, obs0, steps, horizon, iters, regions):
    """seconds of ONE mpg_model_mpc_rollout launch (tol 0, cold from zeros, eps NULL), the entry point alone between two device events:
    every buffer is allocated before, and the start rows are copied back into obs_io outside the timed region"""
    import ctypes
    from mpg_amd import _lib as L
    n, od, ad = obs0.shape[0], cfg.obs_dim, cfg.act_dim
    f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device='cuda')
    obs_io, u_io = obs0.clone(), torch.zeros(n, horizon, ad, device='cuda')
    obs_traj, plan_traj, rew, cost, pg = f(steps, n, od), f(steps, n, horizon, ad), f(steps, n), f(steps, n), f(steps, n)
    info = torch.empty(steps, n, dtype=torch.int32, device='cuda')
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = []
    for i in range(1 + regions):                 # one warm-up launch
        obs_io.copy_(obs0)
        e0.record()
        L.call('mpg_model_mpc_rollout', ctypes.byref(cfg), L.c_int(n), L.c_int(steps), L.c_int(horizon), L.c_int(iters), L.c_float(0.), L.c_int(0),
               L.ptr(obs_io), L.ptr(u_io), L.ptr(None), L.ptr(obs_traj), L.ptr(plan_traj), L.ptr(rew), L.ptr(cost), L.ptr(pg), L.ptr(info), L.stream())
        e1.record()
        e1.synchronize()
        if i >= 1:
            t.append(e0.elapsed_time(e1) / 1e3)
    return t


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
    # one closed-loop launch at each kind's work cap, and the corner the cap does not count: many steps of few iterations (every step's
    # solve has a setup forward and reverse pass, and the plant's step comes on top: about one iteration-equivalent per step)
    out['rollout_caps'] = []
    print('\n| model | rows | steps x iterations | steps * iters | one launch, horizon %d, tol 0, cold: s | ms per (iteration + 1 per step) '
          '| largest round work under %.2f s |\n|---|---|---|---|---|---|---|' % (CAP_HORIZON, CAP_SECONDS), flush=True)
    for env_id, kind in MODELS:
        cfg = ops.make_cfg(env_id)
        work = M.MODEL_MAX_ROLLOUT_WORK[kind]
        its = max(d for d in range(1, CAP_ROLLOUT_ITERS + 1) if work % d == 0)
        cases = [(work // its, its, REGIONS)] + [(min(M.MODEL_MAX_ROLLOUT_STEPS, work // k if k else work + M.MODEL_MAX_ROLLOUT_STEPS), k, 3)
                                                for k in (0, 1, 2)]
        obs0 = start_rows(env_id, rows)
        for steps, k, regions in cases:
            t = rollout_launch_seconds(cfg, obs0, steps, CAP_HORIZON, k, regions)
            m = statistics.median(t)
            at_cap = steps * k == work and k == its
            fit = int(work * CAP_SECONDS / m) if at_cap else None
            out['rollout_caps'].append(dict(env=env_id, rows=rows, steps=steps, iters=k, work=steps * k, seconds=m, range=(min(t), max(t)),
                                            ms_per_pass=1e3 * m / (steps * (k + 1)), fits=fit, round=round_down(fit) if fit else None))
            print('| %s | %d | %d x %d | %d | %.4f (%.4f .. %.4f) | %.4f | %s |'
                  % (env_id, rows, steps, k, steps * k, m, min(t), max(t), 1e3 * m / (steps * (k + 1)),
                     '%d (%d fit)' % (round_down(fit), fit) if fit else '-'), flush=True)
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


def closed_loop(a):
    out = {'closed_loop': []}
    print('| model | agents | setting | loop form (2 launches per step), s | one launch per chunk, s | loop / one launch | accepted iterations per solve '
          '| failed searches | mean reward sum, loop | mean reward sum, one launch |\n|---|---|---|---|---|---|---|---|---|---|', flush=True)
    for env_id, _ in MODELS:
        if a.models and env_id not in a.models:
            continue
        cfg = ops.make_cfg(env_id)
        for n in (a.agents or LOOP_AGENTS):
            obs0 = start_rows(env_id, n)
            for name, tol, warm in (('warm, tol 1e-3', 1e-3, True), ('cold, tol 0', 0., False)):
                if a.setting and not name.startswith(a.setting):
                    continue
                t, rec = {}, {}
                for form in (False, True):
                    ts = []
                    for i in range(a.warmup + a.regions):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        rec[form] = M.run_model_mpc(cfg, obs0, LOOP_STEPS, HORIZON, ITERS, tol, warm, one_launch=form)
                        torch.cuda.synchronize()
                        if i >= a.warmup:
                            ts.append(time.perf_counter() - t0)
                    t[form] = (statistics.median(ts), min(ts), max(ts))
                info = rec[True]['info']
                accepted = float(torch.where(info < 0, -info - 1, info).float().mean())
                row = dict(env=env_id, agents=n, setting=name, loop=t[False], one_launch=t[True], ratio=t[False][0] / t[True][0], accepted=accepted,
                           failed=int((info < 0).sum()), rew_loop=float(rec[False]['rew_traj'].double().sum(0).mean()),
                           rew_one_launch=float(rec[True]['rew_traj'].double().sum(0).mean()))
                out['closed_loop'].append(row)
                print('| %s | %d | %s | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) | %.2f | %.1f | %d | %.4f | %.4f |'
                      % ((env_id, n, name) + t[False] + t[True] + (row['ratio'], accepted, row['failed'], row['rew_loop'], row['rew_one_launch'])), flush=True)
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
    ap.add_argument('--closed-loop', action='store_true')
    ap.add_argument('--models', nargs='*', default=None, help='--closed-loop: env ids (default: all three)')
    ap.add_argument('--agents', nargs='*', type=int, default=None, help='--closed-loop: agent counts (default: 64 256)')
    ap.add_argument('--setting', choices=('warm', 'cold'), default=None, help='--closed-loop: one setting only')
    ap.add_argument('--regions', type=int, default=REGIONS)
    ap.add_argument('--warmup', type=int, default=WARMUP)
    ap.add_argument('--iters', type=int, default=3000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_model_mpc.py needs a GPU: nothing here is measured without one'
    if a.caps:
        return caps(a)
    if a.closed_loop:
        return closed_loop(a)
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
