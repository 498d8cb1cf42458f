#!/usr/bin/env python3
"""Times of the MPC baseline on the device, one process, medians of REGIONS timed regions after a warm-up, with the range:

  (a) one mpg_mpc_solve at horizon 25 and 200 iterations from zeros, for 1, 64, 4096 and 16384 rows: device events around REPS
      back-to-back solves of the same start states (drawn like the fixture's SLSQP states), a synchronise at the end of every region;
  (b) wall time of one run_mpc of 90 steps at 1 and 256 agents (horizon 25, 200 iterations per solve), host-inclusive, a synchronise
      at its end.

  --closed-loop: (c) the same run_mpc of 90 steps at 1 and 256 agents in four forms - the loop as it was (cold, tol 0), the one-launch
      form at the same settings (mpg_mpc_rollout per chunk of steps, mpg_eval_rollout, one policy pass), and both with warm_start and
      tol 1e-3 - wall time, host-inclusive, a synchronise at the end; the four forms alternate region by region, so that whatever else
      the machine is doing falls on all of them alike.  Beside the times: the mean accepted iterations per solve (from an untimed
      mpc_rollout of the same start, whose solves are the loop's bit for bit) and mpc_rl_summary's reward sums, mean over the agents.

There is no parent number for (a) and (b).  For comparison: the reference's recorded 2.14 s (SLSQP) and 33.8 ms (IPOPT) per solve on its authors' CPU
(SURVEY.md section 5), and 2.25 s per SLSQP solve on this project's CPU.

    python tools/bench_mpc.py [--json out.json]                  prints markdown tables
    python tools/bench_mpc.py --closed-loop [--json out.json]    (c) alone"""
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
from mpg_amd.policy import PolicyWithQs                      # noqa: E402

REGIONS, WARMUP = 7, 2
HORIZON, ITERS = 25, 200


def start_states(n):
    rng = np.random.default_rng(0)
    x = np.stack([rng.uniform(15, 25, n), rng.normal(0, 0.3, n), rng.normal(0, 0.1, n), rng.normal(0, 1, n), rng.normal(0, 0.3, n),
                  rng.uniform(0, 100, n)], 1)
    return torch.as_tensor(x, dtype=torch.float32).to('cuda')


def solve_case(rows, reps):
    x0 = start_states(rows)
    zeros = torch.zeros(rows, HORIZON, 2, device='cuda')
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(WARMUP):
        out = M.mpc_solve(x0, zeros, ITERS)
    torch.cuda.synchronize()
    t = []
    for _ in range(REGIONS):
        e0.record()
        for _ in range(reps):
            out = M.mpc_solve(x0, zeros, ITERS)
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1) / reps)
    info = out[3]
    return statistics.median(t), (min(t), max(t)), float(info.abs().float().mean()), int((info < 0).sum())


def loop_case(policy, agents):
    def wall():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        M.run_mpc(policy, num_agent=agents, steps=90, horizon=HORIZON, seed=1, iters=ITERS)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    wall()
    t = [wall() for _ in range(REGIONS)]
    return statistics.median(t), (min(t), max(t))


CLOSED_LOOP_FORMS = (('loop, cold, tol 0 (as it was)', dict()),
                     ('one launch, cold, tol 0', dict(one_launch=True)),
                     ('loop, warm, tol 1e-3', dict(warm_start=True, tol=1e-3)),
                     ('one launch, warm, tol 1e-3', dict(one_launch=True, warm_start=True, tol=1e-3)))


def accepted_iterations(agents, warm_start, tol):
    """mean accepted iterations per solve over run_mpc's 90 steps from its start (untimed)"""
    from mpg_amd.envs import PathTrackingEnv
    env = PathTrackingEnv(num_future_data=0, num_agent=agents, device='cuda', seed=1)
    env.reset()
    u = torch.zeros(agents, HORIZON, 2, device='cuda')
    chunk, info = max(1, M.MAX_ROLLOUT_WORK // ITERS), []
    for t0 in range(0, 90, chunk):
        out = M.mpc_rollout(env, u, min(chunk, 90 - t0), HORIZON, ITERS, tol, warm_start)
        u = out[6]
        info.append(out[5])
    info = torch.cat(info)
    return float(torch.where(info < 0, -info - 1, info).double().mean())


def closed_loop_case(policy, agents):
    def wall(kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rec = M.run_mpc(policy, num_agent=agents, steps=90, horizon=HORIZON, seed=1, iters=ITERS, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, rec
    times = {name: [] for name, _ in CLOSED_LOOP_FORMS}
    recs = {}
    for name, kw in CLOSED_LOOP_FORMS:                    # warm-up: every form once
        recs[name] = wall(kw)[1]
    for _ in range(REGIONS):                             # the forms alternate region by region
        for name, kw in CLOSED_LOOP_FORMS:
            times[name].append(wall(kw)[0])
    rows = []
    for name, kw in CLOSED_LOOP_FORMS:
        s = M.mpc_rl_summary(recs[name])
        t = times[name]
        rows.append(dict(agents=agents, form=name, ms=statistics.median(t), range=(min(t), max(t)),
                         iterations=accepted_iterations(agents, kw.get('warm_start', False), kw.get('tol', 0.)),
                         mpc_rew_sum=float(s['mpc_rew_sum'].mean()), rl_rew_sum=float(s['rl_rew_sum'].mean())))
    same = all(torch.equal(recs[CLOSED_LOOP_FORMS[a][0]][k], recs[CLOSED_LOOP_FORMS[b][0]][k]) for a, b in ((0, 1), (2, 3)) for k in recs[CLOSED_LOOP_FORMS[a][0]])
    return rows, same


def closed_loop(a):
    policy = PolicyWithQs(6, 2, init_seed=0, device='cuda')
    out = {'closed_loop': []}
    print('| agents | run_mpc, 90 steps | wall ms (host-inclusive) | per step, ms | accepted iterations per solve | MPC reward sum | '
          'policy reward sum |\n|---|---|---|---|---|---|---|', flush=True)
    for agents in (1, 256):
        rows, same = closed_loop_case(policy, agents)
        assert same, 'the one-launch record differs from the loop\'s'
        out['closed_loop'] += rows
        for r in rows:
            print('| %d | %s | %.1f (%.1f .. %.1f) | %.3f | %.1f | %.4f | %.4f |' % (agents, r['form'], r['ms'], r['range'][0], r['range'][1],
                                                                                  r['ms'] / 90, r['iterations'], r['mpc_rew_sum'], r['rl_rew_sum']),
                  flush=True)
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--closed-loop', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_mpc.py needs a GPU: nothing here is measured without one'
    if a.closed_loop:
        return closed_loop(a)
    out = {'solve': [], 'run_mpc': []}
    print('| rows | one solve (horizon %d, %d iterations), ms | per row, us | mean |info| | failed searches |\n|---|---|---|---|---|'
          % (HORIZON, ITERS), flush=True)
    for rows in (1, 64, 4096, 16384):
        m, r, it, failed = solve_case(rows, reps=3)
        out['solve'].append(dict(rows=rows, ms=m, range=r, mean_abs_info=it, failed=failed))
        print('| %d | %.3f (%.3f .. %.3f) | %.2f | %.1f | %d |' % (rows, m, r[0], r[1], 1e3 * m / rows, it, failed), flush=True)
    policy = PolicyWithQs(6, 2, init_seed=0, device='cuda')
    print('\n| agents | run_mpc, 90 steps, wall ms | per step, ms |\n|---|---|---|', flush=True)
    for agents in (1, 256):
        m, r = loop_case(policy, agents)
        out['run_mpc'].append(dict(agents=agents, ms=m, range=r))
        print('| %d | %.1f (%.1f .. %.1f) | %.3f |' % (agents, m, r[0], r[1], m / 90), flush=True)
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
