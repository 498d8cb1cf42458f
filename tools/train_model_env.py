#!/usr/bin/env python3
"""NADP or AMPC end to end on the model-backed InvertedDoublePendulum-v2 env (args.env_on_model) with the stock
worker, buffer, optimizer and learner at default_args' values: ModelEvaluator's mean return over `--episodes` episodes of `--steps`
steps from reset-law starts before and after `--iters` optimizer steps, the share of done rows among the sampled transitions, and the
wall time of the training loop.  A measurement: nothing is asserted beyond finite numbers.

    python tools/train_model_env.py [--alg NADP] [--iters 3000] [--loop] [--json out.json]      (--loop: OffPolicyWorker's loop instead of
                                                                                                 the one-launch sample)"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--alg', default='NADP', choices=('NADP', 'AMPC'))
    ap.add_argument('--iters', type=int, default=3000)
    ap.add_argument('--episodes', type=int, default=64)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--loop', action='store_true')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'train_model_env.py needs a GPU: nothing here is measured without one'
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.envs import make_model_env
    from mpg_amd.evaluator import ModelEvaluator
    from mpg_amd.learners import AMPCLearner, NADPLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer, quiesce_gc
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    env_id = 'InvertedDoublePendulum-v2'
    more = dict(num_rollout_list_for_policy_update=[25]) if a.alg == 'AMPC' else {}
    args = default_args(a.alg, env_id=env_id, env_on_model=True, one_launch_sample=not a.loop, seed=a.seed, init_seed=a.seed,
                        fixed_steps=a.steps, **more)
    worker = OffPolicyWorker(PolicyWithQs, env_id, args, 0)
    learner = (AMPCLearner if a.alg == 'AMPC' else NADPLearner)(PolicyWithQs, args)
    rb = ReplayBuffer(args, 0)
    evaluator = ModelEvaluator(PolicyWithQs, env_id, args)
    opt = SingleProcessOffPolicyOptimizer(worker, learner, rb, evaluator, args, sampling_interval=10)
    assert opt._fused is None
    evaluator.share_policy(worker.policy_with_value)
    starts = make_model_env(env_id, num_agent=a.episodes, seed=a.seed + 424242).reset()
    before = evaluator.run_n_episodes_parallel(starts)[1]['episode_return']
    quiesce_gc()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        opt.step()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    after = evaluator.run_n_episodes_parallel(starts)[1]['episode_return']
    n = len(rb)
    done = int(rb.done[:n].sum().item())
    out = dict(alg=a.alg, iters=a.iters, sample='loop' if a.loop else 'one launch', num_agent=args.num_agent, batch_size=args.batch_size,
               replay_batch_size=args.replay_batch_size, episodes=a.episodes, steps=a.steps, return_before=before, return_after=after,
               sampled=opt.num_sampled_steps, ring_rows=n, done_rows=done, wall_s=wall, ms_per_iteration=1e3 * wall / max(a.iters, 1))
    assert all(x == x and abs(x) != float('inf') for x in (before, after))
    print('| learner | iterations | sample | mean return of %d x %d model steps, before -> after | sampled transitions | done rows in the buffer | '
          'ms per iteration (wall) |\n|---|---|---|---|---|---|---|' % (a.episodes, a.steps))
    print('| %s | %d | %s | %.2f -> %.2f | %d | %d of %d | %.3f |'
          % (a.alg, a.iters, out['sample'], before, after, out['sampled'], done, n, out['ms_per_iteration']), flush=True)
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
