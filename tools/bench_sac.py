#!/usr/bin/env python3
"""Time of one SAC training step through the method-by-method path of SingleProcessOffPolicyOptimizer, and - in the same process and
in the same form - of the method-path TD3 step, at B = 256 and B = 4096: medians of REGIONS timed regions of STEPS steps after a
warm-up (device events around the region, a synchronise at its end), the two learners alternating region by region.

TD3 is the comparison, not a bar: per step it runs the same network passes as SAC (targets: policy + two critics; two critic
losses; policy gradient: policy, two critics forward, two critics backward with dx, policy backward, weight gradient) less the
Gaussian-head launches and two output columns.  Both are the per-call Python path (fused=False for TD3): the native step driver
removes that host time for TD3 and is not built for SAC.

    python tools/bench_sac.py [--json out.json]          prints a markdown table (EXPERIMENTS.md)

--squashed: the tanh-squashed head instead.  The three squashed entry points (mpg_policy_sample_squashed, mpg_sac_targets_squashed,
mpg_sac_policy_grad_squashed) against their plain siblings on PathTracking at B = 256 and B = 4096 - the same weights, observations
and draws, one cfg with action_range 2 and one without, candidates alternating region by region - and one SAC step (method path) on
InvertedPendulumConti-v0 beside the plain PathTracking SAC step at the same batch sizes."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REGIONS, STEPS, WARMUP = 7, 200, 40


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def stack(alg, B, **kw):
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import SACLearner, TD3Learner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    # (the same replay settings for both; TD3's own parser has delay_update 2: set to SAC's 1 so that both update the policy every step)
    args = default_args(alg, replay_batch_size=B, replay_starts=max(3000, B), delay_update=1, nan_check_interval=10 ** 9, **kw)
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    learner = (SACLearner if alg == 'SAC' else TD3Learner)(PolicyWithQs, args)
    opt = SingleProcessOffPolicyOptimizer(worker, learner, ReplayBuffer(args, 0), None, args, fused=False)
    assert opt._fused is None
    return opt


def alternate(fa, fb, steps=STEPS):
    """(median, min, max) of REGIONS regions of `steps` calls of each candidate, the two alternating region by region"""
    for _ in range(WARMUP):
        fa(), fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(REGIONS):
        ta.append(timed(fa, steps))
        tb.append(timed(fb, steps))
    return [(statistics.median(t), min(t), max(t)) for t in (ta, tb)]


def squashed(a):
    from mpg_amd import ops
    from mpg_amd.optimizer import quiesce_gc
    from mpg_amd.policy import init_mlp_flat
    out, dev = [], 'cuda'
    fmt = lambda t: '%.4f (%.4f .. %.4f)' % t
    print('| B | entry point | squashed, ms | plain, ms | squashed / plain |\n|---|---|---|---|---|')
    for B in (256, 4096):
        gen = torch.Generator().manual_seed(B)
        wp, q1, q2 = [init_mlp_flat(gen, i, o).to(dev) for i, o in ((6, 4), (8, 1), (8, 1))]
        obs = (torch.randn(B, 6, generator=gen) * torch.tensor([2., 1., 0.3, 1., 0.3, 100.])).to(dev)
        eps, rew = torch.randn(B, 2, generator=gen).to(dev), -torch.rand(B, generator=gen).to(dev)
        plain = ops.make_cfg(policy_out_activation='linear')
        ranged = ops.make_cfg(policy_out_activation='linear', action_range=2.0)
        pairs = (('policy_sample', lambda: ops.policy_sample_squashed(ranged, wp, obs, eps), lambda: ops.policy_sample(plain, wp, obs, eps)),
                 ('sac_targets', lambda: ops.sac_targets_squashed(ranged, wp, q1, q2, rew, obs, eps, 0.03),
                  lambda: ops.sac_targets(plain, wp, q1, q2, rew, obs, eps, 0.03)),
                 ('sac_policy_grad', lambda: ops.sac_policy_grad_squashed(ranged, wp, q1, q2, obs, eps, 0.03),
                  lambda: ops.sac_policy_grad(plain, wp, q1, q2, obs, eps, 0.03)))
        for name, fs, fp in pairs:
            ts, tp = alternate(fs, fp)
            out.append(dict(B=B, entry=name, squashed_ms=ts, plain_ms=tp))
            print('| %d | %s | %s | %s | %.3f |' % (B, name, fmt(ts), fmt(tp), ts[0] / tp[0]))
    print('\n| B | SAC step, pendulum, squashed head (method path), ms | SAC step, PathTracking, plain head, ms | ratio |\n|---|---|---|---|')
    for B in (256, 4096):
        pend = stack('SAC', B, env_id='InvertedPendulumConti-v0', squashed_head=True, num_agent=8)
        pt = stack('SAC', B)
        quiesce_gc()
        ts, tp = alternate(pend.step, pt.step)
        out.append(dict(B=B, entry='step', pendulum_squashed_ms=ts, path_tracking_plain_ms=tp))
        print('| %d | %s | %s | %.3f |' % (B, fmt(ts), fmt(tp), ts[0] / tp[0]))
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--squashed', action='store_true', help='the tanh-squashed head against the plain one, and the pendulum step')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_sac.py needs a GPU: nothing here is measured without one'
    if a.squashed:
        return squashed(a)
    from mpg_amd.optimizer import quiesce_gc
    out = []
    print('| B | SAC step (method path), ms | TD3 step (method path), ms | SAC / TD3 |\n|---|---|---|---|')
    for B in (256, 4096):
        sac, td3 = stack('SAC', B), stack('TD3', B)
        quiesce_gc()
        for _ in range(WARMUP):
            sac.step(), td3.step()
        torch.cuda.synchronize()
        ts, tt = [], []
        for _ in range(REGIONS):                              # alternating: both see the same machine
            ts.append(timed(sac.step, STEPS))
            tt.append(timed(td3.step, STEPS))
        ms, mt = statistics.median(ts), statistics.median(tt)
        out.append(dict(B=B, sac_ms=ms, sac_range=(min(ts), max(ts)), td3_ms=mt, td3_range=(min(tt), max(tt))))
        print('| %d | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) | %.2f |' % (B, ms, min(ts), max(ts), mt, min(tt), max(tt), ms / mt))
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
