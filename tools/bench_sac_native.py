#!/usr/bin/env python3
"""Times of SAC's native pieces on the GPU, one process, medians of REGIONS timed regions of REPS steps after a warm-up (device events
around the region, a synchronise at its end), the candidates alternating region by region:

  (a) the stochastic worker step as ONE launch (mpg_worker_sample_step) against the three calls it replaces (mpg_normal_fill,
      mpg_policy_sample, mpg_env_step_store_reset: four launches), both enqueued by the same C loop (tools/bench_sac_native_chain.c,
      compiled on first use) from the same start, bit-identical at the end; 8 and 4096 agents, obs_dim 6 and 9.  The rule of the
      driver (train_step.cpp, sac_worker_one_launch): at a width it takes the one launch only if that is at least as fast at BOTH sizes;
  (b) one SAC step at the reference's worker defaults (8 agents, batch_size 512, sampling every 10th step), B = 256 and 4096: the
      native step (native_sac=True), the method-by-method path, and the native TD3 step.

  (c) --auto: the learned temperature (alpha = 'auto', target_entropy -2) - the native step (mpg_sac_auto_step_begin / _end) beside the
      native fixed-alpha step and the 'auto' method path, same settings, B = 256 and 4096.  No bar: the fixed-alpha native step of
      the same run is the comparison (the 'auto' step adds one mpg_normal_fill and the temperature's one-thread launch).

tools/bench_sac.py stays as the record of the method-path measurement.

    python tools/bench_sac_native.py [--auto] [--json out.json]          prints markdown tables (EXPERIMENTS.md)"""
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
from tests.golden_inputs import mlp_weights_flat             # noqa: E402

REGIONS, REPS, WARMUP = 7, 200, 40
I, U64, SZ, P = ctypes.c_int, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_void_p


class Bufs(ctypes.Structure):
    """bench_bufs_t"""
    _fields_ = [(k, P) for k in ('state', 'obs', 'eps', 'act', 'logp', 'ring_obs', 'ring_act', 'ring_rew', 'ring_obs2', 'ring_done', 'done',
                                 'ws')] + [('ws_bytes', SZ), ('capacity', I)]


def host_loops():
    """tools/bench_sac_native_chain.c as a shared object beside it (rebuilt when the source is newer)"""
    here = os.path.dirname(os.path.abspath(__file__))
    src, so = os.path.join(here, 'bench_sac_native_chain.c'), os.path.join(here, 'bench_sac_native_chain.so')
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


def worker_case(n, od):
    from mpg_amd.envs import PathTrackingEnv
    dev = 'cuda'
    rng = np.random.Generator(np.random.PCG64(n + od))
    cfg = ops.make_cfg(obs_dim=od, policy_out_activation='linear')
    pol = torch.as_tensor(mlp_weights_flat(rng, od, 4)).to(dev)
    wc = ops.WeightCache(pol, [(od, 4)])
    cfg.wcache[0] = wc.pointer
    env = PathTrackingEnv(num_future_data=od - 6, num_agent=n, seed=n)
    obs0, state0 = env.reset().clone(), None
    state0 = env._state.clone()
    cap = 4 * n + 24                                              # (the ring wraps inside a region)
    ws = torch.empty(L.lib().mpg_policy_sample_workspace_bytes(ctypes.byref(cfg), I(n)) + 256, dtype=torch.uint8, device=dev)
    keep, sides = [wc, ws], []
    for _ in range(2):                                            # one set of buffers per candidate, from the same start
        f = dict(dtype=torch.float32, device=dev)
        t = dict(state=state0.clone(), obs=obs0.clone(), eps=torch.zeros(n, 2, **f), act=torch.zeros(n, 2, **f), logp=torch.zeros(n, **f),
                 ring_obs=torch.zeros(cap, od, **f), ring_act=torch.zeros(cap, 2, **f), ring_rew=torch.zeros(cap, **f),
                 ring_obs2=torch.zeros(cap, od, **f), ring_done=torch.zeros(cap, dtype=torch.uint8, device=dev),
                 done=torch.zeros(n, dtype=torch.uint8, device=dev))
        b = Bufs()
        for k, v in t.items():
            setattr(b, k, v.data_ptr())
        b.ws, b.ws_bytes, b.capacity = ws.data_ptr(), ws.numel(), cap
        sides.append((t, b))
    lib, s, c = L.lib(), L.stream(), ctypes.byref(cfg)
    fp = lambda f: ctypes.cast(f, ctypes.c_void_p)
    host = host_loops()
    ctr = [0, 0]

    def chain(reps):
        assert host.bench_chain(fp(lib.mpg_normal_fill), fp(lib.mpg_policy_sample), fp(lib.mpg_env_step_store_reset), c, L.ptr(pol), I(n),
                                ctypes.byref(sides[0][1]), U64(ctr[0]), s, I(reps)) == 0
        ctr[0] += reps

    def launch(reps):
        assert host.bench_launch(fp(lib.mpg_worker_sample_step), c, L.ptr(pol), I(n), ctypes.byref(sides[1][1]), U64(ctr[1]), s, I(reps)) == 0
        ctr[1] += reps
    chain(WARMUP), launch(WARMUP)
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(REGIONS):                                      # alternating: both see the same machine
        ta.append(timed(chain, batched=True))
        tb.append(timed(launch, batched=True))
    torch.cuda.synchronize()
    for k in ('state', 'obs', 'act'):                             # the two did the same work: bit-identical at the end
        assert torch.equal(sides[0][0][k].view(torch.int32), sides[1][0][k].view(torch.int32)), k
    del keep
    return statistics.median(ta), statistics.median(tb), (min(ta), max(ta)), (min(tb), max(tb))


def stack(alg, B, native, auto=False):
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import SACLearner, TD3Learner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    # (the settings of tools/bench_sac.py: the same replay settings for both; TD3's own parser has delay_update 2: set to SAC's 1)
    more = dict(alpha='auto', target_entropy=-2.) if auto else {}
    args = default_args(alg, replay_batch_size=B, replay_starts=max(3000, B), delay_update=1, nan_check_interval=10 ** 9, **more)
    assert (args.num_agent, args.batch_size) == (8, 512)
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    learner = (SACLearner if alg == 'SAC' else TD3Learner)(PolicyWithQs, args)
    more = dict(native_sac=True) if (alg == 'SAC' and native) else {}
    opt = SingleProcessOffPolicyOptimizer(worker, learner, ReplayBuffer(args, 0), None, args, sampling_interval=10, **more)
    assert (opt._fused is not None) == native
    return opt


def auto_leg(out):
    from mpg_amd.optimizer import quiesce_gc
    out['auto'] = []
    print("| B | SAC 'auto' native, ms | SAC fixed alpha native, ms | SAC 'auto' method path, ms | auto / fixed (native) | method / native (auto) |"
          '\n|---|---|---|---|---|---|', flush=True)
    for B in (256, 4096):
        opts = [stack('SAC', B, True, auto=True), stack('SAC', B, True), stack('SAC', B, False, auto=True)]
        quiesce_gc()
        for _ in range(WARMUP):
            for o in opts:
                o.step()
        torch.cuda.synchronize()
        t = [[], [], []]
        for _ in range(REGIONS):                              # alternating: all three see the same machine
            for k, o in enumerate(opts):
                t[k].append(timed(o.step, REPS))
        m = [statistics.median(x) for x in t]
        out['auto'].append(dict(B=B, auto_native_ms=m[0], auto_native_range=(min(t[0]), max(t[0])), fixed_native_ms=m[1],
                                fixed_native_range=(min(t[1]), max(t[1])), auto_method_ms=m[2], auto_method_range=(min(t[2]), max(t[2]))))
        print('| %d | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) | %.2f | %.2f |'
              % (B, m[0], min(t[0]), max(t[0]), m[1], min(t[1]), max(t[1]), m[2], min(t[2]), max(t[2]), m[0] / m[1], m[2] / m[0]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--auto', action='store_true', help="the learned temperature's table only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_sac_native.py needs a GPU: nothing here is measured without one'
    from mpg_amd.optimizer import quiesce_gc
    if a.auto:
        out = {}
        auto_leg(out)
        if a.json:
            with open(a.json, 'w') as fh:
                json.dump(out, fh, indent=1)
        return
    out = {'worker': [], 'step': []}
    print('| agents | obs_dim | (a) three calls, 4 launches, ms | (b) mpg_worker_sample_step, ms | (a) / (b) |\n|---|---|---|---|---|', flush=True)
    for od in (6, 9):
        for n in (8, 4096):
            ma, mb, ra, rb = worker_case(n, od)
            out['worker'].append(dict(agents=n, obs_dim=od, chain_ms=ma, chain_range=ra, launch_ms=mb, launch_range=rb))
            print('| %d | %d | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) | %.2f |' % (n, od, ma, ra[0], ra[1], mb, rb[0], rb[1], ma / mb), flush=True)
    print('\n| B | SAC native, ms | SAC method path, ms | TD3 native, ms | method / native | native SAC / native TD3 |\n|---|---|---|---|---|---|', flush=True)
    for B in (256, 4096):
        opts = [stack('SAC', B, True), stack('SAC', B, False), stack('TD3', B, True)]
        quiesce_gc()
        for _ in range(WARMUP):
            for o in opts:
                o.step()
        torch.cuda.synchronize()
        t = [[], [], []]
        for _ in range(REGIONS):                              # alternating: all three see the same machine
            for k, o in enumerate(opts):
                t[k].append(timed(o.step, REPS))
        m = [statistics.median(x) for x in t]
        out['step'].append(dict(B=B, sac_native_ms=m[0], sac_native_range=(min(t[0]), max(t[0])), sac_method_ms=m[1],
                                sac_method_range=(min(t[1]), max(t[1])), td3_native_ms=m[2], td3_native_range=(min(t[2]), max(t[2]))))
        print('| %d | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) | %.2f | %.2f |'
              % (B, m[0], min(t[0]), max(t[0]), m[1], min(t[1]), max(t[1]), m[2], min(t[2]), max(t[2]), m[1] / m[0], m[0] / m[2]), flush=True)
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
