"""mpg_worker_step with look-ahead observations (num_future_data = K > 0, obs_dim = 6 + K in 7 .. 16): the worker's policy pass on the
16-wide first layer and the env step as ONE launch, against the two stand-alone calls (mpg_policy_action + mpg_env_step_store_reset) it
replaces - bit for bit, like the six-wide launch in tests/test_env_gpu.py - and the native step driver, which takes that launch at
K > 0 from both branches of mpg_step_begin, against the method-by-method path (whose python classes keep calling the two stand-alone
entry points).  The refusals of the entry point need no GPU: every argument is validated before anything is enqueued."""
import ctypes

import numpy as np
import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops

NULL, FAKE = ctypes.c_void_p(0), ctypes.c_void_p(0x1000)      # FAKE: never dereferenced - the call must be refused before any launch
I, U64, F = ctypes.c_int, ctypes.c_uint64, ctypes.c_float
MPG_EINVAL = -1000


def _pair(K, n, sigma, cache, cfg, poison=None):
    """(two stand-alone calls, one mpg_worker_step) on twin envs: actions, ring arrays, env state, next observations, done flags"""
    from mpg_amd.envs import PathTrackingEnv
    from tests.golden_inputs import mlp_weights_flat
    od = 6 + K
    rng = np.random.Generator(np.random.PCG64(n))
    cap, nxt = 3 * n + 5, 2 * n + 9                   # next + n wraps around the ring
    pol = torch.as_tensor(mlp_weights_flat(rng, od, 4)).cuda()
    wc = None
    if cache:                                         # the packed-image instantiation: cfg.wcache[0] -> the policy's images
        wc = ops.WeightCache(pol, [(od, 4)])
        cfg.wcache[0] = wc.pointer
    env_a, env_b = PathTrackingEnv(num_future_data=K, num_agent=n, seed=4), PathTrackingEnv(num_future_data=K, num_agent=n, seed=4)
    obs_a, obs_b = env_a.reset().clone(), env_b.reset().clone()
    assert obs_a.shape == (n, od)
    if poison is not None:
        obs_a[poison], obs_b[poison] = float('nan'), float('nan')
    ring_a = [torch.zeros(cap, od).cuda(), torch.zeros(cap, 2).cuda(), torch.zeros(cap).cuda(), torch.zeros(cap, od).cuda(),
              torch.zeros(cap, dtype=torch.uint8).cuda()]
    ring_b = [torch.zeros_like(t) for t in ring_a]
    done_a, done_b = torch.empty(n, dtype=torch.uint8).cuda(), torch.empty(n, dtype=torch.uint8).cuda()
    status = []
    st = torch.zeros(1, dtype=torch.int32).cuda() if poison is not None else None
    if st is not None:
        cfg.status = st.data_ptr()
    # two calls
    act_a = ops.policy_action(cfg, pol, obs_a, explore_sigma=sigma, seed=11, ctr=5)
    L.call('mpg_env_step_store_reset', L.c_int(0), L.c_int(n), L.c_int(od), L.ptr(env_a._state), L.ptr(act_a), L.c_int(cap), L.c_int(nxt),
           *[L.ptr(t) for t in ring_a], L.c_u64(env_a.seed), L.c_u64(env_a._ctr), L.ptr(obs_a), L.ptr(done_a), L.stream())
    if st is not None:
        status.append(int(st.item()))
        st.zero_()
    # one call
    act_b = torch.empty(n, 2).cuda()
    L.call('mpg_worker_step', ctypes.byref(cfg), L.ptr(pol), L.c_int(n), L.ptr(env_b._state), L.ptr(obs_b), L.c_float(sigma), L.c_u64(11),
           L.c_u64(5), L.ptr(act_b), L.c_int(cap), L.c_int(nxt), *[L.ptr(t) for t in ring_b], L.c_u64(env_b.seed), L.c_u64(env_b._ctr),
           L.ptr(done_b), L.ptr(None), L.c_int(0), L.ptr(None), L.ptr(None), L.ptr(None), L.ptr(None), L.stream())
    torch.cuda.synchronize()
    if st is not None:
        status.append(int(st.item()))
    del wc
    return (act_a, ring_a, env_a._state, obs_a, done_a), (act_b, ring_b, env_b._state, obs_b, done_b), status


@pytest.mark.gpu
@pytest.mark.parametrize('engine', ['split', 'f32'])
@pytest.mark.parametrize('K,n,sigma,cache', [(1, 17, 0.3, False), (3, 300, 0.0, True), (10, 300, 0.3, False), (2, 48, 0.3, True)])
def test_wide_worker_step_equals_policy_action_plus_env_step_store_reset(K, n, sigma, cache, engine):
    """obs_dim 7 (one ragged group), 9 (ragged last group, packed weight cache), 16 (the 16-wide input block is full) and 8 (which the
    network dispatch sends to the 16-wide engine): actions with exploration noise, the five ring arrays (wrapping), env state, next
    observations and done flags are those of the two stand-alone calls, bit for bit, under both engines."""
    with L.engine(engine):
        a, b, _ = _pair(K, n, sigma, cache, ops.make_cfg(obs_dim=6 + K))
    assert torch.equal(a[0], b[0])
    assert bool((b[1][0][:, 6:] != 0).any())          # the look-ahead entries went into the ring
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)
    assert torch.equal(a[3], b[3]) and torch.equal(a[2], b[2]) and torch.equal(a[4], b[4])


@pytest.mark.gpu
def test_wide_worker_step_reports_a_nan_observation_like_the_two_calls():
    """judge_is_nan on the device (worker.py:95-107): one NaN look-ahead entry of one row sets MPG_STATUS_NAN and poisons that row's
    action, in the one launch exactly as in the stand-alone policy launch - same status word, same NaN mask, same finite entries."""
    a, b, status = _pair(3, 48, 0.3, False, ops.make_cfg(obs_dim=9), poison=(21, 7))
    assert status[0] == status[1] and status[1] & ops.STATUS_NAN, status
    nan_a, nan_b = torch.isnan(a[0]), torch.isnan(b[0])
    assert torch.equal(nan_a, nan_b) and bool(nan_b[21].all()) and int(nan_b.any(1).sum()) == 1
    assert torch.equal(a[0][~nan_a], b[0][~nan_b])


def _refused(obs_dim, draw):
    lib, c = L.lib(), ops.make_cfg(obs_dim=9)
    c.obs_dim = obs_dim
    rc = lib.mpg_worker_step(ctypes.byref(c), FAKE, I(16), FAKE, FAKE, F(0.1), U64(1), U64(0), FAKE, I(64), I(0), FAKE, FAKE, FAKE, FAKE, FAKE,
                             U64(1), U64(0), NULL, draw, I(16), FAKE, FAKE, FAKE, FAKE, NULL)
    return rc, lib.mpg_last_error().decode()


def test_worker_step_refuses_observations_wider_than_16():
    rc, msg = _refused(17, NULL)
    assert rc == MPG_EINVAL and 'mpg_worker_step' in msg and 'obs_dim 6 .. 16' in msg, msg


def test_worker_step_refuses_a_draw_with_look_ahead_observations():
    """the pre-gathered draw is six wide and feeds the fused gradient launch, which these widths do not have: refused with a message
    that names the restriction, not with the entry point's general one"""
    rc, msg = _refused(9, FAKE)
    assert rc == MPG_EINVAL and 'mpg_worker_step' in msg and 'draw' in msg and 'obs_dim 6 only' in msg and 'obs_dim 9' in msg, msg


@pytest.mark.gpu
def test_native_step_driver_equals_method_by_method_path_with_look_ahead():
    """tests/test_learner_gpu.py::test_native_step_driver_equals_method_by_method_path for MPG-v2 at num_future_data = 3: the
    regression net for the MPG branch of mpg_step_begin, whichever form of the worker step train_step.cpp::worker_step_fused selects
    at obs_dim 9 (the python worker issues mpg_policy_action + mpg_env_step_store_reset).  Same assertions, same tolerances."""
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import MPGLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker

    def run(fused):
        args = default_args('MPG-v2', num_agent=64, batch_size=128, replay_batch_size=96, replay_starts=512, max_buffer_size=1000,
                            num_batch_reuse=1, num_future_data=3)
        worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
        learner = MPGLearner(PolicyWithQs, args)
        rb = ReplayBuffer(args, 0)
        opt = SingleProcessOffPolicyOptimizer(worker, learner, rb, None, args, sampling_interval=3, fused=fused)
        assert (opt._fused is not None) == fused
        for _ in range(9):
            opt.step()
        pw = worker.policy_with_value
        st = learner.get_stats()
        assert rb.obs.shape[1] == 9
        return [pw.params.clone(), pw.targets.clone(), pw.m.clone(), pw.v.clone(), rb.obs.clone(), rb.rew.clone(),
                learner.flat.clone()], (dict(pw.opt_steps), rb._next_idx, len(rb), worker._noise_ctr, st['q_loss1'])
    a, ca = run(True)
    b, cb = run(False)
    assert ca[:4] == cb[:4], (ca, cb)
    assert abs(ca[4] - cb[4]) <= 1e-6 * abs(cb[4])
    assert torch.equal(a[4], b[4])                    # ring: same reset-law draws in the same slots
    assert (a[5] - b[5]).abs().max().item() < 1e-4    # rewards depend on the (rounding-different) policy
    for x, y in zip(a[:4], b[:4]):
        assert (x - y).abs().max().item() <= 1e-6 * max(1.0, y.abs().max().item())
    g1, g2 = a[6], b[6]
    assert ((g1 - g2).norm() / g2.norm()).item() < 1e-5


@pytest.mark.gpu
def test_native_step_driver_equals_method_path_for_td3_with_look_ahead():
    """tests/test_config34_gpu.py::test_native_step_driver_equals_method_path_for_td3_and_nadp for TD3 (uniform replay) at
    num_future_data = 3: the regression net for `sample_and_add` as the NADP / TD3 branch calls it (no draw request).  Same assertions,
    same tolerances."""
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import TD3Learner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker

    def run(fused):
        args = default_args('TD3', num_agent=64, batch_size=128, replay_batch_size=96, replay_starts=512, max_buffer_size=1000,
                            buffer_type='normal', num_future_data=3)
        worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
        learner = TD3Learner(PolicyWithQs, args)
        rb = ReplayBuffer(args, 0)
        opt = SingleProcessOffPolicyOptimizer(worker, learner, rb, None, args, sampling_interval=3, fused=fused)
        assert (opt._fused is not None) == fused
        for _ in range(9):
            opt.step()
        pw = worker.policy_with_value
        st = learner.get_stats()
        torch.cuda.synchronize()
        assert rb.obs.shape[1] == 9
        out = [pw.params.clone(), pw.targets.clone(), pw.m.clone(), pw.v.clone(), rb.obs.clone(), learner.flat.clone()]
        return out, (dict(pw.opt_steps), rb._next_idx, len(rb), rb.replay_times, worker._noise_ctr, learner.counter, float(st['q_loss1']))
    a, ca = run(True)
    b, cb = run(False)
    assert ca[:6] == cb[:6], (ca, cb)
    assert abs(ca[6] - cb[6]) <= 1e-5 * abs(cb[6]) + 1e-7
    assert torch.equal(a[4], b[4])                    # ring observations: the same reset-law draws in the same slots
    for x, y in zip(a[:4], b[:4]):
        assert (x - y).abs().max().item() <= 2e-6 * max(1.0, y.abs().max().item())
    assert ((a[5] - b[5]).norm() / b[5].norm()).item() < 1e-4
