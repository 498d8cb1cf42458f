"""mpg_worker_rollout_pendulum on the GPU: the one launch against the chain of mpg_policy_action + mpg_env_step_store_reset pairs it
replaces, from identical starts, bit for bit - env state, observations, last actions, last done flags, all five ring arrays WHOLE
(prefilled with a sentinel, so the slots nobody writes count) and the status word; its callers - OffPolicyWorker.sample
(one_launch_sample) against the loop, the native step driver with the launch against the same driver kept on the chain
(sample_iters < 0).  The buffers, the comparison (floats as their 32-bit patterns: a NaN row has to match too) and the callers' pairs
are those of tests/rollout_harness.py.  Unlike PathTracking's, this env's done flag is real: the tests assert on the device's own
rows that agents were carried across iterations, fell, were re-drawn and went on."""
import ctypes
from functools import partial

import numpy as np
import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops
from tests import rollout_harness as H
from tests.rollout_harness import assert_same, bits, engine, ring_ptrs  # noqa: F401 (engine: a fixture)

pytestmark = pytest.mark.gpu
ENV_ID = 'InvertedPendulumConti-v0'


def gentle_last_layer(flat):
    flat[-(2 * 256 + 2):] *= np.float32(0.01)             # W3 [256][2] and b3 [2]


def Policy(packed, seed=0, gentle=False):
    """the pendulum's policy network (4 inputs, mean | log-std) under a linear output with action_range 3: a = 3 tanh(mean).  gentle:
    the last layer scaled by 0.01 - actions of a few hundredths, so that an agent near the upright stays up for many iterations and
    falls on its own."""
    return H.PolicyNet(4, 2, ops.make_cfg(ENV_ID), packed, 400 + seed, gentle_last_layer if gentle else None)


def reset_law_starts(n, seed=7):
    """U(-0.01, 0.01) on all four entries: the env's reset law (inverted_pendulum_conti.py:21-25)"""
    return np.random.Generator(np.random.PCG64(seed)).uniform(-0.01, 0.01, (n, 4)).astype(np.float32)


def mixed_starts(n):
    """even agents from the reset law; odd agents at p = 1.999 with pdot = 1: such an agent leaves |p| < 2 on the first step whatever
    the action does (at the largest force, 300 N on the cart, p changes by at least 0.04 * 1 - 1/2 * 30 * 0.04^2 = +0.016)"""
    s = reset_law_starts(n)
    s[1::2, 0] = 1.999
    s[1::2, 2] = 1.0
    return s


def start(n, cap, init_obs=None, nan_row=None):
    """agents from the reset law (seed 4) or from init_obs (through mpg_env_reset_from_obs)"""
    from mpg_amd.envs import InvertedPendulumContiEnv
    return H.start(InvertedPendulumContiEnv(num_agent=n, seed=4), 4, 1, n, cap, init_obs, nan_row)


def run_chain(p, t, n, iters, sigma, cap, nxt, nctr, ectr):
    p.status.zero_()
    for it in range(iters):
        L.call('mpg_policy_action', ctypes.byref(p.cfg), L.ptr(p.pol), L.c_int(n), L.ptr(t['obs_io']), L.c_float(sigma), L.c_u64(11),
               L.c_u64(nctr + it), L.ptr(t['act_out']), L.stream())
        L.call('mpg_env_step_store_reset', L.c_int(1), L.c_int(n), L.c_int(4), L.ptr(t['state']), L.ptr(t['act_out']), L.c_int(cap),
               L.c_int((nxt + it * n) % cap), *ring_ptrs(t), L.c_u64(4), L.c_u64(ectr + it), L.ptr(t['obs_io']), L.ptr(t['done_out']),
               L.stream())
    t['status'] = p.status.clone()


def run_launch(p, t, n, iters, sigma, cap, nxt, nctr, ectr):
    p.status.zero_()
    L.call('mpg_worker_rollout_pendulum', ctypes.byref(p.cfg), L.ptr(p.pol), L.c_int(n), L.c_int(iters), L.ptr(t['state']),
           L.ptr(t['obs_io']), L.c_float(sigma), L.c_u64(11), L.c_u64(nctr), L.ptr(t['act_out']), L.c_int(cap), L.c_int(nxt), *ring_ptrs(t),
           L.c_u64(4), L.c_u64(ectr), L.ptr(t['done_out']), L.stream())
    t['status'] = p.status.clone()


def both(p, n, iters, sigma, init_obs=None, nan_row=None, **where):
    """-> (chain, launch)"""
    def at_sigma(run):
        return lambda t, n, iters, *rest: run(p, t, n, iters, sigma, *rest)
    return H.both((at_sigma(run_chain), at_sigma(run_launch)), partial(start, init_obs=init_obs, nan_row=nan_row), n, iters, **where)


@pytest.mark.parametrize('packed', [False, True], ids=['strided', 'packed'])
def test_one_launch_equals_the_chain_of_policy_and_env_launches_bit_for_bit(engine, packed):
    """n: one agent (the reference's default: one live lane), half a 16-agent group, one group, a ragged third group.  iters = 1 is a
    single pair, 2 the first hand-over of the observations through LDS, 64 and 1 x 512 long enough for agents to fall."""
    p = Policy(packed)
    for n, all_iters in ((1, (1, 2, 5, 64, 512)), (8, (1, 2, 5, 64)), (16, (1, 2, 5, 64)), (40, (1, 2, 5, 64))):
        for iters in all_iters:
            for sigma in (0., 0.1):
                a, b = both(p, n, iters, sigma)
                assert_same(a, b, (n, iters, sigma))
                assert int(b['status'].item()) == 0
                w = H.touched(iters * n + 13, 5, iters * n)
                assert (b['ring_rew'][~w] == -7.).all() and (b['ring_rew'][w] != -7.).all()
                assert (b['ring_done'][~w] == 0xAB).all() and (b['ring_done'][w] <= 1).all()
                assert torch.isfinite(b['ring_obs2'][w]).all()


@pytest.mark.parametrize('packed', [False, True], ids=['strided', 'packed'])
def test_both_branches_of_done_in_one_run(engine, packed):
    """agents that live in a lane's registers for many iterations, fall, are re-drawn and go on - beside agents that fall at once.
    With the gentle policy the reset-law agents stay up for a dozen iterations or more and fall on their own inside 64 (checked on
    oracle.mpg_oracle.InvertedPendulumContiOracle for these starts and this policy under three noise draws of its own: first falls
    between iterations 10 and 33, every agent alive again behind its reset); the conditions are
    asserted on the DEVICE's own ring rows, so an all-done or all-alive run cannot pass."""
    n, iters = 40, 64
    for gentle in (True, False):
        p = Policy(packed, gentle=gentle)
        a, b = both(p, n, iters, 0.1, init_obs=mixed_starts(n))
        assert_same(a, b, ('gentle' if gentle else 'as drawn',))
        assert int(b['status'].item()) == 0
        if not gentle:
            continue
        done = b['ring_done'][5:5 + iters * n].view(iters, n).cpu().numpy()          # [iteration][agent]
        assert set(np.unique(done)) == {0, 1}
        assert (done[0, 1::2] == 1).all() and (done[0, 0::2] == 0).all()              # the starts did what they were built for
        lived_then_fell = after_reset = 0
        for i in range(n):
            col = done[:, i]
            lived_then_fell += any(col[t] == 1 and col[t - 1] == 0 and col[t - 2] == 0 for t in range(2, iters - 1))
            falls = np.flatnonzero(col)
            after_reset += bool(len(falls) and falls[0] < iters - 1 and col[falls[0] + 1] == 0)
        assert lived_then_fell >= 1 and after_reset >= 1, (lived_then_fell, after_reset)
        # a re-drawn agent starts from the reset law: the observation behind a done row lies in it
        obs = b['ring_obs'][5:5 + iters * n].view(iters, n, 4).cpu().numpy()
        t, i = np.nonzero(done[:-1])
        assert len(t) and (np.abs(obs[t + 1, i]) <= 0.01).all()


@pytest.mark.parametrize('packed', [True, False], ids=['packed', 'strided'])
def test_ring_wrap_inside_an_iteration_and_the_counters_carry(engine, packed):
    """capacity == iters * n with next_idx = capacity - 3: every slot is written once and the wrap falls inside an iteration's block;
    noise_ctr = env_ctr = 2^32 - 2: the counters' low words overflow at the third iteration"""
    p = Policy(packed, seed=1)
    for n, iters in ((8, 5), (40, 5), (16, 64), (1, 64)):
        cap = iters * n
        a, b = both(p, n, iters, 0.1, cap=cap, nxt=cap - 3, ctr=2 ** 32 - 2, ectr=2 ** 32 - 2, init_obs=mixed_starts(n))
        assert_same(a, b, (n, iters))
        assert (b['ring_rew'] != -7.).all() and (b['ring_done'] <= 1).all()
    # the high words matter: the same start and the same low words under another high word draw other noise, and - the odd agents fall
    # at the first step - other reset states
    n, iters, cap = 16, 5, 5 * 16 + 13
    lo = start(n, cap, mixed_starts(n))
    run_launch(p, lo, n, iters, 0.1, cap, 5, (2 ** 32 - 2) & 0xFFFFFFFF, (2 ** 32 - 2) & 0xFFFFFFFF)
    hi = start(n, cap, mixed_starts(n))
    run_launch(p, hi, n, iters, 0.1, cap, 5, 2 ** 33 - 2, 2 ** 33 - 2)       # the same low words, another high word
    torch.cuda.synchronize()
    assert not torch.equal(bits(lo['act_out']), bits(hi['act_out']))
    assert (lo['ring_done'][5 + 1:5 + n:2] == 1).all() and (hi['ring_done'][5 + 1:5 + n:2] == 1).all()
    first_reset = slice(5 + n + 1, 5 + 2 * n, 2)              # iteration 1's observations of the odd agents: their reset states
    assert not torch.equal(bits(lo['ring_obs'][first_reset]), bits(hi['ring_obs'][first_reset]))


@pytest.mark.parametrize('packed', [False, True], ids=['strided', 'packed'])
def test_a_nan_start_row_is_reported_and_stored_like_the_chain(engine, packed):
    """one agent and its observation NaN from the start: the policy pass sees the NaN observation, its action and the transition are
    NaN, and both paths OR MPG_STATUS_NAN into the status word; everything - the NaN entries' bit patterns included - is equal.  A NaN
    state is done (neither |p| < 2 nor |theta| <= 0.2 holds), so the agent is re-drawn and every other row is finite."""
    p = Policy(packed, seed=2)
    n, iters, row = 40, 5, 21
    a, b = both(p, n, iters, 0.1, nan_row=row)
    assert_same(a, b, 'nan row')
    assert int(a['status'].item()) == int(b['status'].item()) and int(b['status'].item()) & ops.STATUS_NAN
    slot = 5 + row                                         # the row's transition of iteration 0
    assert torch.isnan(b['ring_obs'][slot]).all() and torch.isnan(b['ring_act'][slot]).all() and torch.isnan(b['ring_rew'][slot])
    assert torch.isnan(b['ring_obs2'][slot]).all() and int(b['ring_done'][slot]) == 1
    keep = ~H.touched(iters * n + 13, slot, 1)
    for k in ('ring_obs', 'ring_act', 'ring_rew', 'ring_obs2'):
        assert torch.isfinite(b[k][keep]).all(), k
    assert torch.isfinite(b['state'][:4]).all() and torch.isfinite(b['obs_io']).all() and torch.isfinite(b['act_out']).all()


def test_repeated_launches_are_bit_identical(engine):
    """100 launches from one start: the hand-overs between the env lanes and the policy pass through LDS are the new thing here"""
    p = Policy(True, seed=3)
    n, iters, cap = 40, 5, 40 * 5 + 13
    H.assert_repeatable(lambda: start(n, cap, mixed_starts(n)), lambda t: run_launch(p, t, n, iters, 0.1, cap, 5, 7, 3), 100)


# ---- OffPolicyWorker.sample ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sigma', [None, 0.1], ids=['no_noise', 'sigma_0.1'])
@pytest.mark.parametrize('num_agent', [1, 8])
def test_worker_sample_one_launch_equals_the_loop(engine, num_agent, sigma):
    from mpg_amd.config import default_args

    def make(**more):
        args = default_args('NADP', num_agent=num_agent, batch_size=64, explore_sigma=sigma, seed=5, init_seed=5, **more)
        assert args.env_id == ENV_ID
        return args
    (_, _, ca), (_, _, cb) = H.worker_sample_pair(make)
    assert ca[0] == 2 * (64 // num_agent) and ca[2:] == (128, 2), (ca, cb)


# ---- native step driver ---------------------------------------------------------------------------------------------------------
def _stack(alg, per, **over):
    from mpg_amd.buffer import PrioritizedReplayBuffer, ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import NADPLearner, TD3Learner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    # replay_starts 512: one worker sample fills half the ring of 1024 before the first step (the default, 3000, never fits it)
    args = default_args(alg, env_id=ENV_ID, replay_batch_size=64, max_buffer_size=1024, replay_starts=512, seed=3, init_seed=3,
                        buffer_type='priority' if per else 'normal', nan_check_interval=10 ** 9, **over)
    assert (args.num_agent, args.batch_size) == (1, 512)              # the pendulum parsers' worker defaults: 512 iterations per sample
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    learner = (TD3Learner if alg == 'TD3' else NADPLearner)(PolicyWithQs, args)
    rb = (PrioritizedReplayBuffer if per else ReplayBuffer)(args, 0)
    opt = SingleProcessOffPolicyOptimizer(worker, learner, rb, None, args, sampling_interval=10)
    assert opt._fused is not None
    return opt


def _pair(alg, per, **over):
    """the driver with the launch against the driver on the chain (512 iterations, two launches each), 25 steps; either run wrapped
    the ring and stored both branches of done"""
    for tensors, c in H.driver_chain_pair(partial(_stack, alg, per, **over), 512, extra=H.per_trees if per else None):
        assert c[0] >= 3 * 512 and c[3] == 1024                       # noise_ctr, ring_size: samples at 0, 10 and 20, the ring of 1024 has wrapped
        assert 0 < int(tensors[8].sum().item()) < 1024                # the ring's done column: both branches of done went into it


@pytest.mark.parametrize('sigma', [None, 0.1], ids=['no_noise', 'sigma_0.1'])
def test_native_driver_with_the_launch_equals_the_driver_on_the_chain(engine, sigma):
    """NADP at the pendulum defaults, 25 iterations (samples at 0, 10, 20): the driver that issues mpg_worker_rollout_pendulum for the
    512 iterations of a sample against the same driver kept on the chain: parameters, Adam moments, targets, ring, worker buffers, env
    state, the learner's flat gradient, status word and counters, bit for bit."""
    _pair('NADP', False, explore_sigma=sigma)


@pytest.mark.parametrize('per', [False, True], ids=['td3', 'td3_priority'])
def test_native_td3_driver_with_the_launch_equals_the_driver_on_the_chain(engine, per):
    """TD3 on the pendulum, uniform and prioritized: the mpg_per_add calls follow the launch in iteration order, so the trees are
    compared too"""
    _pair('TD3', per)


def test_native_driver_issues_one_worker_launch_per_sample():
    """the driver's own timer counts the worker's launches (slot 2): one per sample with the launch, 512 env launches on the chain
    (slot 2 brackets mpg_env_step_store_reset there; the 512 policy launches count in slot 3) - the pairs above do compare two
    different launch sequences"""
    counts = H.worker_launch_counts(partial(_stack, 'NADP', False), 512, 2048)
    assert counts == [1, 512], counts
