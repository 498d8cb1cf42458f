"""mpg_worker_rollout on the GPU: the one launch against the chain of mpg_worker_step calls it replaces, from identical starts, bit
for bit - env state, observations, last actions, last done flags, all five ring arrays WHOLE (prefilled with a sentinel, so the slots
nobody writes count) and the status word; its callers - OffPolicyWorker.sample(one_launch_sample) against the loop, the native step
driver with the launch against the same driver kept on the chain (sample_iters < 0).  The buffers, the comparison (floats as their
32-bit patterns: a NaN row has to match too) and the callers' pairs are those of tests/rollout_harness.py."""
import ctypes
from functools import partial

import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops
from tests import rollout_harness as H
from tests.rollout_harness import assert_same, bits, engine, ring_ptrs  # noqa: F401 (engine: a fixture)

pytestmark = pytest.mark.gpu


def Policy(od, packed, seed=0):
    return H.PolicyNet(od, 4, ops.make_cfg(obs_dim=od), packed, 100 * od + seed)


def start(p, n, cap, nan_row=None):
    """agents from the reset law (seed 4)"""
    from mpg_amd.envs import PathTrackingEnv
    return H.start(PathTrackingEnv(num_agent=n, num_future_data=p.od - 6, seed=4), p.od, 2, n, cap, nan_row=nan_row)


def run_chain(p, t, n, iters, sigma, cap, nxt, nctr, ectr):
    p.status.zero_()
    for it in range(iters):
        L.call('mpg_worker_step', ctypes.byref(p.cfg), L.ptr(p.pol), L.c_int(n), L.ptr(t['state']), L.ptr(t['obs_io']), L.c_float(sigma),
               L.c_u64(11), L.c_u64(nctr + it), L.ptr(t['act_out']), L.c_int(cap), L.c_int((nxt + it * n) % cap), *ring_ptrs(t),
               L.c_u64(4), L.c_u64(ectr + it), L.ptr(t['done_out']), L.ptr(None), L.c_int(0), L.ptr(None), L.ptr(None), L.ptr(None),
               L.ptr(None), L.stream())
    t['status'] = p.status.clone()


def run_launch(p, t, n, iters, sigma, cap, nxt, nctr, ectr):
    p.status.zero_()
    L.call('mpg_worker_rollout', ctypes.byref(p.cfg), L.ptr(p.pol), L.c_int(n), L.c_int(iters), L.ptr(t['state']), L.ptr(t['obs_io']),
           L.c_float(sigma), L.c_u64(11), L.c_u64(nctr), L.ptr(t['act_out']), L.c_int(cap), L.c_int(nxt), *ring_ptrs(t), L.c_u64(4),
           L.c_u64(ectr), L.ptr(t['done_out']), L.stream())
    t['status'] = p.status.clone()


def both(p, n, iters, sigma, nan_row=None, **where):
    """-> (chain, launch)"""
    def at_sigma(run):
        return lambda t, n, iters, *rest: run(p, t, n, iters, sigma, *rest)
    return H.both((at_sigma(run_chain), at_sigma(run_launch)), partial(start, p, nan_row=nan_row), n, iters, **where)


@pytest.mark.parametrize('packed', [False, True], ids=['strided', 'packed'])
@pytest.mark.parametrize('od', [6, 9, 16])
def test_one_launch_equals_the_chain_of_worker_steps_bit_for_bit(engine, od, packed):
    """n: half a 16-agent group, one group, a ragged third group.  iters = 1 is a single mpg_worker_step, 2 the first hand-over of the
    observations through LDS, 64 the reference's worker.  obs_dim 6 (the eight-wide input block), 9 and 16 (the 16-wide one)."""
    p = Policy(od, packed)
    for n in (8, 16, 40):
        for iters in (1, 2, 5, 64):
            for sigma in (0., 0.1):
                a, b = both(p, n, iters, sigma)
                assert_same(a, b, (n, iters, sigma))
                assert int(b['status'].item()) == 0
                w = H.touched(iters * n + 13, 5, iters * n)
                assert (b['ring_rew'][~w] == -7.).all() and (b['ring_rew'][w] != -7.).all()
                assert torch.isfinite(b['ring_obs2'][w]).all() and (b['ring_done'][w] == 1).all()   # SURVEY B-0


@pytest.mark.parametrize('od,packed', [(6, True), (9, False)])
def test_ring_wrap_inside_an_iteration_and_the_counters_carry(engine, od, packed):
    """capacity == iters * n with next_idx = capacity - 3: every slot is written once and the wrap falls inside an iteration's block;
    noise_ctr = env_ctr = 2^32 - 2: the counters' low words overflow at the third iteration"""
    p = Policy(od, packed, seed=1)
    for n, iters in ((8, 5), (40, 5), (16, 64)):
        cap = iters * n
        a, b = both(p, n, iters, 0.1, cap=cap, nxt=cap - 3, ctr=2 ** 32 - 2, ectr=2 ** 32 - 2)
        assert_same(a, b, (n, iters))
        assert (b['ring_rew'] != -7.).all() and (b['ring_done'] == 1).all()
    # the high words matter: the same start and the same low words under another high word draw other noise and other resets
    lo = start(p, 16, 5 * 16 + 13)
    run_launch(p, lo, 16, 5, 0.1, 5 * 16 + 13, 5, (2 ** 32 - 2) & 0xFFFFFFFF, (2 ** 32 - 2) & 0xFFFFFFFF)
    hi = start(p, 16, 5 * 16 + 13)
    run_launch(p, hi, 16, 5, 0.1, 5 * 16 + 13, 5, 2 ** 33 - 2, 2 ** 33 - 2)       # the same low words, another high word
    torch.cuda.synchronize()
    assert not torch.equal(bits(lo['obs_io']), bits(hi['obs_io'])) and not torch.equal(bits(lo['act_out']), bits(hi['act_out']))


@pytest.mark.parametrize('od,packed', [(6, False), (9, True)])
def test_a_nan_start_row_is_reported_and_stored_like_the_chain(engine, od, packed):
    """one agent and its observation NaN from the start: the policy pass sees the NaN observation, its action and the transition's
    reward are NaN, and both paths OR MPG_STATUS_NAN into the status word; everything - the NaN entries' bit patterns included - is
    equal.  (This does NOT reach the not-done branch: the sub-steps clamp v_x with fminf / fmaxf, a NaN v_x comes out as 1 < 2, so
    the agent is done and re-drawn like every finite one - SURVEY B-0 - and the later iterations are finite again.)"""
    p = Policy(od, packed, seed=2)
    n, iters, row = 40, 5, 21
    a, b = both(p, n, iters, 0.1, nan_row=row)
    assert_same(a, b, 'nan row')
    assert int(a['status'].item()) == int(b['status'].item()) and int(b['status'].item()) & ops.STATUS_NAN
    slot = 5 + row                                         # the row's transition of iteration 0
    assert torch.isnan(b['ring_obs'][slot]).all() and torch.isnan(b['ring_act'][slot]).all() and torch.isnan(b['ring_rew'][slot])
    keep = ~H.touched(iters * n + 13, slot, 1)
    assert not torch.isnan(b['ring_rew'][keep]).any() and torch.isfinite(b['state']).all() and (b['done_out'] == 1).all()


@pytest.mark.parametrize('od', [6, 9])
def test_repeated_launches_are_bit_identical(engine, od):
    """100 launches from one start: the hand-overs between wave 0 and the policy pass through LDS are the new thing here"""
    p = Policy(od, True, seed=3)
    n, iters, cap = 40, 5, 40 * 5 + 13
    H.assert_repeatable(lambda: start(p, n, cap), lambda t: run_launch(p, t, n, iters, 0.1, cap, 5, 7, 3), 100)


# ---- OffPolicyWorker.sample ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('future', [0, 3])
def test_worker_sample_one_launch_equals_the_loop(engine, future):
    from mpg_amd.config import default_args
    (_, _, ca), (_, _, cb) = H.worker_sample_pair(partial(default_args, 'TD3', num_agent=8, batch_size=64, num_future_data=future, seed=5,
                                                          init_seed=5))
    assert ca[0] == 16 and ca[2:] == (128, 2), (ca, cb)


# ---- native step driver ---------------------------------------------------------------------------------------------------------
def _stack(alg, per):
    from mpg_amd.buffer import PrioritizedReplayBuffer, ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import MPGLearner, TD3Learner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    args = default_args(alg, replay_batch_size=64, max_buffer_size=8192, seed=3, init_seed=3, buffer_type='priority' if per else 'normal',
                        nan_check_interval=10 ** 9)
    assert (args.num_agent, args.batch_size) == (8, 512)              # the reference's worker defaults: 64 iterations per sample
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    learner = (TD3Learner if alg == 'TD3' else MPGLearner)(PolicyWithQs, args)
    rb = (PrioritizedReplayBuffer if per else ReplayBuffer)(args, 0)
    opt = SingleProcessOffPolicyOptimizer(worker, learner, rb, None, args, sampling_interval=10)
    assert opt._fused is not None
    return opt


@pytest.mark.parametrize('alg,per', [('MPG-v2', False), ('TD3', False), ('TD3', True)], ids=['mpg_v2', 'td3', 'td3_priority'])
def test_native_driver_with_the_launch_equals_the_driver_on_the_chain(engine, alg, per):
    """25 iterations (samples at 0, 10, 20) at the reference's worker defaults: the driver that issues mpg_worker_rollout for the first
    63 (MPG-v2: the 64th pre-gathers the draw) or 64 (TD3) iterations of a sample against the same driver kept on the chain (one
    mpg_worker_step each): parameters, Adam moments, targets, ring, the trees of the prioritized pair (its mpg_per_add calls follow
    the launch, in iteration order), worker buffers, status word and counters, bit for bit.  The ring of 8192 wraps at the third
    sample."""
    H.driver_chain_pair(partial(_stack, alg, per), 64, extra=H.per_trees if per else None)


def test_native_driver_issues_one_worker_launch_per_sample():
    """the driver's own timer counts the worker's launches (slot 2): one per sample with the launch (TD3: all 64 iterations), 64 on the
    chain - the pair above does compare two different launch sequences"""
    counts = H.worker_launch_counts(partial(_stack, 'TD3', False), 64, 256)
    assert counts == [1, 64], counts
