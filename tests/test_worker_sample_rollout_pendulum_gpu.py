"""mpg_worker_sample_rollout_pendulum on the GPU: the one launch against the chain of mpg_normal_fill + mpg_policy_sample_squashed +
mpg_env_step_store_reset triples it replaces, from identical starts, bit for bit - env state, observations, last actions, last done
flags, all five ring arrays WHOLE (prefilled with a sentinel, so the slots nobody writes count) and the status word; its caller -
OffPolicyWorker.sample (one_launch_sample) with the tanh-squashed SAC policy against the loop, alone and under
SingleProcessOffPolicyOptimizer.  The buffers, the comparison (floats as their 32-bit patterns: a NaN row has to match too) and the
worker pair are those of tests/rollout_harness.py; the policy here is the SAMPLED one: a = 3 tanh(mean + exp(clip(log_std)) eps)."""
import ctypes
from functools import partial

import numpy as np
import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops
from tests import rollout_harness as H
from tests.rollout_harness import DEV, assert_same, bits, engine, ring_ptrs  # noqa: F401 (engine: a fixture)

pytestmark = pytest.mark.gpu
ENV_ID = 'InvertedPendulumConti-v0'
SAMPLE_SEED, ENV_SEED = 11, 4
GENTLE_LOG_STD = -3.5            # sigma = exp(-3.5) = 0.030 (test_both_branches_of_done_in_one_run says what the oracle showed)


def Policy(packed, seed=0, gentle=False, last_scale=None):
    """the pendulum's policy network (4 inputs, mean | log-std) under a linear output with action_range 3.  gentle: the last layer
    scaled by 0.01 and the log-std bias at GENTLE_LOG_STD - means of a few hundredths under a sigma of 0.03, so that an agent near the
    upright stays up for many iterations and falls on its own.  last_scale: the last layer scaled UP (the head's edges)."""
    def last_layer(flat):
        if gentle:
            flat[-(2 * 256 + 2):] *= np.float32(0.01)     # W3 [256][2] and b3 [2]
            flat[-1] = np.float32(GENTLE_LOG_STD)         # b3[1]: the log-std column's bias
        if last_scale is not None:
            flat[-(2 * 256 + 2):] *= np.float32(last_scale)
    cfg = ops.make_cfg(ENV_ID)
    assert cfg.action_range == 3.0
    return H.PolicyNet(4, 2, cfg, packed, 400 + seed, last_layer)


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
    return H.start(InvertedPendulumContiEnv(num_agent=n, seed=ENV_SEED), 4, 1, n, cap, init_obs, nan_row)


def run_chain(p, t, n, iters, cap, nxt, sctr, ectr):
    """the three entry points per iteration, as include/mpg_hip.h states the contract"""
    p.status.zero_()
    eps = torch.empty(n, dtype=torch.float32, device=DEV)
    logp = torch.empty(n, dtype=torch.float32, device=DEV)
    ws = ops._ws(DEV, 0, 'mpg_policy_sample_squashed_workspace_bytes', p.cfg, n)
    for it in range(iters):
        L.call('mpg_normal_fill', L.c_int(n), L.c_u64(SAMPLE_SEED), L.c_u64(sctr + it), L.ptr(eps), L.stream())
        L.call('mpg_policy_sample_squashed', ctypes.byref(p.cfg), L.ptr(p.pol), L.c_int(n), L.ptr(t['obs_io']), L.ptr(eps), L.ptr(t['act_out']),
               L.ptr(logp), L.ptr(None), *ws, L.stream())
        L.call('mpg_env_step_store_reset', L.c_int(1), L.c_int(n), L.c_int(4), L.ptr(t['state']), L.ptr(t['act_out']), L.c_int(cap),
               L.c_int((nxt + it * n) % cap), *ring_ptrs(t), L.c_u64(ENV_SEED), L.c_u64(ectr + it), L.ptr(t['obs_io']), L.ptr(t['done_out']),
               L.stream())
    t['status'] = p.status.clone()


def run_launch(p, t, n, iters, cap, nxt, sctr, ectr):
    p.status.zero_()
    L.call('mpg_worker_sample_rollout_pendulum', ctypes.byref(p.cfg), L.ptr(p.pol), L.c_int(n), L.c_int(iters), L.ptr(t['state']),
           L.ptr(t['obs_io']), L.c_u64(SAMPLE_SEED), L.c_u64(sctr), L.ptr(t['act_out']), L.c_int(cap), L.c_int(nxt), *ring_ptrs(t),
           L.c_u64(ENV_SEED), L.c_u64(ectr), L.ptr(t['done_out']), L.stream())
    t['status'] = p.status.clone()


def both(p, n, iters, init_obs=None, nan_row=None, **where):
    """-> (chain, launch)"""
    return H.both((partial(run_chain, p), partial(run_launch, p)), partial(start, init_obs=init_obs, nan_row=nan_row), n, iters, **where)


@pytest.mark.parametrize('packed', [False, True], ids=['strided', 'packed'])
def test_one_launch_equals_the_chain_of_draw_sample_and_env_launches_bit_for_bit(engine, packed):
    """n: one agent (the reference's default: one live lane), half a 16-agent group, one group, a ragged third group - n = 40 holds every
    (Philox block, pair, parity) position of the draw, over several blocks.  iters = 1 is a single triple, 2 the first hand-over of the
    observations through LDS, 64 and 1 x 512 long enough for agents to fall."""
    p = Policy(packed)
    for n, all_iters in ((1, (1, 2, 5, 64, 512)), (8, (1, 2, 5, 64)), (16, (1, 2, 5, 64)), (40, (1, 2, 5, 64))):
        for iters in all_iters:
            a, b = both(p, n, iters)
            assert_same(a, b, (n, iters))
            assert int(b['status'].item()) == 0
            w = H.touched(iters * n + 13, 5, iters * n)
            assert (b['ring_rew'][~w] == -7.).all() and (b['ring_rew'][w] != -7.).all()
            assert (b['ring_done'][~w] == 0xAB).all() and (b['ring_done'][w] <= 1).all()
            assert (b['ring_act'][~w] == -7.).all() and (b['ring_act'][w].abs() <= 3.).all()
            assert torch.isfinite(b['ring_obs'][w]).all() and torch.isfinite(b['ring_obs2'][w]).all()


@pytest.mark.parametrize('packed', [False, True], ids=['strided', 'packed'])
def test_both_branches_of_done_in_one_run(engine, packed):
    """agents that live in a lane's registers for many iterations, fall, are re-drawn and go on - beside agents that fall at once.
    The gentle policy's log-std bias was picked on the CPU: oracle.mpg_oracle.InvertedPendulumContiOracle (float64) from these starts
    under this policy (a = 3 tanh(mean + sigma eps), sigma = exp(-3.5) = 0.0302 on every row) and three standard-normal draws of its
    own showed every reset-law agent alive through iterations 0 and 1, its first fall between iterations 12 and 34 (of 64), all 20
    alive again in the iteration behind their reset, and every odd agent done at iteration 0 (biases -3 and -4 gave 10 .. 38 and
    14 .. 36).  The conditions are asserted on the DEVICE's own ring rows, so an all-done or all-alive run cannot pass."""
    n, iters = 40, 64
    for gentle in (True, False):
        p = Policy(packed, gentle=gentle)
        a, b = both(p, n, iters, init_obs=mixed_starts(n))
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


def wide_starts(n):
    """starts all over the env's live region (|p| < 1.9, |theta| < 0.19, velocities up to 5): under obs_scale the reset law's
    observations are all but one point to the network; these spread its logits"""
    r = np.random.Generator(np.random.PCG64(9))
    return (r.uniform(-1, 1, (n, 4)) * np.array([1.9, 0.19, 5., 5.])).astype(np.float32)


@pytest.mark.parametrize('packed', [False, True], ids=['strided', 'packed'])
def test_the_heads_edges_saturated_tanh_and_clipped_log_std(engine, packed):
    """the last layer scaled by 60 on wide starts: means beyond +-12 on both sides, where float32 tanh(mean + sigma eps) is exactly +-1
    under a sigma of at most e (actions exactly +-3), and log-std logits on both sides of [-5, 1] as well as inside it (the clip's two
    bounds) - shown on the start observations' own logits and on the device's ring; the launch equals the chain bit for bit, every
    action lies within [-3, 3], and whatever the scaled weights report in the status word (the activation range, on the split engine)
    the launch reports too"""
    n, iters = 40, 5
    p = Policy(packed, seed=7, last_scale=60.)
    obs0 = torch.as_tensor(wide_starts(n)).to(DEV)
    _, _, logits = ops.policy_sample_squashed(p.cfg, p.pol, obs0, torch.zeros(n, 1, device=DEV), want_logits=True)
    mean, log_std = logits[:, 0], logits[:, 1]
    assert (mean < -12.).any() and (mean > 12.).any() and (mean.abs() < 5.).any(), mean
    assert (log_std < -5.).any() and (log_std > 1.).any() and ((log_std > -5.) & (log_std < 1.)).any(), log_std
    a, b = both(p, n, iters, init_obs=wide_starts(n))
    assert_same(a, b, 'edges')
    assert int(a['status'].item()) == int(b['status'].item()) and not int(b['status'].item()) & ops.STATUS_NAN
    acts = b['ring_act'][5:5 + iters * n]
    assert (acts.abs() <= 3.).all() and (acts == 3.).any() and (acts == -3.).any() and (acts.abs() < 3.).any()


@pytest.mark.parametrize('packed', [True, False], ids=['packed', 'strided'])
def test_ring_wrap_inside_an_iteration_and_the_counters_carry(engine, packed):
    """capacity == iters * n with next_idx = capacity - 3: every slot is written once and the wrap falls inside an iteration's block;
    sample_ctr = env_ctr = 2^32 - 2: the counters' low words overflow at the third iteration"""
    p = Policy(packed, seed=1)
    for n, iters in ((8, 5), (40, 5), (16, 64), (1, 64)):
        cap = iters * n
        a, b = both(p, n, iters, cap=cap, nxt=cap - 3, ctr=2 ** 32 - 2, ectr=2 ** 32 - 2, init_obs=mixed_starts(n))
        assert_same(a, b, (n, iters))
        assert (b['ring_rew'] != -7.).all() and (b['ring_done'] <= 1).all()
    # the high words matter: the same start and the same low words under another high word draw other actions, and - the odd agents
    # fall at the first step - other reset states
    n, iters, cap = 16, 5, 5 * 16 + 13
    lo = start(n, cap, mixed_starts(n))
    run_launch(p, lo, n, iters, cap, 5, (2 ** 32 - 2) & 0xFFFFFFFF, (2 ** 32 - 2) & 0xFFFFFFFF)
    hi = start(n, cap, mixed_starts(n))
    run_launch(p, hi, n, iters, cap, 5, 2 ** 33 - 2, 2 ** 33 - 2)            # the same low words, another high word
    torch.cuda.synchronize()
    assert not torch.equal(bits(lo['act_out']), bits(hi['act_out']))
    assert not torch.equal(bits(lo['ring_act'][5:5 + n]), bits(hi['ring_act'][5:5 + n]))
    assert (lo['ring_done'][5 + 1:5 + n:2] == 1).all() and (hi['ring_done'][5 + 1:5 + n:2] == 1).all()
    first_reset = slice(5 + n + 1, 5 + 2 * n, 2)              # iteration 1's observations of the odd agents: their reset states
    assert not torch.equal(bits(lo['ring_obs'][first_reset]), bits(hi['ring_obs'][first_reset]))


@pytest.mark.parametrize('packed', [False, True], ids=['strided', 'packed'])
def test_a_nan_start_row_is_reported_and_stored_like_the_chain(engine, packed):
    """one agent and its observation NaN from the start: the policy pass sees the NaN observation, its logits, action and transition
    are NaN, and both paths OR MPG_STATUS_NAN into the status word; everything - the NaN entries' bit patterns included - is equal.  A
    NaN state is done (neither |p| < 2 nor |theta| <= 0.2 holds), so the agent is re-drawn and every other row is finite."""
    p = Policy(packed, seed=2)
    n, iters, row = 40, 5, 21
    a, b = both(p, n, iters, nan_row=row)
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
    """100 launches from one start: the hand-overs through LDS - observations to the pass, logits to the env lanes - are the new thing"""
    p = Policy(True, seed=3)
    n, iters, cap = 40, 5, 40 * 5 + 13
    H.assert_repeatable(lambda: start(n, cap, mixed_starts(n)), lambda t: run_launch(p, t, n, iters, cap, 5, 7, 3), 100)


# ---- OffPolicyWorker.sample ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('num_agent', [1, 8])
def test_worker_sample_one_launch_equals_the_loop(engine, num_agent):
    from mpg_amd.config import default_args

    def make(**more):
        args = default_args('SAC', env_id=ENV_ID, squashed_head=True, num_agent=num_agent, batch_size=64, seed=5, init_seed=5, **more)
        assert args.action_range == 3.0 and args.explore_sigma is None
        return args
    (wa, ba, ca), (wb, _, cb) = H.worker_sample_pair(make, extra_counters=True)
    for w in (wa, wb):
        assert w.policy_with_value.squashed_head and not w.policy_with_value.deterministic_policy
    assert ca[0] == 2 * (64 // num_agent) and ca[2:4] == (128, 2), (ca, cb)
    assert all(x[1].abs().max().item() <= 3.0 for x in ba)


# ---- the loop (the _stack of tests/test_sac_tanh_gpu.py section 8, restated) -------------------------------------------------------
def _stack(auto, **more):
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import SACLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    extra = dict(alpha='auto', target_entropy=-1., delay_update=2) if auto else {}
    # a ring of 256 rows under six samples of 64 behind the two that start it: it wraps inside the run
    args = default_args('SAC', env_id=ENV_ID, seed=5, squashed_head=True, buffer_type='normal', num_agent=8, batch_size=64,
                        replay_batch_size=64, replay_starts=128, max_buffer_size=256, **extra, **more)
    assert args.action_range == 3.0
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    learner = SACLearner(PolicyWithQs, args)
    opt = SingleProcessOffPolicyOptimizer(worker, learner, ReplayBuffer(args, 0), None, args, sampling_interval=2)
    assert opt._fused is None and worker.policy_with_value.squashed_head
    return opt


def _state(opt):
    pw, rb, w, ln = opt.worker.policy_with_value, opt.replay_buffer, opt.worker, opt.learner
    torch.cuda.synchronize()
    tensors = [t.clone() for t in (pw.params, pw.targets, pw.m, pw.v, rb.obs, rb.act, rb.rew, rb.obs2, rb.done, w.obs, w.env._state, pw.status)]
    if pw.auto_alpha:
        tensors.append(pw.alpha_state.clone())
    counters = (dict(pw.opt_steps), rb._next_idx, len(rb), rb.replay_times, w._noise_ctr, w.env._ctr, ln.counter, pw._sample_ctr,
                opt.num_sampled_steps, w.num_sample, w.sample_times)
    return tensors, counters


@pytest.mark.parametrize('auto', [False, True], ids=['fixed-alpha', 'auto-alpha'])
def test_the_loop_with_the_launch_equals_the_loop_without(engine, auto):
    """12 iterations of SingleProcessOffPolicyOptimizer with the squashed SACLearner, 8 agents x 8 iterations per sample, the worker
    on the one launch against the worker on its loop: parameters, targets, Adam moments, replay arrays, worker observations, env state,
    status word, the temperature's state and every counter, bit for bit"""
    out = []
    for one in (False, True):
        opt = _stack(auto, **(dict(one_launch_sample=True) if one else {}))
        for _ in range(12):
            opt.step()
        out.append(_state(opt))
    (ta, ca), (tb, cb) = out
    assert ca == cb, (ca, cb)
    assert ca[2] == 256 and ca[4] == 8 * 8 and ca[8] == 8 * 64          # the ring is full (it wrapped); 8 samples of 8 iterations
    assert all(torch.isfinite(t).all() for t in ta[:4])
    assert len(ta) == (13 if auto else 12)
    for k, (x, y) in enumerate(zip(ta, tb)):
        assert x.dtype == y.dtype and torch.equal(bits(x), bits(y)), k
