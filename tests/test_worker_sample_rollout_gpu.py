"""mpg_worker_sample_rollout on the GPU: the one launch against the chain of mpg_normal_fill + mpg_policy_sample (with an action range:
mpg_policy_sample_squashed) + mpg_env_step_store_reset triples it replaces - and, for the plain head, against the chain of
mpg_worker_sample_step calls - from identical starts, bit for bit: env state, observations, last actions, last done flags, all five
ring arrays WHOLE (prefilled with a sentinel, so the slots nobody writes count) and the status word; its callers -
OffPolicyWorker.sample(one_launch_sample) with a stochastic policy against the loop, the native SAC driver with the launch against the
same driver kept on the chain (sample_iters < 0).  The buffers, the comparison (floats as their 32-bit patterns: a NaN row has to match
too) and the callers' pairs are those of tests/rollout_harness.py."""
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
SAMPLE_SEED, ENV_SEED = 11, 4
RANGE = 1.5
HEADS = ('plain', 'squashed')


def Policy(od, packed, head, seed=0, out_act='linear', b3=None):
    """a four-output policy network (mean | log-std).  head 'plain': the Gaussian head (no action range); 'squashed': a = RANGE
    tanh(mean + sigma eps).  Linear output (SAC's default, and what the squashed head asks for) unless out_act says otherwise.  b3:
    the last layer's bias replaced, W3 scaled by 0.1 (the heads' edges)."""
    def edges(flat):
        flat[-(4 * 256 + 4):-4] *= np.float32(0.1)
        flat[-4:] = np.asarray(b3, dtype=np.float32)
    cfg = ops.make_cfg(obs_dim=od, policy_out_activation=out_act, action_range=RANGE if head == 'squashed' else None)
    p = H.PolicyNet(od, 4, cfg, packed, 100 * od + seed, None if b3 is None else edges)
    p.sample_entry = 'mpg_policy_sample_squashed' if head == 'squashed' else 'mpg_policy_sample'
    return p


def start(p, n, cap, nan_row=None):
    """agents from the reset law (seed 4)"""
    from mpg_amd.envs import PathTrackingEnv
    return H.start(PathTrackingEnv(num_agent=n, num_future_data=p.od - 6, seed=ENV_SEED), p.od, 2, n, cap, nan_row=nan_row)


def run_chain(p, t, n, iters, cap, nxt, sctr, ectr):
    """the three entry points per iteration, as include/mpg_hip.h states the contract"""
    p.status.zero_()
    eps = torch.empty(2 * n, dtype=torch.float32, device=DEV)
    logp = torch.empty(n, dtype=torch.float32, device=DEV)
    ws = ops._ws(DEV, 0, p.sample_entry + '_workspace_bytes', p.cfg, n)
    for it in range(iters):
        L.call('mpg_normal_fill', L.c_int(2 * n), L.c_u64(SAMPLE_SEED), L.c_u64(sctr + it), L.ptr(eps), L.stream())
        L.call(p.sample_entry, ctypes.byref(p.cfg), L.ptr(p.pol), L.c_int(n), L.ptr(t['obs_io']), L.ptr(eps), L.ptr(t['act_out']), L.ptr(logp),
               L.ptr(None), *ws, L.stream())
        L.call('mpg_env_step_store_reset', L.c_int(0), L.c_int(n), L.c_int(p.od), L.ptr(t['state']), L.ptr(t['act_out']), L.c_int(cap),
               L.c_int((nxt + it * n) % cap), *ring_ptrs(t), L.c_u64(ENV_SEED), L.c_u64(ectr + it), L.ptr(t['obs_io']), L.ptr(t['done_out']),
               L.stream())
    t['status'] = p.status.clone()


def run_steps(p, t, n, iters, cap, nxt, sctr, ectr):
    """the plain head's other chain: one mpg_worker_sample_step per iteration"""
    p.status.zero_()
    for it in range(iters):
        L.call('mpg_worker_sample_step', ctypes.byref(p.cfg), L.ptr(p.pol), L.c_int(n), L.ptr(t['state']), L.ptr(t['obs_io']), L.c_u64(SAMPLE_SEED),
               L.c_u64(sctr + it), L.ptr(t['act_out']), L.ptr(None), L.c_int(cap), L.c_int((nxt + it * n) % cap), *ring_ptrs(t),
               L.c_u64(ENV_SEED), L.c_u64(ectr + it), L.ptr(t['done_out']), L.stream())
    t['status'] = p.status.clone()


def run_launch(p, t, n, iters, cap, nxt, sctr, ectr):
    p.status.zero_()
    L.call('mpg_worker_sample_rollout', ctypes.byref(p.cfg), L.ptr(p.pol), L.c_int(n), L.c_int(iters), L.ptr(t['state']), L.ptr(t['obs_io']),
           L.c_u64(SAMPLE_SEED), L.c_u64(sctr), L.ptr(t['act_out']), L.c_int(cap), L.c_int(nxt), *ring_ptrs(t), L.c_u64(ENV_SEED),
           L.c_u64(ectr), L.ptr(t['done_out']), L.stream())
    t['status'] = p.status.clone()


def both(p, n, iters, nan_row=None, steps=False, **where):
    """-> (chain, launch[, chain of mpg_worker_sample_step])"""
    runs = (run_chain, run_launch) + ((run_steps,) if steps else ())
    return H.both([partial(run, p) for run in runs], partial(start, p, nan_row=nan_row), n, iters, **where)


@pytest.mark.parametrize('packed', [False, True], ids=['strided', 'packed'])
@pytest.mark.parametrize('od', [6, 9, 16])
@pytest.mark.parametrize('head', HEADS)
def test_one_launch_equals_the_chain_of_draw_sample_and_env_launches_bit_for_bit(engine, head, od, packed):
    """n: half a 16-agent group, one group, a ragged third group.  iters = 1 is a single triple, 2 the first hand-over of the
    observations through LDS, 64 the reference's worker.  obs_dim 6 (the eight-wide input block), 9 and 16 (the 16-wide one).  The
    plain head also against `iters` x mpg_worker_sample_step."""
    p = Policy(od, packed, head)
    for n in (8, 16, 40):
        for iters in (1, 2, 5, 64):
            out = both(p, n, iters, steps=head == 'plain')
            a, b = out[:2]
            assert_same(a, b, (n, iters))
            if head == 'plain':
                assert_same(out[2], b, (n, iters, 'mpg_worker_sample_step'))
            assert int(b['status'].item()) == 0
            w = H.touched(iters * n + 13, 5, iters * n)
            assert (b['ring_rew'][~w] == -7.).all() and (b['ring_rew'][w] != -7.).all()
            assert (b['ring_done'][~w] == 0xAB).all() and (b['ring_done'][w] == 1).all()                       # SURVEY B-0
            for k in ('ring_obs', 'ring_act', 'ring_obs2'):
                assert (b[k][~w] == -7.).all() and torch.isfinite(b[k][w]).all(), k
            if head == 'squashed':
                assert (b['ring_act'][w].abs() <= RANGE).all()


def test_the_output_activation_reaches_all_four_logits(engine):
    """PathTracking's deterministic default, a tanh output, under the plain head: tanh on the means AND on the log-std columns"""
    for od, packed in ((6, True), (9, False)):
        p = Policy(od, packed, 'plain', seed=4, out_act='tanh')
        a, b, c = both(p, 40, 5, steps=True)
        assert_same(a, b, (od, 'tanh output'))
        assert_same(c, b, (od, 'tanh output', 'mpg_worker_sample_step'))


@pytest.mark.parametrize('od,packed', [(6, True), (9, False)])
@pytest.mark.parametrize('head', HEADS)
def test_ring_wrap_inside_an_iteration_and_the_counters_carry(engine, head, od, packed):
    """capacity == iters * n with next_idx = capacity - 3: every slot is written once and the wrap falls inside an iteration's block;
    sample_ctr = env_ctr = 2^32 - 2: the counters' low words overflow at the third iteration"""
    p = Policy(od, packed, head, seed=1)
    for n, iters in ((8, 5), (40, 5), (16, 64)):
        cap = iters * n
        a, b = both(p, n, iters, cap=cap, nxt=cap - 3, ctr=2 ** 32 - 2, ectr=2 ** 32 - 2)
        assert_same(a, b, (n, iters))
        assert (b['ring_rew'] != -7.).all() and (b['ring_done'] == 1).all()
    # the high words matter: the same start and the same low words under another high word draw other actions and other resets
    lo = start(p, 16, 5 * 16 + 13)
    run_launch(p, lo, 16, 5, 5 * 16 + 13, 5, (2 ** 32 - 2) & 0xFFFFFFFF, (2 ** 32 - 2) & 0xFFFFFFFF)
    hi = start(p, 16, 5 * 16 + 13)
    run_launch(p, hi, 16, 5, 5 * 16 + 13, 5, 2 ** 33 - 2, 2 ** 33 - 2)            # the same low words, another high word
    torch.cuda.synchronize()
    assert not torch.equal(bits(lo['obs_io']), bits(hi['obs_io'])) and not torch.equal(bits(lo['act_out']), bits(hi['act_out']))


@pytest.mark.parametrize('packed', [False, True], ids=['strided', 'packed'])
@pytest.mark.parametrize('head', HEADS)
def test_the_heads_edges_clipped_log_std_and_saturated_tanh(engine, head, packed):
    """a last-layer bias of (12, -12, -8, 3) over a damped W3: the first component's log-std lies below -5 (sigma = exp(-5)), the
    second's above 1 (sigma = e) - shown on the chain's own logits - and, squashed, u = 12 + exp(-5) eps is beyond where float32 tanh
    is exactly 1: the first action is exactly +RANGE on every row, the second -RANGE wherever eps < 1 (u < -12 + e).  Plain: the first
    action of iteration 0 IS mean + float32(exp(-5)) * eps, product and sum rounded separately.  Launch against chain bit for bit."""
    n, iters, od = 40, 5, 9
    p = Policy(od, packed, head, seed=7, b3=(12., -12., -8., 3.))
    obs0 = start(p, n, 1)['obs_io']
    eps0 = ops.normal_fill(2 * n, SAMPLE_SEED, 7, DEV).view(n, 2)
    sample = ops.policy_sample_squashed if head == 'squashed' else ops.policy_sample
    act0, _, logits = sample(p.cfg, p.pol, obs0, eps0, want_logits=True)
    assert (logits[:, 2] < -5.).all() and (logits[:, 3] > 1.).all(), logits
    assert (logits[:, 0] > 11.).all() and (logits[:, 1] < -11.).all(), logits
    a, b = both(p, n, iters)
    assert_same(a, b, 'edges')
    assert int(a['status'].item()) == int(b['status'].item()) and not int(b['status'].item()) & ops.STATUS_NAN
    assert torch.equal(bits(a['ring_act'][5:5 + n]), bits(act0))                   # the chain's iteration 0 is that call
    acts = a['ring_act'][5:5 + iters * n]
    if head == 'squashed':
        assert (acts[:, 0] == RANGE).all() and (acts[:, 1] == -RANGE).any() and (acts.abs() <= RANGE).all()
        assert (acts[:n, 1][eps0[:, 1] < 1.] == -RANGE).all()
    else:
        lo = torch.tensor(np.float32(np.exp(np.float64(-5.))), device=DEV)
        assert torch.equal(bits(acts[:n, 0]), bits(lo * eps0[:, 0] + logits[:, 0]))
        hi = torch.tensor(np.float32(np.exp(np.float64(1.))), device=DEV)
        assert torch.equal(bits(acts[:n, 1]), bits(hi * eps0[:, 1] + logits[:, 1]))


@pytest.mark.parametrize('od,packed', [(6, False), (9, True)])
@pytest.mark.parametrize('head', HEADS)
def test_a_nan_start_row_is_reported_and_stored_like_the_chain(engine, head, od, packed):
    """one agent and its observation NaN from the start: the policy pass sees the NaN observation, its logits, action and the
    transition's reward are NaN, and both paths OR MPG_STATUS_NAN into the status word; everything - the NaN entries' bit patterns
    included - is equal.  (The agent is done and re-drawn like every finite one - SURVEY B-0 - so the later iterations are finite.)"""
    p = Policy(od, packed, head, seed=2)
    n, iters, row = 40, 5, 21
    a, b = both(p, n, iters, nan_row=row)
    assert_same(a, b, 'nan row')
    assert int(a['status'].item()) == int(b['status'].item()) and int(b['status'].item()) & ops.STATUS_NAN
    slot = 5 + row                                         # the row's transition of iteration 0
    assert torch.isnan(b['ring_obs'][slot]).all() and torch.isnan(b['ring_act'][slot]).all() and torch.isnan(b['ring_rew'][slot])
    keep = ~H.touched(iters * n + 13, slot, 1)
    assert not torch.isnan(b['ring_rew'][keep]).any() and torch.isfinite(b['state']).all() and (b['done_out'] == 1).all()


@pytest.mark.parametrize('head', HEADS)
def test_repeated_launches_are_bit_identical(engine, head):
    """ten launches from one start: the hand-overs through LDS - observations to the pass, logits and actions within wave 0"""
    p = Policy(9, True, head, seed=3)
    n, iters, cap = 40, 5, 40 * 5 + 13
    H.assert_repeatable(lambda: start(p, n, cap), lambda t: run_launch(p, t, n, iters, cap, 5, 7, 3), 10)


# ---- OffPolicyWorker.sample ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stack', ['sac-0', 'sac-3', 'squashed'])
def test_worker_sample_one_launch_equals_the_loop(engine, stack):
    from mpg_amd.config import default_args
    kw = dict(squashed_head=True, action_range=RANGE) if stack == 'squashed' else dict(num_future_data=int(stack[-1]))

    def make(**more):
        args = default_args('SAC', num_agent=8, batch_size=64, seed=5, init_seed=5, **kw, **more)
        assert args.explore_sigma is None and args.env_id == 'PathTracking-v0'
        return args
    (wa, ba, ca), (wb, _, cb) = H.worker_sample_pair(make, extra_counters=True)
    for w in (wa, wb):
        assert not w.policy_with_value.deterministic_policy and w.policy_with_value.squashed_head == (stack == 'squashed')
    assert ca[0] == 16 and ca[2:4] == (128, 2), (ca, cb)
    if stack == 'squashed':
        assert all(x[1].abs().max().item() <= RANGE for x in ba)


# ---- native SAC driver -----------------------------------------------------------------------------------------------------------
def _stack(auto, **over):
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import SACLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    more = dict(alpha='auto', target_entropy=-2., delay_update=2) if auto else {}
    # the start fills 3072 rows of the ring's 4096 (six samples of 512); the third sample of the run wraps it
    args = default_args('SAC', seed=3, init_seed=3, max_buffer_size=4096, nan_check_interval=10 ** 9, **more, **over)
    assert (args.num_agent, args.batch_size, args.replay_batch_size, args.replay_starts) == (8, 512, 256, 3000)
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    learner = SACLearner(PolicyWithQs, args)
    opt = SingleProcessOffPolicyOptimizer(worker, learner, ReplayBuffer(args, 0), None, args, sampling_interval=10, native_sac=True)
    assert opt._fused is not None and opt._fused.c.learner_version == 7 and opt._fused.c.sample_iters == 64
    return opt


def sac_state(auto, opt):
    return [opt.worker.policy_with_value.alpha_state] if auto else [], (opt.num_sampled_steps,)


@pytest.mark.parametrize('K', [0, 3], ids=['obs6', 'obs9'])
@pytest.mark.parametrize('auto', [False, True], ids=['fixed-alpha', 'auto-alpha'])
def test_native_driver_with_the_launch_equals_the_driver_on_the_chain(engine, auto, K):
    """25 iterations (samples at 0, 10, 20) at the reference's worker defaults, B = 256: the driver that issues mpg_worker_sample_rollout
    for the 64 iterations of a sample against the same driver kept on the chain (one mpg_worker_sample_step each): parameters, Adam
    moments, targets, ring, worker buffers, env state, gradients, status word, the temperature's state and counters, bit for bit.  The
    ring of 4096 wraps at the third sample.  Both widths the driver's rule was measured at: six-entry
    observations and the 16-wide form."""
    (a, ca), _ = H.driver_chain_pair(partial(_stack, auto, num_future_data=K), 64, extra=partial(sac_state, auto))
    assert ca[2:4] == ((3072 + 3 * 512) % 4096, 4096), ca              # it wrapped
    assert all(torch.isfinite(t).all() for t in a[:4])


@pytest.mark.parametrize('K', [0, 3], ids=['obs6', 'obs9'])
@pytest.mark.parametrize('auto', [False, True], ids=['fixed-alpha', 'auto-alpha'])
def test_native_driver_issues_one_worker_launch_per_sample(auto, K):
    """the driver's own timer counts the worker's launches (slot 2): one per sample with the launch, 64 on the chain - the pair above
    does compare two different launch sequences"""
    counts = H.worker_launch_counts(partial(_stack, auto, num_future_data=K), 64, 256)
    assert counts == [1, 64], counts
