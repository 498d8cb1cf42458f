"""SAC's two native pieces on the GPU.  mpg_worker_sample_step - the stochastic worker step in ONE launch - against the three calls it
replaces (mpg_normal_fill, mpg_policy_sample, mpg_env_step_store_reset), bit for bit: actions, log-densities, the five ring arrays, env
state, next observations, done flags and the policy's status word.  The native step (mpg_sac_step_begin, learner_version 7, taken with
SingleProcessOffPolicyOptimizer(native_sac=True)) against the method-by-method path: parameters, targets, Adam moments, ring, worker
observations, counters and statistics, also with stock methods in between and across a checkpoint.  Both engines."""
import functools

import numpy as np
import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops
from tests.golden_inputs import mlp_weights_flat

pytestmark = pytest.mark.gpu
DEV = 'cuda'
STATUS_NAN = ops.STATUS_NAN


def bits(t):
    t = t.contiguous()
    return t if t.dtype in (torch.uint8, torch.int32) else t.view(torch.int32)


@pytest.fixture(params=['split', 'f32'])
def engine(request):
    with L.engine(request.param):
        yield request.param


# ---- 1 - 3: the launch against the sequence ---------------------------------------------------------------------------------------
SAMPLE_KEY, ENV_KEY = (0x1234567 << 20) + 99, 77      # (a sample seed with bits in both halves of the 64-bit key)


@functools.lru_cache(maxsize=None)
def policy_weights(od):
    """an output layer as in tests/test_sac_gpu.py::test_worker_samples_from_the_stochastic_policy, spread further: the log-std columns
    scaled and shifted so that sigma varies over the agents and, with a linear output, some logits sit on either side of [-5, 1]
    (computed once per width and never written to)"""
    rng = np.random.Generator(np.random.PCG64(1100 + od))
    flat = mlp_weights_flat(rng, od, 4)
    flat[-(256 * 4 + 4):-4].reshape(256, 4)[:, 2:] *= 30.0
    flat[-2:] += np.float32(0.5)
    flat.setflags(write=False)
    return flat


class Case(object):
    """n agents after env.reset(), a policy, a ring whose slots [next_idx, next_idx + n) wrap past its end, a status word"""

    def __init__(self, n, od, act, cache, nan_row=None):
        from mpg_amd.envs import PathTrackingEnv
        self.n, self.od = n, od
        self.cfg = ops.make_cfg(obs_dim=od, policy_out_activation=act)
        self.params = torch.as_tensor(policy_weights(od).copy()).to(DEV)
        self.status = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.cfg.status = self.status.data_ptr()
        if cache:
            self.wc = ops.WeightCache(self.params, [(od, 4)])
            self.cfg.wcache[0] = self.wc.pointer
        env = PathTrackingEnv(num_future_data=od - 6, num_agent=n, seed=41 + n)
        self.obs0 = env.reset().clone()
        if nan_row is not None:
            self.obs0[nan_row, 1] = float('nan')
        self.state0 = env._state.clone()
        self.capacity = n + 5
        self.next_idx = self.capacity - 3              # three rows at the end of the ring, the others from slot 0 on
        torch.cuda.synchronize()

    def fresh(self):
        f = dict(dtype=torch.float32, device=DEV)
        c = self.capacity
        ring = (torch.full((c, self.od), -7., **f), torch.full((c, 2), -7., **f), torch.full((c,), -7., **f), torch.full((c, self.od), -7., **f),
                torch.full((c,), 9, dtype=torch.uint8, device=DEV))
        self.status.zero_()
        return self.state0.clone(), self.obs0.clone(), ring, torch.full((self.n,), 9, dtype=torch.uint8, device=DEV)

    def sequence(self, ctr=5):
        state, obs, ring, done = self.fresh()
        n = self.n
        eps = ops.normal_fill(2 * n, SAMPLE_KEY, ctr, DEV).view(n, 2)
        act, logp, logits = ops.policy_sample(self.cfg, self.params, obs, eps, want_logits=True)
        L.call('mpg_env_step_store_reset', L.c_int(0), L.c_int(n), L.c_int(self.od), L.ptr(state), L.ptr(act), L.c_int(self.capacity),
               L.c_int(self.next_idx), *[L.ptr(r) for r in ring], L.c_u64(ENV_KEY), L.c_u64(3), L.ptr(obs), L.ptr(done), L.stream())
        return [act, logp, *ring, state, obs, done, self.status.clone()], logits

    def launch(self, ctr=5, want_logp=True):
        state, obs, ring, done = self.fresh()
        act, logp = ops.worker_sample_step(self.cfg, self.params, state, obs, SAMPLE_KEY, ctr, ring, self.capacity, self.next_idx, ENV_KEY, 3,
                                           want_logp=want_logp, done_out=done)
        return [act, logp, *ring, state, obs, done, self.status.clone()]


NAMES = ('act_out', 'logp_out', 'ring_obs', 'ring_act', 'ring_rew', 'ring_obs2', 'ring_done', 'env state', 'obs_io', 'done_out', 'status')


def same(a, b, where):
    for nm, x, y in zip(NAMES, a, b):
        if x is None or y is None:
            continue
        assert x.shape == y.shape and torch.equal(bits(x), bits(y)), (where, nm, (bits(x) != bits(y)).sum().item())


@pytest.mark.parametrize('act', ['linear', 'tanh'])
@pytest.mark.parametrize('cache', [False, True], ids=['strided', 'packed'])
def test_one_launch_equals_the_three_calls_bit_for_bit(engine, cache, act):
    """n = 8: less than a group; 16: one group; 40: a ragged last group; 272: more than 256 rows (17 groups).  obs_dim 6 (the six-wide
    instantiation), 9 and 16 (the 16-wide one, partly and wholly filled)"""
    for od in (6, 9, 16):
        for n in (8, 16, 40, 272):
            c = Case(n, od, act, cache)
            seq, logits = c.sequence()
            one = c.launch()
            where = (engine, cache, act, od, n)
            ls = logits[:, 2:]
            sigma = torch.exp(torch.clamp(ls, -5., 1.))
            assert sigma.max().item() > 2 * sigma.min().item(), where                        # sigma varies over the agents
            if act == 'linear' and n >= 40:                                                   # (a tanh output cannot leave the clip)
                assert (ls > 1).any() and (ls < -5).any() and ((ls > -5) & (ls < 1)).any(), where
            # the sequence did what the case is about: wrapped ring rows written, the others untouched, nothing reported
            ring_act = seq[3]
            assert (ring_act[c.next_idx:] != -7.).all() and (ring_act[:n - 3] != -7.).all() and (ring_act[n - 3:c.next_idx] == -7.).all(), where
            assert torch.equal(ring_act[c.next_idx:], seq[0][:3]) and seq[10].item() == 0, where
            assert torch.isfinite(seq[0]).all() and torch.isfinite(seq[1]).all(), where
            same(seq, one, where)
            if n == 40:                                                                       # logp_out = NULL: everything else as before
                same(seq, c.launch(want_logp=False), where + ('no logp',))
            if n == 16:                                                                       # another counter: another draw
                assert not torch.equal(c.launch(ctr=6)[0], one[0]), where


@pytest.mark.parametrize('od', [6, 9])
def test_a_nan_observation_sets_the_same_status_bits(engine, od):
    c = Case(40, od, 'linear', True, nan_row=17)
    seq, _ = c.sequence()
    one = c.launch()
    assert seq[10].item() & STATUS_NAN, 'the sequence reports the NaN row (k_forward)'
    assert torch.isnan(seq[0][17]).all() and torch.isfinite(seq[0][:17]).all() and torch.isfinite(seq[0][18:]).all()
    same(seq, one, ('nan', engine, od))


def test_a_hundred_launches_are_bit_identical(engine):
    c = Case(272, 9, 'linear', True)
    first = c.launch()
    for i in range(100):
        same(first, c.launch(), ('repeat', i))


# ---- 4 - 7: the native step ---------------------------------------------------------------------------------------------------------
def _stack(native, seed=0, interval=10, **kw):
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import SACLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    args = default_args('SAC', seed=seed, **kw)
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    learner = SACLearner(PolicyWithQs, args)
    more = dict(native_sac=True) if native else {}           # the method path is built WITHOUT the keyword
    opt = SingleProcessOffPolicyOptimizer(worker, learner, ReplayBuffer(args, 0), None, args, sampling_interval=interval, **more)
    assert (opt._fused is not None) == native
    return opt


def _state(opt):
    """tests/test_sac_gpu.py::_state"""
    pw, rb, w, ln = opt.worker.policy_with_value, opt.replay_buffer, opt.worker, opt.learner
    torch.cuda.synchronize()
    tensors = [t.clone() for t in (pw.params, pw.targets, pw.m, pw.v, rb.obs, rb.act, rb.rew, rb.obs2, rb.done, w.obs)]
    counters = (dict(pw.opt_steps), rb._next_idx, len(rb), rb.replay_times, w._noise_ctr, w.env._ctr, ln.counter, pw._sample_ctr,
                opt.num_sampled_steps)
    return tensors, counters


def _equal_states(a, b):
    (ta, ca), (tb, cb) = a, b
    assert ca == cb, (ca, cb)
    for i, (x, y) in enumerate(zip(ta, tb)):
        assert torch.equal(bits(x), bits(y)), i


@pytest.mark.parametrize('K', [0, 3])
@pytest.mark.parametrize('reuse', [1, 3])
def test_native_step_equals_method_by_method_path(engine, reuse, K):
    """learner_version 7 enqueues what the python classes enqueue: 25 iterations from the same seeds at the reference's worker defaults
    (8 agents, batch_size 512: 64 worker steps every 10th iteration), B = 256"""
    def run(native):
        opt = _stack(native, num_agent=8, batch_size=512, replay_batch_size=256, replay_starts=1024, max_buffer_size=4096,
                     num_batch_reuse=reuse, num_future_data=K)
        for _ in range(25):
            opt.step()
        opt.worker.policy_with_value.check_status()
        return _state(opt), opt.learner.get_stats()
    a, sa = run(True)
    b, sb = run(False)
    _equal_states(a, b)
    assert a[1][0] == {'Q1': 25, 'Q2': 25, 'policy': 25} and a[1][4] == 2 * 64 + 3 * 64       # warm-up and three sampling calls
    both = sorted(set(sa) & set(sb))
    assert {'q_loss1', 'q_loss2', 'policy_loss', 'policy_entropy', 'mb_targets_mean', 'value_mean', 'value_var', 'q_gradient_norm1',
            'q_gradient_norm2', 'policy_gradient_norm'} <= set(both)
    for k in both:
        assert sa[k] == sb[k], (k, sa[k], sb[k])


def test_stock_methods_interleaved_with_native_steps(engine):
    """worker.sample() + rb.add_batch() between native steps, on a 700-slot ring that wraps, end in the same state as the method path
    doing the same calls"""
    def run(native):
        opt = _stack(native, interval=2, num_agent=64, batch_size=64, replay_batch_size=96, replay_starts=256, max_buffer_size=700,
                     num_batch_reuse=3)
        for it in range(12):
            opt.step()
            if it % 3 == 1:
                batch, n = opt.worker.sample_with_count()
                opt.replay_buffer.add_batch(batch)
        return _state(opt)
    _equal_states(run(True), run(False))


def test_checkpoint_resume_is_bit_identical(tmp_path, engine):
    """written by a native stack at iteration 8, loaded into a native stack built with another seed: after 12 more iterations the
    result is bit-identical to the uninterrupted run"""
    from mpg_amd.checkpoint import load_checkpoint, save_checkpoint

    def build(seed):
        return _stack(True, seed=seed, interval=3, num_agent=64, batch_size=64, replay_batch_size=128, replay_starts=256,
                      max_buffer_size=1024, num_batch_reuse=2)
    a = build(5)
    for _ in range(8):
        a.step()
    path = save_checkpoint(str(tmp_path / 'ckpt.npz'), a)
    for _ in range(12):
        a.step()
    b = build(99)                        # different seed: every stream must come from the file
    meta = load_checkpoint(path, b)
    assert meta['optimizer']['iteration'] == 8 and b.iteration == 8 and meta['learner_cls'] == 'SACLearner'
    for _ in range(12):
        b.step()
    _equal_states(_state(a), _state(b))


def test_the_default_stays_the_method_path(engine):
    opt = _stack(False, num_agent=64, batch_size=64, replay_batch_size=64, replay_starts=64, max_buffer_size=256)
    assert opt._fused is None
    opt = _stack(True, num_agent=64, batch_size=64, replay_batch_size=64, replay_starts=64, max_buffer_size=256)
    assert opt._fused is not None and opt._fused.c.learner_version == 7
    opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(opt.worker.policy_with_value.params).all()
