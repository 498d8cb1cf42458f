"""Native step driver binding (mpg_step_begin / mpg_step_end): one optimizer iteration enqueued from C++ so that the
Python interpreter is not on the launch path.  Built from - and kept in sync with - the stock worker / buffer / learner
objects, whose methods remain usable at any time: every fused step starts by reading their counters and buffers
(sync_in) and ends by writing them back (push)."""
import ctypes

import torch

from . import _lib as L
from . import dist as D
from .ops import CfgStruct

_P = ctypes.c_void_p


class GradOpts(ctypes.Structure):
    """mpg_grad_opts_t"""
    _fields_ = [('critics_ready_event', _P)]


class TrainCtx(ctypes.Structure):
    """mpg_train_ctx_t (include/mpg_hip.h)"""
    _fields_ = [
        ('cfg', CfgStruct), ('learner_version', ctypes.c_int), ('num_agent', ctypes.c_int), ('sample_iters', ctypes.c_int),
        ('sampling_interval', ctypes.c_int), ('batch', ctypes.c_int), ('n', ctypes.c_int), ('M', ctypes.c_int),
        ('n_select', ctypes.c_int), ('select', ctypes.c_int * 4), ('eta', ctypes.c_float), ('total_ite', ctypes.c_int),
        ('clip', ctypes.c_float), ('tau', ctypes.c_float), ('delay_update', ctypes.c_int), ('num_batch_reuse', ctypes.c_int),
        ('world_size', ctypes.c_int), ('grads_exchanged', ctypes.c_int), ('explore_sigma', ctypes.c_float), ('value_lr', ctypes.c_float * 3),
        ('policy_lr', ctypes.c_float * 3),
        ('worker_seed', ctypes.c_uint64), ('noise_ctr', ctypes.c_uint64), ('env_seed', ctypes.c_uint64),
        ('env_ctr', ctypes.c_uint64), ('replay_seed', ctypes.c_uint64), ('replay_times', ctypes.c_uint64),
        ('learner_seed', ctypes.c_uint64), ('learner_counter', ctypes.c_uint64),
        ('ring_capacity', ctypes.c_int), ('ring_next', ctypes.c_int), ('ring_size', ctypes.c_int),
        ('opt_steps', ctypes.c_longlong * 3),
        ('env_state', _P), ('w_obs', _P), ('w_act', _P), ('w_rew', _P), ('w_obs2', _P), ('w_done', _P), ('w_done_intended', _P),
        ('ring_obs', _P), ('ring_act', _P), ('ring_rew', _P), ('ring_obs2', _P), ('ring_done', _P),
        ('idx', _P), ('b_obs', _P), ('b_act', _P), ('b_rew', _P), ('b_obs2', _P), ('b_done', _P), ('b_targets', _P),
        ('params', _P), ('targets', _P), ('adam_m', _P), ('adam_v', _P), ('grad', _P), ('norms', _P), ('clip_scratch', _P), ('nonfinite', _P),
        ('l_env_state', _P), ('l_obs', _P), ('l_act', _P), ('l_rewards', _P), ('l_done', _P), ('l_done_intended', _P),
        ('ws0', _P), ('ws1', _P), ('ws0_bytes', ctypes.c_size_t), ('ws1_bytes', ctypes.c_size_t),
        ('smooth_sigma', ctypes.c_float), ('smooth_clip', ctypes.c_float), ('prioritized', ctypes.c_int),
        ('per_sum', _P), ('per_min', _P), ('per_stamp', _P), ('per_capacity', ctypes.c_int), ('per_max_priority', _P),
        ('per_alpha', ctypes.c_double), ('per_beta', ctypes.c_double), ('per_eps', ctypes.c_double),
        ('b_weights', _P), ('scratch', _P),
        ('critics_ready_event', _P), ('grad_opts', GradOpts), ('clip_partials_ready', ctypes.c_int)]


class LaggedSample(ctypes.Structure):
    """mpg_lagged_sample_t"""
    _fields_ = [('lag', ctypes.c_int), ('side', _P), ('forked', _P), ('done', _P), ('policy', _P),
                ('s_obs', _P), ('s_act', _P), ('s_rew', _P), ('s_obs2', _P), ('s_done', _P), ('pending', ctypes.c_int), ('due', ctypes.c_int)]


ON_REQUEST = (7, 8)      # SAC and AMPC are served, but taken only where the optimizer is asked to (native_sac / native_ampc)


def native_stack(worker, learner, rb):
    """(learner_version, n, M, n_select) of the mpg_train_ctx_t that serves this (worker, learner, replay buffer), or None where the
    driver does not serve it"""
    from .buffer import PrioritizedReplayBuffer
    from .learners import AMPCLearner, MPGLearner, NADPLearner, NDPGLearner, SACLearner, TD3Learner
    per, kind = isinstance(rb, PrioritizedReplayBuffer), type(learner)
    if getattr(getattr(worker, 'env', None), 'kind', None) == 2:
        return None                     # the model-backed env (args.env_on_model): the driver's sample steps the real envs only
    if per != (getattr(getattr(learner, 'args', None), 'buffer_type', 'normal') != 'normal'):
        return None
    if kind is TD3Learner:              # the one learner whose replay may be prioritized
        return (4, 1, 1, 1) if learner.num_batch_reuse == 1 else None
    if per:
        return None
    if kind is MPGLearner and not learner.deriv_interval_policy:
        sel = list(learner.num_rollout_list_for_policy_update)
        return (1 if learner.args.learner_version == 'MPG-v1' else 2, max(sel), learner.M, len(sel))
    if kind is NADPLearner and learner.n_q == learner.n_pi and learner.num_batch_reuse == 1:
        return (3, learner.n_pi, 1, 2)
    if kind is NDPGLearner:
        return (5, learner.sample_num_in_learner, 1, 1)
    if kind is SACLearner and worker.explore_sigma is None:
        return (7, 1, 1, 1)
    if kind is AMPCLearner:
        return (8, learner.n, learner.M, 1)
    return None


class FusedMPGStep(object):
    """step(iteration) == SingleProcessOffPolicyOptimizer.step for (OffPolicyWorker, replay buffer, learner) sharing one
    PolicyWithQs: MPGLearner + ReplayBuffer (learner_version 1 / 2), NADPLearner + ReplayBuffer (3), TD3Learner + ReplayBuffer
    or PrioritizedReplayBuffer (4; the priority update of optimizer.py:351-353 included), NDPGLearner + ReplayBuffer (5),
    SACLearner + ReplayBuffer without explore_sigma (7: mpg_sac_step_begin, which takes the learner's fixed alpha, or with
    alpha = 'auto' the pair mpg_sac_auto_step_begin / mpg_sac_auto_step_end on the policy's device-resident temperature),
    AMPCLearner + ReplayBuffer (8: the policy alone - no critic, no target, no ws0; SingleProcessOffPolicyOptimizer takes it with
    native_ampc=True).

    sample_lag = L (1 .. sampling_interval; include/mpg_hip.h, mpg_lagged_sample_t): the sample that starts at iteration k reads the
    policy as it stands then and its rows enter the ring at the start of iteration k + L; it runs on a second stream beside the steps
    between (side_stream=False: the same calls in the same order on the one stream - the reference form, bit-identical).  This object
    owns the side stream, the two events, the worker's copy and the staging rows.  From a fork to the next join the worker's observation, done mask and env state belong to
    the side stream: the worker's Python-side `obs` and counters, and the ring, are valid after drain() or at the next join."""

    def __init__(self, worker, learner, rb, sampling_interval, always_exchange=False, sample_lag=None, side_stream=True):
        stack = native_stack(worker, learner, rb)
        assert stack is not None, 'the native step driver does not serve this stack'
        assert learner.policy_with_value is worker.policy_with_value
        self.worker, self.learner, self.rb = worker, learner, rb
        pw, a, dev = worker.policy_with_value, learner.args, worker.device
        self.pw = pw
        c = self.c = TrainCtx()
        c.cfg = pw.cfg
        c.learner_version, c.n, c.M, c.n_select = stack
        if c.learner_version in (1, 2):
            for i, k in enumerate(learner.num_rollout_list_for_policy_update):
                c.select[i] = k
        if c.learner_version == 4:
            c.smooth_sigma, c.smooth_clip = float(a.policy_smoothing_sigma), float(a.policy_smoothing_clip)
        c.num_agent, c.sample_iters = worker.num_agent, max(1, worker.batch_size // worker.num_agent)
        c.sampling_interval = sampling_interval
        c.batch = learner.batch_size
        c.eta, c.total_ite = float(getattr(a, 'eta', 0.1)), int(getattr(a, 'rule_based_bias_total_ite', 9000))
        c.clip, c.tau, c.delay_update = float(a.gradient_clip_norm), pw.tau, pw.delay_update
        c.num_batch_reuse, c.world_size = learner.num_batch_reuse, D.world_size()
        # always_exchange: run the collective (and the exchanged-gradient form of the clip) even in a one-process group
        self.always_exchange = bool(always_exchange)
        c.grads_exchanged = 1 if (c.world_size > 1 or self.always_exchange) else 0
        c.explore_sigma = float(worker.explore_sigma or 0.)
        for i in range(3):
            c.policy_lr[i] = pw.schedules['policy'][i]
            if 'Q1' in pw.schedules:            # (a policy-only stack has no critic schedule: value_lr stays zero)
                c.value_lr[i] = pw.schedules['Q1'][i]
        c.worker_seed, c.env_seed, c.replay_seed, c.learner_seed = worker.seed, worker.env.seed, rb.seed, learner.seed
        n, B, od, ad = worker.num_agent, learner.batch_size, pw.obs_dim, pw.act_dim
        f = dict(dtype=torch.float32, device=dev)
        u8 = dict(dtype=torch.uint8, device=dev)
        self.t = t = dict(
            w_obs=worker.obs.clone(), w_act=torch.empty(n, ad, **f), w_rew=torch.empty(n, **f), w_obs2=torch.empty(n, od, **f),
            w_done=torch.ones(n, **u8), w_done_intended=torch.zeros(n, **u8),
            idx=torch.empty(B, dtype=torch.int32, device=dev), b_obs=torch.empty(B, od, **f), b_act=torch.empty(B, ad, **f),
            b_rew=torch.empty(B, **f), b_obs2=torch.empty(B, od, **f), b_done=torch.empty(B, **f), b_targets=torch.empty(B, **f))
        if c.learner_version == 1:
            t.update(l_obs=torch.empty(B, od, **f), l_act=torch.empty(B, ad, **f), l_rewards=torch.empty(c.n, B, **f),
                     l_done=torch.ones(B, **u8), l_done_intended=torch.zeros(B, **u8))
            if learner.env is None:         # the pendulum: one launch holds the agents in registers; the chain (sample_iters < 0,
                self.l_env_state = torch.zeros(8, B, **f)      # n > 1024) steps this block of MPG_ENV_STATE_DIM rows
                c.l_env_state = L.ptr(self.l_env_state)
            else:
                c.l_env_state = L.ptr(learner.env._state)
        elif c.learner_version == 5:        # the one-launch sampler keeps its agents in registers: rewards and last observations only
            t.update(l_obs=torch.empty(B, od, **f), l_rewards=torch.empty(c.n, B, **f))
        for k, v in t.items():
            setattr(c, k, L.ptr(v))
        c.env_state = L.ptr(worker.env._state)
        c.ring_capacity = rb._maxsize
        for k, v in (('ring_obs', rb.obs), ('ring_act', rb.act), ('ring_rew', rb.rew), ('ring_obs2', rb.obs2), ('ring_done', rb.done)):
            setattr(c, k, L.ptr(v))
        c.params, c.targets, c.adam_m, c.adam_v = L.ptr(pw.params), L.ptr(pw.targets), L.ptr(pw.m), L.ptr(pw.v)
        c.grad, c.norms, c.nonfinite = L.ptr(learner.flat), L.ptr(learner.norms), L.ptr(pw.nonfinite)
        c.clip_scratch = L.ptr(learner.clip_scratch)
        if c.learner_version == 7:          # the learner's draws (the size include/mpg_hip.h documents for this version)
            self.auto_alpha = bool(getattr(learner, 'auto_alpha', False))
            self.scratch = torch.empty(max((2 if self.auto_alpha else 1) * B * ad, n * (ad + 1)) + 64, **f)
            c.scratch = L.ptr(self.scratch)
        if c.learner_version == 4:
            self.scratch = torch.empty(max(B * (ad + 3), 2 * n) + 64, **f)
            c.scratch = L.ptr(self.scratch)
            per = a.buffer_type != 'normal'          # (native_stack: the buffer's class says the same)
            c.prioritized = 1 if per else 0
            if per:
                t['b_weights'] = torch.empty(B, **f)
                c.b_weights = L.ptr(t['b_weights'])
                c.per_sum, c.per_min, c.per_stamp = L.ptr(rb._it_sum), L.ptr(rb._it_min), L.ptr(rb._stamp)
                c.per_capacity, c.per_max_priority = rb._cap, L.ptr(rb._max_priority)
                c.per_alpha, c.per_beta, c.per_eps = rb._alpha, rb._beta, rb._eps
        # scheduling option of the MPG step (include/mpg_hip.h, mpg_grad_opts_t; leaves every number unchanged): with an exchange,
        # MPG_OVERLAP_EXCHANGE=1 (off by default): the critics' gradient is finished ahead of the reverse sweep and exchanged on a
        # second stream under it (costs ~9 us on one GPU, where there is nothing to hide)
        import os
        self.overlap = None
        if c.learner_version in (1, 2):
            if c.grads_exchanged and os.environ.get('MPG_OVERLAP_EXCHANGE') == '1':
                side = torch.cuda.Stream(device=dev)
                e1, e2 = torch.cuda.Event(), torch.cuda.Event()
                e1.record()                       # (the handle exists once the event has been recorded)
                e2.record()
                n_crit = int(sum(pw.sizes[:len(pw.names) - 1]))
                self.overlap = (side, e1, e2, n_crit)
                c.critics_ready_event = e1.cuda_event
        w0, w1 = ctypes.c_size_t(0), ctypes.c_size_t(0)
        L.call('mpg_step_workspace_bytes', ctypes.byref(c), ctypes.byref(w0), ctypes.byref(w1))
        self.ws0 = torch.empty(w0.value + 256, dtype=torch.uint8, device=dev)
        self.ws1 = torch.empty(w1.value + 256, dtype=torch.uint8, device=dev)
        c.ws0, c.ws1, c.ws0_bytes, c.ws1_bytes = L.ptr(self.ws0), L.ptr(self.ws1), self.ws0.numel(), self.ws1.numel()
        self._lib = L.lib()
        self._ref = ctypes.byref(c)
        # the entry points of this version, chosen once (the library is looked up at call time: self._lib may be wrapped)
        self._end = lambda it, s: L.check(self._lib.mpg_step_end(self._ref, ctypes.c_int(it), s), 'mpg_step_end')
        if c.learner_version == 7 and self.auto_alpha:
            # the learned temperature: read on the device, never here (its step counter lives in the policy's own struct: nothing to
            # pull or push)
            self._begin = lambda it, s: L.check(
                self._lib.mpg_sac_auto_step_begin(self._ref, ctypes.byref(pw.alpha_desc), ctypes.c_int(it), s), 'mpg_sac_auto_step_begin')
            self._end = lambda it, s: L.check(
                self._lib.mpg_sac_auto_step_end(self._ref, ctypes.byref(pw.alpha_desc), ctypes.c_int(it), s), 'mpg_sac_auto_step_end')
        elif c.learner_version == 7:        # the fixed temperature travels as an argument (mpg_train_ctx_t has no field for it)
            self._begin = lambda it, s: L.check(
                self._lib.mpg_sac_step_begin(self._ref, ctypes.c_float(learner.alpha), ctypes.c_int(it), s), 'mpg_sac_step_begin')
        else:
            self._begin = lambda it, s: L.check(self._lib.mpg_step_begin(self._ref, ctypes.c_int(it), s), 'mpg_step_begin')
        self.lagged = None
        if sample_lag is not None:
            self._bind_lagged(int(sample_lag), side_stream)
        # the python objects now look at the driver's buffers
        learner.batch_data = {'batch_obs': t['b_obs'], 'batch_actions': t['b_act'], 'batch_rewards': t['b_rew'],
                              'batch_obs_tp1': t['b_obs2'], 'batch_dones': t['b_done'], 'batch_targets': t['b_targets']}
        learner._views = None
        self.pull()

    def _bind_lagged(self, lag, side_stream):
        """the caller-owned half of mpg_lagged_sample_t and the *_lagged entry points in the place of the plain begins"""
        c, pw, dev = self.c, self.pw, self.worker.device
        if not 1 <= lag <= c.sampling_interval:
            raise ValueError('sample_lag must be within 1 .. sampling_interval = %d (got %d)' % (c.sampling_interval, lag))
        if c.world_size > 1:
            raise ValueError('sample_lag is not served with world_size > 1 (got %d)' % c.world_size)
        g = self.lagged = LaggedSample()
        g.lag = lag
        rows, od, ad = abs(c.sample_iters) * c.num_agent, pw.obs_dim, pw.act_dim
        f = dict(dtype=torch.float32, device=dev)
        self.lag_t = lt = dict(policy=torch.empty(pw.sizes[-1], **f), s_obs=torch.empty(rows, od, **f), s_act=torch.empty(rows, ad, **f),
                               s_rew=torch.empty(rows, **f), s_obs2=torch.empty(rows, od, **f),
                               s_done=torch.empty(rows, dtype=torch.uint8, device=dev))
        for k, v in lt.items():
            setattr(g, k, L.ptr(v))
        if side_stream:
            self.side = torch.cuda.Stream(device=dev)
            self.lag_events = e1, e2 = torch.cuda.Event(), torch.cuda.Event()
            e1.record()                       # (the handle exists once the event has been recorded)
            e2.record()
            g.side, g.forked, g.done = self.side.cuda_stream, e1.cuda_event, e2.cuda_event
        gref = ctypes.byref(g)
        learner, I = self.learner, ctypes.c_int
        if c.learner_version == 7 and self.auto_alpha:
            self._begin = lambda it, s: L.check(
                self._lib.mpg_sac_auto_step_begin_lagged(self._ref, ctypes.byref(pw.alpha_desc), gref, I(it), s), 'mpg_sac_auto_step_begin_lagged')
        elif c.learner_version == 7:
            self._begin = lambda it, s: L.check(
                self._lib.mpg_sac_step_begin_lagged(self._ref, ctypes.c_float(learner.alpha), gref, I(it), s), 'mpg_sac_step_begin_lagged')
        else:
            self._begin = lambda it, s: L.check(self._lib.mpg_step_begin_lagged(self._ref, gref, I(it), s), 'mpg_step_begin_lagged')

    @property
    def pending(self):
        """a lagged sample has been started and its rows are not in the ring yet"""
        return self.lagged is not None and self.lagged.pending > 0

    def drain(self):
        """mpg_lagged_sample_drain: a pending sample is joined and added now (the end of a run, ahead of a checkpoint or of any stock
        method that reads the ring or the worker)"""
        if self.lagged is None:
            return
        self.sync_in()
        L.check(self._lib.mpg_lagged_sample_drain(self._ref, ctypes.byref(self.lagged), L.stream()), 'mpg_lagged_sample_drain')
        self.push()

    def discard_pending(self):
        """ahead of a checkpoint restore: a sample of the state about to be replaced finishes, and its rows are dropped"""
        if self.pending:
            torch.cuda.synchronize()
            self.lagged.pending = 0

    def pull(self):
        """python objects -> context counters"""
        c, w, rb, ln, pw = self.c, self.worker, self.rb, self.learner, self.pw
        c.noise_ctr, c.env_ctr, c.replay_times, c.learner_counter = w._noise_ctr, w.env._ctr, rb.replay_times, ln.counter
        c.worker_seed, c.env_seed, c.replay_seed, c.learner_seed = w.seed, w.env.seed, rb.seed, ln.seed
        c.ring_next, c.ring_size = rb._next_idx, rb._size
        for i, n in enumerate(pw.names):
            c.opt_steps[i] = pw.opt_steps[n]

    def push(self):
        """context counters -> python objects (so their own methods can be mixed with fused steps)"""
        c, w, rb, ln, pw = self.c, self.worker, self.rb, self.learner, self.pw
        w._noise_ctr, w.env._ctr, rb.replay_times, ln.counter = c.noise_ctr, c.env_ctr, c.replay_times, c.learner_counter
        rb._next_idx, rb._size = c.ring_next, c.ring_size
        for i, n in enumerate(pw.names):
            pw.opt_steps[n] = c.opt_steps[i]
        w.obs = w.env.obs = self.t['w_obs']
        w.env.done = self.t['w_done']
        w.env._initialised = True

    def sync_in(self):
        """python objects -> driver (counters, and the worker's observation / done buffers if they were re-bound):
        whatever the stock methods did since the last fused step - worker.sample(), rb.add_batch(), rb.replay(),
        learner.compute_gradient(), a checkpoint restore - is what the next fused step continues from."""
        w = self.worker
        if w.obs is not self.t['w_obs']:
            self.t['w_obs'].copy_(w.obs)
        if w.env.done is not self.t['w_done']:
            self.t['w_done'].copy_(w.env.done)
        self.pull()

    def reload(self):
        """after the python objects were restored from a checkpoint: refresh the driver's own buffers and counters"""
        self.sync_in()
        self.push()

    def step(self, iteration):
        self.sync_in()           # a few host scalar copies; the tensor copies only happen after a stock-method call
        s = L.stream()
        c, flat = self.c, self.learner.flat
        c.clip_partials_ready = 0
        # without the overlap option, where the backend offers a staging slot (D.grad_slot: the one-shot backend), the step writes its
        # partial gradient STRAIGHT into it and the exchange's sum leaves the clip's partials of the reduced gradient behind
        # (mpg_sum_slots_sq) - on one GPU the exchange path is then one launch on top of the unexchanged step instead of three
        slot = D.grad_slot(flat.numel(), flat.device, force=self.always_exchange) if c.grads_exchanged and self.overlap is None else None
        try:
            if slot is not None:
                c.grad = slot.data_ptr()
            self._begin(iteration, s)
            if c.grads_exchanged:
                # the ONE exchange step, timed under the caller's kernel timer (slot 8, HIP events on the launch stream: bench.py's
                # `exchange_ms`) - a null or stopped timer makes both calls no-ops
                prof = ctypes.c_void_p(c.cfg.prof)
                self._lib.mpg_prof_region_begin(prof, ctypes.c_int(8), s)
                if self.overlap is not None:
                    # the critics' slice was complete when the library recorded e1 (ahead of the reverse sweep): its exchange runs on
                    # the side stream under the sweep, the policy's slice + statistics follow the sweep on the launch stream
                    side, e1, e2, n_crit = self.overlap
                    main = torch.cuda.current_stream()
                    side.wait_event(e1)
                    with torch.cuda.stream(side):
                        D.all_reduce_sum_(flat[:n_crit], force=self.always_exchange, tag=1)
                        e2.record(side)
                    D.all_reduce_sum_(flat[n_crit:], force=self.always_exchange)
                    main.wait_event(e2)
                elif slot is not None:
                    D.all_reduce_sum_(flat, force=self.always_exchange, in_slot=True, seg_sizes=self.pw.sizes, sq_part=self.learner.clip_scratch)
                    c.clip_partials_ready = 1
                else:
                    D.all_reduce_sum_(flat, force=self.always_exchange)
                self._lib.mpg_prof_region_end(prof, ctypes.c_int(8), s)
        finally:
            # mpg_step_end reads the reduced gradient from `flat`; a slot whose exchange did not run is handed back
            c.grad = flat.data_ptr()
            if slot is not None and not c.clip_partials_ready:
                D.release_slot(flat.numel())
        self._end(iteration, s)
        self.push()
