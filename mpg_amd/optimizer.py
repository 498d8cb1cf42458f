"""SingleProcessOffPolicyOptimizer - mirror of optimizer.py:286-397: the per-iteration order
(sample every 10th iteration -> replay -> set_weights -> compute_gradient -> (priorities) -> NaN guard ->
apply_gradients) is the contract; Ray / TensorBoard plumbing is out of scope.  One instance per GPU process."""
import gc
import logging

logger = logging.getLogger(__name__)


def quiesce_gc():
    """Collect once, then move everything alive into the permanent generation (gc.freeze).  `import torch` leaves ~10^6
    container objects behind; a generation-2 pass over them takes 40-100 ms and the step loop's own small allocations
    trigger one every few thousand iterations - 10 % of a 0.45 ms step (tools/stall_scan.py).  After the freeze the
    collector only ever walks what the loop itself allocates.  Call it once after the training stack is built."""
    gc.collect()
    gc.freeze()


class SingleProcessOffPolicyOptimizer(object):
    def __init__(self, worker, learner, replay_buffer, evaluator, args, sampling_interval=10, fused=True,
                 always_exchange=False, native_sac=False, native_ampc=False, sample_lag=None):
        """sample_lag = L (1 <= L <= sampling_interval; None: off, the serial order of the reference's single-process optimizer): the
        deterministic form of the reference's default optimizer, OffPolicyAsync, whose workers sample with weights up to
        max_weight_sync_delay iterations old.  The sample that starts at iteration k (k % sampling_interval == 0) reads the policy as it
        stands at the start of iteration k; its rows enter the replay buffer at the start of iteration k + L, before that iteration's
        draw; num_sampled_steps counts at k.  On the native driver the sample then runs on a second stream beside the steps
        (mpg_amd/fused.py); there the worker's Python-side `obs` and counters, and the buffer, are valid after drain() or at the next
        join.  drain() adds a held batch now: the end of a run, or ahead of save_checkpoint, which refuses a pending sample."""
        if sample_lag is not None:
            from . import dist as D
            if isinstance(sample_lag, bool) or int(sample_lag) != sample_lag or not 1 <= sample_lag <= sampling_interval:
                raise ValueError('sample_lag must be an integer within 1 .. sampling_interval = %d (got %r)' % (sampling_interval, sample_lag))
            if D.world_size() > 1:
                raise ValueError('sample_lag is not served with world_size > 1 (got %d): every rank would hold a pending sample of its own'
                                 % D.world_size())
        self.sample_lag = None if sample_lag is None else int(sample_lag)
        self._held = None                  # the method path's pending sample: (batch, the iteration it is due at)
        if native_sac or native_ampc:
            # SAC's native step (mpg_sac_step_begin, or the mpg_sac_auto_step_* pair with alpha = 'auto') and AMPC's (learner_version 8 of
            # mpg_step_begin / mpg_step_end) are taken on request only; a request the driver cannot serve is an error - raised before
            # anything is sampled - never a silent fall-back to the method path
            keyword = 'native_ampc' if native_ampc else 'native_sac'
            reason = self._native_refusal(keyword, worker, learner, replay_buffer, args, both=bool(native_sac and native_ampc))
            if reason:
                raise ValueError('%s=True: %s' % (keyword, reason))
        self.args = args
        self.worker, self.learner, self.replay_buffer, self.evaluator = worker, learner, replay_buffer, evaluator
        self.num_sampled_steps = 0
        self.iteration = 0
        self.sampling_interval = sampling_interval
        self.stats = {}
        # single process: share one PolicyWithQs between worker and learner (no 1.6 MB weight copy per iteration)
        self.learner.share_policy(self.worker.policy_with_value)
        while not len(self.replay_buffer) >= self.args.replay_starts:      # optimizer.py:310-313
            sample_batch, count = self.worker.sample_with_count()
            self.num_sampled_steps += count
            self.replay_buffer.add_batch(sample_batch)
        # native step driver (mpg_step_begin/_end) when the stock MPG components are plugged in; otherwise the
        # method-by-method path below, which computes the same thing
        self._fused = None
        if native_sac or native_ampc or fused:
            from .fused import ON_REQUEST, FusedMPGStep, native_stack
            stack = native_stack(worker, learner, replay_buffer)
            if native_sac or native_ampc or (stack is not None and stack[0] not in ON_REQUEST):
                self._fused = FusedMPGStep(worker, learner, replay_buffer, sampling_interval, always_exchange=always_exchange,
                                           sample_lag=self.sample_lag)

    @staticmethod
    def _native_refusal(keyword, worker, learner, replay_buffer, args, both=False):
        """why the native step asked for by `keyword` ('native_sac': mpg_sac_step_begin; 'native_ampc': learner_version 8 of
        mpg_step_begin) does not serve this stack, or None"""
        from .buffer import PrioritizedReplayBuffer
        from .learners import AMPCLearner, SACLearner
        if both:
            return 'native_sac and native_ampc are both set: a stack has one learner, ask for its keyword alone'
        cls, what = {'native_sac': (SACLearner, 'SAC'), 'native_ampc': (AMPCLearner, 'AMPC')}[keyword]
        if type(learner) is not cls:
            return 'the learner is %s, not %s (every learner but SACLearner and AMPCLearner takes the native step by default)' \
                % (type(learner).__name__, cls.__name__)
        if isinstance(replay_buffer, PrioritizedReplayBuffer) or getattr(args, 'buffer_type', 'normal') != 'normal':
            return 'a prioritized replay buffer is not served by the native %s step (uniform ReplayBuffer only)' % what
        if getattr(getattr(worker, 'env', None), 'kind', None) == 2:
            return 'the worker samples the model-backed env (env_on_model), which the native step driver does not step'
        if keyword == 'native_ampc':
            # what mpg_step_begin refuses of a learner_version 8 context (include/mpg_hip.h), said where the stack is built
            if not 1 <= learner.n <= 31:
                return 'the rollout horizon n = %d is outside 1 .. 31 (mpg_ampc_pg: 0 < n < 32)' % learner.n
            if (learner.batch_size * learner.M) % 16 != 0:
                return 'replay_batch_size * M = %d is not a multiple of 16 (mpg_ampc_pg differentiates every step through the policy ' \
                       'in 16-row groups)' % (learner.batch_size * learner.M)
            return None
        if getattr(learner, 'squashed', False) or getattr(getattr(worker, 'policy_with_value', None), 'squashed_head', False):
            return 'the tanh-squashed head (squashed_head=True) is not served by the native SAC step: build the optimizer without native_sac'
        if worker.explore_sigma is not None:
            return 'explore_sigma (%r) on top of the stochastic policy is not served by the native SAC step' % (worker.explore_sigma,)
        return None

    def set_profiler(self, prof):
        """attach an ops.Profiler (or None) to every cfg this optimizer launches with"""
        cfgs = [self.worker.policy_with_value.cfg, self.learner.policy_with_value.cfg]
        if self._fused is not None:
            cfgs.append(self._fused.c.cfg)
        old = getattr(self, '_prof', None)
        if old is not None:
            old.detach(*cfgs)
        for c in cfgs:
            c.prof = None
        self._prof = prof            # the optimizer keeps the timer alive for as long as its cfgs point at it
        if prof is not None:
            prof.attach(*cfgs)

    def get_stats(self):
        self.stats.update(dict(num_sampled_steps=self.num_sampled_steps, iteration=self.iteration))
        return self.stats

    def step(self):
        if self._fused is not None:
            self._fused.step(self.iteration)                   # (a refused step raises here: nothing below has been counted)
            if self.iteration % self.sampling_interval == 0:
                self.num_sampled_steps += self.worker.num_agent * abs(self._fused.c.sample_iters)      # (< 0: the chain kept, include/mpg_hip.h)
            self.learner._lazy_stats = self.learner._native_lazy_stats(self.iteration)
            self.iteration += 1
            self._check_status()
            return
        if self._held is not None and self.iteration >= self._held[1]:     # sample_lag: the rows of iteration k enter at k + L
            self.drain()
        if self.iteration % self.sampling_interval == 0:                   # optimizer.py:332-337
            sample_batch, count = self.worker.sample_with_count()
            self.num_sampled_steps += count
            if self.sample_lag is None:
                self.replay_buffer.add_batch(sample_batch)
            else:
                self._held = (sample_batch, self.iteration + self.sample_lag)
        samples = self.replay_buffer.replay()                              # :340-341
        self.learner.set_weights(self.worker.policy_with_value)            # :345 (shared object: no copy)
        grads = self.learner.compute_gradient(samples[:5], self.replay_buffer, samples[-1], self.iteration)   # :349
        if getattr(self.args, 'buffer_type', 'normal') == 'priority':     # :351-353
            info = self.learner.get_info_for_buffer()
            info['rb'].update_priorities(info['indexes'], info['td_error'])
        # NaN guard (:357-361) lives on the device: the clip kernel raises a flag that makes Adam see zero gradients
        self.worker.apply_gradients(self.iteration, self.learner.flat_grad)   # :362
        self.get_stats()
        self.iteration += 1
        self._check_status()

    @property
    def sample_pending(self):
        """sample_lag: a sample has been taken whose rows are not in the replay buffer yet"""
        return self._held is not None or (self._fused is not None and self._fused.pending)

    def drain(self):
        """sample_lag: add a held batch now, whatever its due iteration (the native driver: mpg_lagged_sample_drain, which joins the
        side stream first).  For the end of a run and ahead of save_checkpoint; without a pending sample it does nothing."""
        if self._fused is not None:
            self._fused.drain()
        if self._held is not None:
            self.replay_buffer.add_batch(self._held[0])
            self._held = None

    def discard_pending(self):
        """sample_lag, ahead of load_checkpoint: a pending sample belongs to the state about to be replaced - it is dropped, not added"""
        self._held = None
        if self._fused is not None:
            self._fused.discard_pending()

    def _check_status(self):
        """judge_is_nan / the engine's numerical envelope (include/mpg_hip.h): every kernel of the step ORs its findings into the
        shared policy's sticky status word; it is read (one host synchronisation) every `nan_check_interval` iterations, in BOTH
        branches of step() - the native driver never goes through worker.sample(), which is where the method path reads it
        (worker.py:95-107, optimizer.py:357-361 of the reference stop the run on the same conditions)."""
        k = getattr(self.worker, 'nan_check_interval', 100)
        if k > 0 and self.iteration % k == 0:
            self.worker.policy_with_value.check_status()

    def stop(self):
        pass
