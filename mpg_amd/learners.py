"""Learners - device mirrors of learners/mpg_learner.py (MPGLearner), learners/nadp.py (NADPLearner),
learners/td3.py (TD3Learner), learners/ndpg.py (NDPGLearner), learners/sac.py (SACLearner, fixed or learned temperature) and learners/ampc.py
(AMPCLearner, the policy alone): same constructor signature `(policy_cls, args)`, same methods the optimizer calls
(`set_weights`, `compute_gradient(batch5, rb, indexes, iteration)`, `get_stats`, `get_info_for_buffer`), same
output order `q1 (+q2) + policy`.

Data-parallel form: each process computes sum-reduced, UN-clipped gradient partials already scaled
by 1/B_global into one flat buffer [grads | stats]; ONE all-reduce; then per-network tf.clip_by_global_norm
(non-linear, must follow the reduce).  On one process this is exactly the reference computation."""
import numpy as np
import torch

from . import dist as D
from . import ops
from .envs import InvertedPendulumContiEnv, PathTrackingEnv

PENDULUM = 'InvertedPendulumConti-v0'


def rule_based_weights(ite, total_ite, eta, select):
    """MPGLearner.rule_based_weights, mpg_learner.py:384-399 (float32 like the TF graph)."""
    f = np.float32
    lam = f(1. - eta) + f(2. * eta / total_ite) * f(ite)
    lam = f(min(max(lam, f(0.)), f(1.5)))
    if lam < 1.:
        biases = np.array([np.power(lam, f(i)) for i in select], dtype=f)
    else:
        mx = max(select)
        biases = np.array([np.power(f(2.) - lam, f(mx - i)) for i in select], dtype=f)
    inv = (f(1.) / (biases + f(1e-8))).astype(f)
    e = np.exp(inv - inv.max()).astype(f)
    return (e / e.sum()).astype(f)


N_STATS = 16     # floats appended to the gradient buffer and summed by the same all-reduce


class _LearnerBase(object):
    def __init__(self, policy_cls, args, device='cuda'):
        self.args = args
        self.device = torch.device(device)
        self.batch_size = args.replay_batch_size
        self.policy_with_value = policy_cls(**vars(args), device=device)
        self.cfg = self.policy_with_value.cfg
        self.batch_data = {}
        self.counter = 0
        self.num_batch_reuse = getattr(args, 'num_batch_reuse', 1)
        self.stats = {}
        self.info_for_buffer = {}
        pw = self.policy_with_value
        self.n_grad = int(pw.offsets[-1])
        self.flat = torch.zeros(self.n_grad + N_STATS, dtype=torch.float32, device=self.device)
        self.norms = torch.zeros(len(pw.names), dtype=torch.float32, device=self.device)
        self.clip_scratch = torch.zeros(len(pw.names) * ops.CLIP_PARTS, dtype=torch.float32, device=self.device)
        self.seed = int(getattr(args, 'seed', 0)) + 12345
        self._noise_gen = torch.Generator(device=self.device)
        self._noise_gen.manual_seed(self.seed)
        self._views = None
        self._lazy_stats = None

    # ---- optimizer-facing API ----
    def get_stats(self):
        """Host copy of the stats of the last compute_gradient (device scalars are only read here, so the training
        loop itself never synchronises)."""
        if self._lazy_stats is not None:
            self.stats.update(self._lazy_stats())
        return {k: (v.item() if isinstance(v, torch.Tensor) and v.numel() == 1 else
                    (v.tolist() if isinstance(v, torch.Tensor) else v)) for k, v in self.stats.items()}

    def get_info_for_buffer(self):
        return self.info_for_buffer

    def get_weights(self):
        return self.policy_with_value.get_weights()

    def set_weights(self, weights):
        if weights is self.policy_with_value or weights is None:
            return
        return self.policy_with_value.set_weights(weights)

    def share_policy(self, policy):
        """Single-process mode: learner and worker use ONE PolicyWithQs instead of copying 1.6 MB of weights every
        iteration (optimizer.py:345 `learner.set_weights(worker.get_weights())` becomes a no-op)."""
        self.policy_with_value = policy
        self.cfg = policy.cfg
        self._views = None

    def set_ppc_params(self, params):
        pass

    def grad(self, name):
        pw = self.policy_with_value
        i = pw.names.index(name)
        return self.flat[pw.offsets[i]:pw.offsets[i + 1]]

    def _get_batch(self, batch_data):
        def f32(t):
            if t.dtype == torch.float32 and t.device == self.device and t.is_contiguous():
                return t
            return t.to(self.device, torch.float32).contiguous()
        self.batch_data = {k: f32(batch_data[i])
                           for i, k in enumerate(('batch_obs', 'batch_actions', 'batch_rewards', 'batch_obs_tp1', 'batch_dones'))}

    def compute_td_error(self):
        """mpg_learner.py:136-144, td3.py:83-92, ndpg.py:116-125 (signed): the plain Q1 target - Q1(s, a)."""
        pw, b = self.policy_with_value, self.batch_data
        y1 = ops.q_targets(self.cfg, pw.net('policy', True), pw.net('Q1', True), None, b['batch_rewards'], b['batch_obs_tp1'])
        return y1 - pw.compute_Q1(b['batch_obs'], b['batch_actions'])

    def _begin(self, batch_data, rb, indexes, *noise):
        """the opening of every compute_gradient: a new batch (get_batch_data, with the caller's draws) unless the last one is reused;
        the call is counted.  Returns (networks, batch, rows, 1 / B_global, the statistics slots behind the gradients)."""
        if self.counter % self.num_batch_reuse == 0:
            self.get_batch_data(batch_data, rb, indexes, *noise)
        self.counter += 1
        rows = self.batch_data['batch_obs'].shape[0]
        return self.policy_with_value, self.batch_data, rows, 1.0 / (rows * D.world_size()), self.flat[self.n_grad:]

    def _finish(self, iteration, lazy_stats=None):
        """the close of every compute_gradient: all-reduce, clip per network, expose the reference's list view; the statistics
        (lazy_stats, default _native_lazy_stats) are evaluated when get_stats() asks."""
        pw, clip = self.policy_with_value, float(self.args.gradient_clip_norm)
        D.all_reduce_sum_(self.flat)
        if self._views is None:
            self.flat_grad = self.flat[:self.n_grad]
            self._views = []
            for i, n in enumerate(pw.names):
                self._views += pw._as_list(self.flat[pw.offsets[i]:pw.offsets[i + 1]], n)
        ops.clip_by_global_norm(self.flat_grad, pw.sizes, clip, norms_out=self.norms, nonfinite=pw.nonfinite,
                                scratch=self.clip_scratch)
        self.stats['iteration'] = iteration
        self._lazy_stats = (lazy_stats or self._native_lazy_stats)(iteration)
        return self._views


class MPGLearner(_LearnerBase):
    def __init__(self, policy_cls, args, device='cuda'):
        super().__init__(policy_cls, args, device)
        self.sample_num_in_learner = args.sample_num_in_learner
        self.M = args.M
        self.num_rollout_list_for_policy_update = list(args.num_rollout_list_for_policy_update)
        self.deriv_interval_policy = bool(getattr(args, 'deriv_interval_policy', False))   # mpg_learner.py:247-248
        # value_mean is the mean return of slice 0 whether or not 0 is in the list (mpg_learner.py:285).  Where it is not, the launches
        # carry it as one more slice with weight exactly 0.0 (its dL/dQ coefficient is then an exact zero: no bit of the gradient moves)
        # - if the statistics block has room for it (n_q losses + 2 sums per slice in 8 jobs, at most 4 slices); else value_mean is None
        select, n_q = self.num_rollout_list_for_policy_update, len(self.policy_with_value.names) - 1
        self._value_slice = 0 not in select and len(select) < 4 and n_q + 2 * (len(select) + 1) <= 8
        if not self.deriv_interval_policy and not ops.mpg_gradients_supported(self.cfg, self.batch_size, self.M, max(select), len(select), n_q):
            # the library's own answer at the first gradient (mpg_mpg_gradients), raised where the learner is built
            raise ops.L.MpgError('MPG_EINVAL: mpg_mpg_gradients: too many statistics (n_select <= 3 with two critics) or an unsupported '
                                 'horizon / slice count: num_rollout_list_for_policy_update %s with %d critic(s)' % (select, n_q))
        self.env = None
        # MPG-v1 on the pendulum (train_script4mujoco.py:169-293): the n real-env steps are one launch on the cart-pole kernel and the
        # bootstrap value is clipped (mpg_learner.py:163-164)
        self.pendulum = getattr(args, 'env_id', None) == PENDULUM
        if args.learner_version == 'MPG-v1':
            # (the pendulum's env is stepped only by the chain, for horizons beyond the one launch's: sample() builds it then)
            if not self.pendulum:
                self.env = PathTrackingEnv(num_agent=self.batch_size, num_future_data=args.num_future_data, device=device)

    # ---- heuristic-bias rollout (defined but never called by the reference's compute_gradient either) ----
    def model_rollout_for_q_estimation(self, start_obses, start_actions, eps=None):
        """mpg_learner.py:180-224: from (s, a_replay) roll the model, later actions from pi_theta, bootstrap every selected
        slice of args.num_rollout_list_for_q_estimation with Q1_target, mean over the M copies; returns the selected
        slices concatenated ([len(list) * B], no gradient).  eps: optional [max(list)][M*B] standard-normal model noise
        (default: Philox draws keyed by the learner's seed and call counter)."""
        sel = list(getattr(self.args, 'num_rollout_list_for_q_estimation', []) or [])
        assert sel, 'args.num_rollout_list_for_q_estimation is empty'
        pw = self.policy_with_value
        self._qest_calls = getattr(self, '_qest_calls', 0) + 1
        return ops.rollout_q_estimation(self.cfg, pw.net('policy'), pw.net('Q1', True), start_obses, start_actions, eps, sel,
                                        M=self.M, noise_seed=self.seed + 7, noise_ctr=self._qest_calls)

    # ---- targets ----
    def compute_clipped_double_q_target(self):
        """mpg_learner.py:126-134"""
        pw, b = self.policy_with_value, self.batch_data
        return ops.q_targets(self.cfg, pw.net('policy', True), pw.net('Q1', True), pw.net('Q2', True),
                             b['batch_rewards'], b['batch_obs_tp1'])

    def sample(self, start_obs, start_action):
        """mpg_learner.py:109-124: n real-env steps; first action from replay, then the ONLINE policy, no noise.  One launch
        (mpg_env_rollout, bit-identical to the chain below) for the horizons it serves (n < 32); the learner's env is not stepped then.
        On the pendulum: mpg_env_rollout_pendulum, n <= 1024."""
        pw = self.policy_with_value
        if self.sample_num_in_learner <= 1024 if self.pendulum else self.sample_num_in_learner < 32:
            rewards, last_obs = ops.env_rollout(self.cfg, pw.net('policy'), start_obs, start_action, self.sample_num_in_learner)
            return {'all_rewards': rewards, 'last_obs': last_obs}
        if self.pendulum and self.env is None:
            self.env = InvertedPendulumContiEnv(num_agent=self.batch_size, device=self.device)
        obs = start_obs
        self.env.reset(init_obs=obs)
        rewards = []
        for t in range(self.sample_num_in_learner):
            action = start_action if t == 0 else ops.policy_action(self.cfg, pw.net('policy'), obs)
            obs, r, _, _ = self.env.step(action)
            rewards.append(r)
        return {'all_rewards': torch.stack(rewards).contiguous(), 'last_obs': obs}

    def compute_n_step_target(self):
        """mpg_learner.py:146-169"""
        pw, b = self.policy_with_value, self.batch_data
        ro = self.sample(b['batch_obs'], b['batch_actions'])
        return ops.nstep_targets(self.cfg, pw.net('policy', True), pw.net('Q1', True), ro['all_rewards'], ro['last_obs'],
                                 clip=ops.PENDULUM_NSTEP_Q_CLIP if self.pendulum else None)

    def get_batch_data(self, batch_data, rb, indexes):
        self._get_batch(batch_data)
        if self.args.learner_version == 'MPG-v1':
            target = self.compute_n_step_target()
        elif self.args.learner_version == 'MPG-v2':
            target = self.compute_clipped_double_q_target()
        else:
            raise ValueError(self.args.learner_version)
        self.batch_data['batch_targets'] = target
        if self.args.buffer_type != 'normal':
            self.info_for_buffer.update(dict(td_error=self.compute_td_error(), rb=rb, indexes=indexes))

    def draw_model_noise(self, n, cols):
        return torch.randn(n, cols, generator=self._noise_gen, device=self.device, dtype=torch.float32)

    def compute_gradient(self, batch_data, rb, indexes, iteration, eps=None):
        """mpg_learner.py:401-455.  Returns the list [q1 (6 arrays) (+ q2) + policy (6 arrays)] of device tensors
        (views of one flat buffer, also available as `self.flat_grad`).  eps: optional [n, M*B] standard-normal model
        noise (parity tests); by default it is drawn inside the rollout kernel."""
        pw, b, rows, inv_b, stats = self._begin(batch_data, rb, indexes)
        select = self.num_rollout_list_for_policy_update
        ws = rule_based_weights(iteration, self.args.rule_based_bias_total_ite, self.args.eta, select)
        n = max(select)
        if self._value_slice:
            select, ws = select + [0], np.append(ws, np.float32(0.0))
        if self.deriv_interval_policy:
            # every rollout step goes through pi_theta (full BPTT, mpg_learner.py:247-248): the fine-grained entry points
            for i, nm in enumerate(n for n in pw.names if n != 'policy'):
                ops.q_loss_grad(self.cfg, pw.net(nm), b['batch_obs'], b['batch_actions'], b['batch_targets'],
                                inv_b_global=inv_b, grad_out=self.grad(nm), loss_out=stats[i:i + 1])
            ops.rollout_pg(self.cfg, pw.net('policy'), pw.net('Q1'), b['batch_obs'], eps, select, ws, M=self.M,
                           inv_b_global=inv_b, all_steps_param_grad=True, grad_out=self.grad('policy'),
                           stats_out=stats[2:2 + 2 * len(select)], n=n, noise_seed=self.seed, noise_ctr=self.counter)
            return self._finish(iteration, self._mpg_lazy_stats)
        # one native call: critic losses/gradients + model rollout + mixed policy gradient (5 launches); the targets
        # were computed by get_batch_data (the reference caches them per batch, mpg_learner.py:402-403)
        ops.mpg_gradients(self.cfg, len(pw.names) - 1, pw.params, pw.targets, b['batch_obs'], b['batch_actions'],
                          b['batch_rewards'], b['batch_obs_tp1'], b['batch_targets'], select, ws, self.flat[:self.n_grad],
                          stats, b['batch_targets'], M=self.M, n=n, eps=eps, noise_seed=self.seed,
                          noise_ctr=self.counter, inv_b_global=inv_b)
        return self._finish(iteration, self._mpg_lazy_stats)

    def _native_lazy_stats(self, iteration):
        """what the native step driver leaves in the statistics slots, as get_stats() reports it"""
        # (the driver forms the slice weights itself from the list as given: no weight-0 slice, value_mean None where 0 is not selected)
        return self._mpg_lazy_stats(iteration, value_slice=False)

    def _mpg_lazy_stats(self, iteration, value_slice=None):
        """stats of mpg_learner.py:433-452, evaluated only when get_stats() is called"""
        pw = self.policy_with_value
        select = self.num_rollout_list_for_policy_update
        ns, nq = len(select), len(pw.names) - 1
        stats = self.flat[self.n_grad:]
        B = self.batch_size * D.world_size()
        value_slice = self._value_slice if value_slice is None else value_slice

        def lazy():
            ws = rule_based_weights(iteration, self.args.rule_based_bias_total_ite, self.args.eta, select)
            mean_ret = stats[2:2 + ns] / B
            # (the weight-0 slice 0 of _value_slice sits behind the list's own slices: reported as value_mean only)
            value_mean = stats[2 + ns] / B if value_slice else (mean_ret[select.index(0)] if 0 in select else None)
            d = dict(iteration=iteration, value_mean=value_mean,
                     policy_total_loss=-(torch.as_tensor(ws, device=self.device) * mean_ret).sum(),
                     policy_gradient_norm=self.norms[nq], q_loss1=stats[0], q_gradient_norm1=self.norms[0],
                     num_rollout_list=select, w_list=list(map(float, ws)), all_losses=-mean_ret)
            if nq == 2:
                d.update(q_loss2=stats[1], q_gradient_norm2=self.norms[1])
            return d
        return lazy


class NADPLearner(_LearnerBase):
    """n-step ADP (learners/nadp.py:23-241), config 3: the Q target AND the policy loss come from 25-step MODEL rollouts;
    every rollout step goes through pi_theta, so parameter gradients accumulate at all 26 policy evaluations."""

    def __init__(self, policy_cls, args, device='cuda'):
        super().__init__(policy_cls, args, device)
        self.M = args.M
        assert self.M == 1
        self.n_q = max(args.num_rollout_list_for_q_estimation)
        self.n_pi = args.num_rollout_list_for_policy_update[0]

    def get_batch_data(self, batch_data, rb, indexes):
        self._get_batch(batch_data)

    def compute_gradient(self, batch_data, rb, indexes, iteration, eps_q=None, eps_pi=None):
        """nadp.py:209-241"""
        pw, b, rows, inv_b, stats = self._begin(batch_data, rb, indexes)
        targets = ops.rollout_q_target(self.cfg, pw.net('policy'), pw.net('Q1', True), b['batch_obs'], b['batch_actions'],
                                       eps_q, n=self.n_q, noise_seed=self.seed, noise_ctr=2 * self.counter)   # nadp.py:87-126
        self.batch_data['batch_targets'] = targets
        ops.q_loss_grad(self.cfg, pw.net('Q1'), b['batch_obs'], b['batch_actions'], targets, inv_b_global=inv_b,
                        grad_out=self.grad('Q1'), loss_out=stats[0:1])                               # :173-184
        # slice 0 only feeds value_mean (weight 0); the loss is -R_n (nadp.py:168-171)
        ops.rollout_pg(self.cfg, pw.net('policy'), pw.net('Q1'), b['batch_obs'], eps_pi, [0, self.n_pi], [0.0, 1.0], M=1,
                       inv_b_global=inv_b, all_steps_param_grad=True, grad_out=self.grad('policy'), stats_out=stats[2:6],
                       n=self.n_pi, noise_seed=self.seed, noise_ctr=2 * self.counter + 1)
        return self._finish(iteration)

    def _native_lazy_stats(self, iteration):
        """evaluated only when get_stats() is called: no elementwise launches in the training loop"""
        stats, B = self.flat[self.n_grad:], self.batch_size * D.world_size()
        return lambda: dict(q_loss=stats[0], policy_loss=-stats[3] / B, value_mean=stats[2] / B,
                            q_gradient_norm=self.norms[0], policy_gradient_norm=self.norms[1])


class AMPCLearner(_LearnerBase):
    """Approximate MPC (learners/ampc.py:22-122): the policy alone.  The loss is minus the mean UNDISCOUNTED reward sum of an
    n-step model rollout from the batch's observations, M copies each, every step through pi_theta (:73-87); no critic, no target,
    a fresh batch on every call (:105-107).  Networks [policy] (policy_only=True)."""

    def __init__(self, policy_cls, args, device='cuda'):
        if not getattr(args, 'policy_only', False):
            raise ValueError('AMPCLearner needs policy_only=True (built_AMPC_parser, train_script.py:57-175): it trains the policy alone '
                             'and its gradient list has no critic entries')
        super().__init__(policy_cls, args, device)
        assert self.policy_with_value.names == ['policy'], 'AMPC trains [policy]'
        self.M = int(args.M)
        self.n = int(args.num_rollout_list_for_policy_update[0])
        self.num_batch_reuse = 1                                # :105-107: get_batch_data on every call

    def get_batch_data(self, batch_data, rb, indexes):
        self._get_batch(batch_data)

    def compute_gradient(self, batch_data, rb, indexes, iteration, eps=None):
        """ampc.py:105-122.  eps: optional [n, M*B] standard-normal model noise (parity tests); by default it is drawn inside the
        rollout kernel, keyed by (learner seed, call counter)."""
        pw, b, rows, inv_b, stats = self._begin(batch_data, rb, indexes)
        ops.ampc_pg(self.cfg, pw.net('policy'), b['batch_obs'], eps, M=self.M, inv_b_global=inv_b, grad_out=self.grad('policy'),
                    stats_out=stats[0:2], n=self.n, noise_seed=self.seed, noise_ctr=2 * self.counter + 1)
        return self._finish(iteration)

    def _native_lazy_stats(self, iteration):
        """evaluated only when get_stats() is called (pg_time: the reference's wall-clock timer; nothing here synchronises to take one)"""
        stats, B = self.flat[self.n_grad:], self.batch_size * D.world_size()
        return lambda: dict(pg_time=None, policy_loss=-stats[0] / B, policy_gradient_norm=self.norms[0])


class TD3Learner(_LearnerBase):
    """learners/td3.py:22-188, config 4."""

    def compute_clipped_double_q_target(self, smooth_eps=None):
        """td3.py:69-81"""
        pw, b = self.policy_with_value, self.batch_data
        rows = b['batch_obs'].shape[0]
        if smooth_eps is None:
            smooth_eps = self._smoothing_noise(rows)
        return ops.q_targets(self.cfg, pw.net('policy', True), pw.net('Q1', True), pw.net('Q2', True), b['batch_rewards'],
                             b['batch_obs_tp1'], smooth_eps=smooth_eps, smooth_sigma=self.args.policy_smoothing_sigma,
                             smooth_clip=self.args.policy_smoothing_clip)

    def _smoothing_noise(self, rows):
        """target-policy smoothing noise (td3.py:74, tf.random.normal in the reference): the library's Philox stream keyed by
        (learner seed, the gradient step this batch is fetched for) - the numbers the native step driver draws"""
        return ops.normal_fill(rows * self.cfg.act_dim, self.seed, self.counter + 1, self.device).view(rows, self.cfg.act_dim)

    def get_batch_data(self, batch_data, rb, indexes, smooth_eps=None):
        self._get_batch(batch_data)
        self._y1 = None
        if self.args.buffer_type != 'normal' and self.num_batch_reuse == 1:
            # the priorities' td error y1 - Q1(s, a) (td3.py:83-92): y1 shares the target policy's pass with the clipped double-Q
            # target (mpg_td3_targets: pi_t(s') once, not twice), and Q1 on the batch is what the critic-loss pass of
            # compute_gradient evaluates anyway, on the same weights: keep y1 and finish there (two network passes less)
            pw, b = self.policy_with_value, self.batch_data
            rows = b['batch_obs'].shape[0]
            if smooth_eps is None:
                smooth_eps = self._smoothing_noise(rows)
            self.batch_data['batch_targets'], self._y1 = ops.td3_targets(
                self.cfg, pw.net('policy', True), pw.net('Q1', True), pw.net('Q2', True), b['batch_rewards'], b['batch_obs_tp1'],
                smooth_eps, smooth_sigma=self.args.policy_smoothing_sigma, smooth_clip=self.args.policy_smoothing_clip)
            self.info_for_buffer.update(dict(td_error=None, rb=rb, indexes=indexes))
            return
        self.batch_data['batch_targets'] = self.compute_clipped_double_q_target(smooth_eps)
        if self.args.buffer_type != 'normal':
            self.info_for_buffer.update(dict(td_error=self.compute_td_error(), rb=rb, indexes=indexes))

    def compute_gradient(self, batch_data, rb, indexes, iteration, smooth_eps=None):
        """td3.py:150-188"""
        pw, b, rows, inv_b, stats = self._begin(batch_data, rb, indexes, smooth_eps)
        for i, nm in enumerate(('Q1', 'Q2')):
            pending = nm == 'Q1' and getattr(self, '_y1', None) is not None
            td = ops.q_loss_grad(self.cfg, pw.net(nm), b['batch_obs'], b['batch_actions'], b['batch_targets'], inv_b_global=inv_b,
                                 grad_out=self.grad(nm), loss_out=stats[i:i + 1], want_td=pending)[2]
            if pending:        # td = Q1(s, a) - y  =>  y1 - Q1(s, a) = (y1 - y) - td  (one launch, like the native step driver)
                self.info_for_buffer['td_error'] = ops.td3_priority_errors(self._y1, b['batch_targets'], td)
                self._y1 = None
        ops.td3_policy_grad(self.cfg, pw.net('policy'), pw.net('Q1'), pw.net('Q2'), b['batch_obs'], inv_b_global=inv_b,
                            grad_out=self.grad('policy'), stats_out=stats[2:4])
        return self._finish(iteration)

    def _native_lazy_stats(self, iteration):
        stats, B = self.flat[self.n_grad:], self.batch_size * D.world_size()

        def lazy():        # evaluated only when get_stats() is called: no elementwise launches in the training loop
            mean = stats[2] / B
            return dict(q_loss1=stats[0], q_loss2=stats[1], policy_loss=-mean, value_mean=mean,
                        value_var=stats[3] / B - mean * mean, q_gradient_norm1=self.norms[0],
                        q_gradient_norm2=self.norms[1], policy_gradient_norm=self.norms[2])
        return lazy


class NDPGLearner(_LearnerBase):
    """n-step DPG (learners/ndpg.py:23-237): the critic's target is MPG-v1's n-step REAL-env return (:127-151), the policy gradient
    is one-step DPG through the single critic (:174-186).  Networks [Q1 | policy] (double_Q=False, target=True).
    PathTracking-v0 with num_future_data 0 .. 10 only: the reference's other branch is a per-row loop over a one-agent gym env
    (:78-98) for which it ships no parser, and the analytic cart-pole here is not pinned to MuJoCo."""

    def __init__(self, policy_cls, args, device='cuda'):
        if args.env_id != 'PathTracking-v0':
            raise ValueError('NDPGLearner serves PathTracking-v0 only (got env_id %r): the reference samples every other env row by '
                             'row from a one-agent gym env (ndpg.py:78-98) and ships no parser for it' % (args.env_id,))
        if not 0 <= int(args.num_future_data) <= PathTrackingEnv.MAX_FUTURE:
            raise ValueError('NDPGLearner: num_future_data in [0, %d] (got %r)' % (PathTrackingEnv.MAX_FUTURE, args.num_future_data))
        super().__init__(policy_cls, args, device)
        assert self.policy_with_value.names == ['Q1', 'policy'], 'NDPG trains [Q1 | policy]: double_Q=False, target=True'
        self.sample_num_in_learner = args.sample_num_in_learner

    def sample(self, start_obs, start_action):
        """ndpg.py:99-114: n real-env steps, the first with the replay action, then the ONLINE policy without noise - one launch"""
        pw = self.policy_with_value
        rewards, last_obs = ops.env_rollout(self.cfg, pw.net('policy'), start_obs, start_action, self.sample_num_in_learner)
        return {'all_rewards': rewards, 'last_obs': last_obs}

    def compute_n_step_target(self):
        """ndpg.py:127-151: target policy and Q1_target at the LAST observation only"""
        pw, b = self.policy_with_value, self.batch_data
        ro = self.sample(b['batch_obs'], b['batch_actions'])
        return ops.nstep_targets(self.cfg, pw.net('policy', True), pw.net('Q1', True), ro['all_rewards'], ro['last_obs'])

    def get_batch_data(self, batch_data, rb, indexes):
        self._get_batch(batch_data)
        self.batch_data['batch_targets'] = self.compute_n_step_target()
        if self.args.buffer_type != 'normal':
            self.info_for_buffer.update(dict(td_error=self.compute_td_error(), rb=rb, indexes=indexes))

    def compute_gradient(self, batch_data, rb, indexes, iteration):
        """ndpg.py:202-237"""
        pw, b, rows, inv_b, stats = self._begin(batch_data, rb, indexes)
        if self.args.buffer_type != 'normal':                  # :206-207: the priorities follow the critic within a reused batch
            self.info_for_buffer.update(dict(td_error=self.compute_td_error()))
        ops.q_loss_grad(self.cfg, pw.net('Q1'), b['batch_obs'], b['batch_actions'], b['batch_targets'], inv_b_global=inv_b,
                        grad_out=self.grad('Q1'), loss_out=stats[0:1])                               # :162-172
        ops.dpg_policy_grad(self.cfg, pw.net('policy'), pw.net('Q1'), b['batch_obs'], inv_b_global=inv_b,
                            grad_out=self.grad('policy'), stats_out=stats[2:4])                      # :174-186
        return self._finish(iteration)

    def _native_lazy_stats(self, iteration):
        stats, B = self.flat[self.n_grad:], self.batch_size * D.world_size()

        def lazy():        # evaluated only when get_stats() is called: no elementwise launches in the training loop
            mean = stats[2] / B
            # (mb_targets_mean: this process's batch, like the reference's np.mean(mb_targets))
            return dict(q_loss=stats[0], policy_loss=-mean, value_mean=mean, value_var=stats[3] / B - mean * mean,
                        mb_targets_mean=self.batch_data['batch_targets'].mean(), q_gradient_norm=self.norms[0],
                        policy_gradient_norm=self.norms[1])
        return lazy


class SACLearner(_LearnerBase):
    """Soft actor-critic (learners/sac.py:21-219): networks [Q1 | Q2 | policy], the policy a diagonal Gaussian over its four logits
    (policy.py:179-204, no action range): PathTracking-v0.  With args.squashed_head the Gaussian sits under the tanh-affine bijectors of
    args.action_range (policy.py:183-190; the mpg_*_squashed entry points): PathTracking-v0 with a range, and InvertedPendulumConti-v0
    (built_SAC_parser of train_script4mujoco.py) - fixed or learned temperature, either buffer, any number of ranks.
    Every draw is the library's Philox stream keyed by (learner seed, call counter): two per gradient call - the action at s' for the
    target (from the ONLINE policy, sac.py:71) and the action of the policy loss (:123) - and one more, from the TARGET policy, for a
    prioritized buffer's td error (:88).
    alpha = 'auto' (with args.target_entropy): the temperature is learned (:138-148).  It stays on the device - the kernels read
    log_alpha there, nothing in the step reads it on the host - its loss takes a third draw (stream seed + 2, the call counter), its
    gradient travels as one more float between the networks' gradients and the statistics ([grads | alpha grad | stats]: one
    all-reduce), and compute_gradient returns it as the 19th array."""

    def __init__(self, policy_cls, args, device='cuda'):
        self.auto_alpha = getattr(args, 'alpha', None) == 'auto'
        if self.auto_alpha and getattr(args, 'target_entropy', None) is None:
            raise ValueError("SACLearner: alpha = 'auto' needs args.target_entropy (the reference's parser adds it with 'auto' only, "
                             "train_script.py:672-792; sac.py:144 reads it): default_args('SAC', alpha='auto', target_entropy=-2.)")
        if getattr(args, 'deterministic_policy', True):
            raise ValueError('SACLearner needs deterministic_policy=False (built_SAC_parser, train_script.py:672-792)')
        # the tanh-squashed head (args.squashed_head, on request): PathTracking-v0 with an action_range, and InvertedPendulumConti-v0
        self.squashed = bool(getattr(args, 'squashed_head', False))
        if self.squashed and args.env_id not in ('PathTracking-v0', 'InvertedPendulumConti-v0'):
            raise ValueError('SACLearner with squashed_head=True serves PathTracking-v0 and InvertedPendulumConti-v0 (got env_id %r)'
                             % (args.env_id,))
        if not self.squashed and args.env_id != 'PathTracking-v0':
            raise ValueError('SACLearner serves PathTracking-v0 only (got env_id %r): the pendulum\'s action_range is a tanh-affine '
                             'bijector whose log-density correction is not built' % (args.env_id,))
        super().__init__(policy_cls, args, device)
        assert self.policy_with_value.names == ['Q1', 'Q2', 'policy'], 'SAC trains [Q1 | Q2 | policy]: double_Q=True, target=True'
        self.n_net_grad = self.n_grad
        if self.auto_alpha:          # one more gradient float behind the networks'; the statistics follow it
            self.n_grad += 1
            self.flat = torch.zeros(self.n_grad + N_STATS, dtype=torch.float32, device=self.device)

    @property
    def alpha(self):
        return self.policy_with_value.alpha

    def _op(self, call, learned):
        """ops.<call>[_squashed][_auto] for this learner's head, looked up at call time"""
        return getattr(ops, call + ('_squashed' if self.squashed else '') + ('_auto' if learned else ''))

    def _draw(self, rows, ctr, stream=0):
        ad = self.cfg.act_dim
        return ops.normal_fill(rows * ad, self.seed + stream, ctr, self.device).view(rows, ad)

    def compute_clipped_double_q_target(self, eps_target=None):
        """sac.py:67-80"""
        pw, b = self.policy_with_value, self.batch_data
        if eps_target is None:
            eps_target = self._draw(b['batch_obs'].shape[0], 2 * (self.counter + 1))
        return self._op('sac_targets', self.auto_alpha)(self.cfg, pw.net('policy'), pw.net('Q1', True), pw.net('Q2', True), b['batch_rewards'],
                                                         b['batch_obs_tp1'], eps_target, pw.log_alpha if self.auto_alpha else self.alpha)

    def compute_td_error(self, eps=None, ctr=None):
        """sac.py:82-91 (signed): r~ + gamma Q1_target(s', a') - Q1(s, a), a' its own draw from the TARGET policy - the soft target's
        launch sequence with the target policy, one critic in both places and alpha 0 (0 * logp is an exact zero).
        ctr: the draw's counter in the learner's second stream (default 2 * counter: the call from get_batch_data)"""
        pw, b = self.policy_with_value, self.batch_data
        if eps is None:
            eps = self._draw(b['batch_obs'].shape[0], 2 * self.counter if ctr is None else ctr, stream=1)
        y1 = self._op('sac_targets', False)(self.cfg, pw.net('policy', True), pw.net('Q1', True), pw.net('Q1', True), b['batch_rewards'],
                                            b['batch_obs_tp1'], eps, 0.0)
        return y1 - pw.compute_Q1(b['batch_obs'], b['batch_actions'])

    def get_batch_data(self, batch_data, rb, indexes, eps_target=None):
        self._get_batch(batch_data)
        self.batch_data['batch_targets'] = self.compute_clipped_double_q_target(eps_target)
        if self.args.buffer_type != 'normal':
            self.info_for_buffer.update(dict(td_error=self.compute_td_error(), rb=rb, indexes=indexes))

    def compute_gradient(self, batch_data, rb, indexes, iteration, eps_target=None, eps_policy=None, eps_alpha=None):
        """sac.py:169-219; output order q1 + q2 + policy (+ the temperature's gradient, a 0-d array, with alpha = 'auto')"""
        pw, b, rows, inv_b, stats = self._begin(batch_data, rb, indexes, eps_target)
        if self.args.buffer_type != 'normal':                  # :173-174: the priorities follow the critic within a reused batch
            self.info_for_buffer.update(dict(td_error=self.compute_td_error(ctr=2 * self.counter - 1)))
        for i, nm in enumerate(('Q1', 'Q2')):                                                          # :102-117
            ops.q_loss_grad(self.cfg, pw.net(nm), b['batch_obs'], b['batch_actions'], b['batch_targets'], inv_b_global=inv_b,
                            grad_out=self.grad(nm), loss_out=stats[i:i + 1])
        if eps_policy is None:
            eps_policy = self._draw(rows, 2 * self.counter + 1)
        grad_fn = self._op('sac_policy_grad', self.auto_alpha)
        if not self.auto_alpha:
            grad_fn(self.cfg, pw.net('policy'), pw.net('Q1'), pw.net('Q2'), b['batch_obs'], eps_policy, self.alpha, inv_b_global=inv_b,
                    grad_out=self.grad('policy'), stats_out=stats[2:5])                                    # :119-136
            return self._finish(iteration)
        if eps_alpha is None:                                                                          # :139: the third draw
            eps_alpha = self._draw(rows, self.counter, stream=2)
        g_alpha = self.flat[self.n_net_grad:self.n_grad]
        grad_fn(self.cfg, pw.net('policy'), pw.net('Q1'), pw.net('Q2'), b['batch_obs'], eps_policy, pw.log_alpha, eps_alpha, pw.target_entropy,
                inv_b_global=inv_b, grad_out=self.grad('policy'), stats_out=stats[2:5], alpha_grad_out=g_alpha)   # :119-148
        fresh = self._views is None
        views = self._finish(iteration)
        if fresh:
            views.append(g_alpha.view(()))                                                             # :216: the last gradient
        # the temperature's own clip (alone in its list, :146) and the snapshot the statistics read
        ops.sac_alpha_update(pw.alpha_desc, g_alpha, clip=float(self.args.gradient_clip_norm), do_clip=True)
        return views

    def _native_lazy_stats(self, iteration):
        stats, B, alpha = self.flat[self.n_grad:], self.batch_size * D.world_size(), self.alpha

        def lazy():        # evaluated only when get_stats() is called: no elementwise launches in the training loop
            mean, logp = stats[2] / B, stats[4] / B
            extra = {}
            if self.auto_alpha:
                # the snapshot mpg_sac_alpha_update took at the gradient call: alpha BEFORE the update that follows it (sac.py:189)
                snap = self.policy_with_value.alpha_state
                extra = dict(alpha=snap[ops.ALPHA_SNAPSHOT], alpha_loss=snap[ops.ALPHA_LOSS], alpha_gradient_norm=snap[ops.ALPHA_NORM],
                             alpha_time=None)
            a = extra['alpha'] if self.auto_alpha else alpha
            return dict(extra, q_loss1=stats[0], q_loss2=stats[1], policy_loss=a * logp - mean, policy_entropy=-logp,
                        mb_targets_mean=self.batch_data['batch_targets'].mean(), value_mean=mean, value_var=stats[3] / B - mean * mean,
                        q_gradient_norm1=self.norms[0], q_gradient_norm2=self.norms[1], policy_gradient_norm=self.norms[2])
        return lazy
