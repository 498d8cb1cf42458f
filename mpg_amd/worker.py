"""OffPolicyWorker - device mirror of worker.py:25-123: the env-step producer that also owns the master weights and
the optimizer state (`apply_gradients`).  `sample()` keeps the reference's loop (policy -> + N(0, sigma) ->
env.step -> env.reset, worker.py:91-119) but every stage is one HIP launch over all `num_agent` agents.  With
`args.one_launch_sample = True` and a deterministic policy all iterations of a sample are ONE launch, bit-identical to the
loop: mpg_worker_rollout on PathTracking-v0, mpg_worker_rollout_pendulum on InvertedPendulumConti-v0 (where the reference's
defaults make a sample one agent's 512 iterations) - and there also with the tanh-squashed Gaussian policy (squashed_head=True):
mpg_worker_sample_rollout_pendulum.  A stochastic policy on PathTracking-v0 (SAC: the Gaussian head or the squashed one) takes
mpg_worker_sample_rollout.  With `args.env_on_model = True` the env is the model-backed one (envs.make_model_env:
InvertedDoublePendulum-v2, whose real env is not provided); its one-launch sample is mpg_worker_rollout_model."""
import torch

from .envs import make_env, make_model_env
from . import ops

# args.one_launch_sample, stated once: (env.kind, stochastic policy) -> the method sample() takes, what it says to the other policy kind
# and to another env (% the env's class), and how it names itself where it bounds the iterations (None: only the library's own bound).
# _one_launch_checked raises them; ops.worker_rollout / ops.worker_sample_rollout choose the entry point by cfg.env_kind.
ONE_LAUNCH = {
    (0, False): ('_sample_one_launch',
                 '_sample_one_launch serves a deterministic policy only (a stochastic one takes _sample_one_launch_stochastic)',
                 'one_launch_sample serves PathTracking-v0 only (the env is %s)', None),
    (1, False): ('_sample_one_launch_pendulum',
                 'one_launch_sample on the pendulum serves a deterministic policy only: a one-launch step for the stochastic or squashed '
                 'policy is not built for this env',
                 '_sample_one_launch_pendulum serves InvertedPendulumConti-v0 only (the env is %s)', 'on the pendulum'),
    (1, True): ('_sample_one_launch_stochastic_pendulum',
                '_sample_one_launch_stochastic_pendulum serves a stochastic policy (a deterministic one takes _sample_one_launch_pendulum)',
                '_sample_one_launch_stochastic_pendulum serves InvertedPendulumConti-v0 only (the env is %s)', 'with the squashed head'),
    (2, False): ('_sample_one_launch_model',
                 'one_launch_sample on the model env serves a deterministic policy only: a one-launch step for a stochastic policy is '
                 'not built for this env',
                 '_sample_one_launch_model serves the model-backed InvertedDoublePendulum-v2 env only (the env is %s)', 'on the model env'),
    (0, True): ('_sample_one_launch_stochastic',
                '_sample_one_launch_stochastic serves a stochastic policy (a deterministic one takes _sample_one_launch)',
                '_sample_one_launch_stochastic serves PathTracking-v0 only (the env is %s)', 'with a stochastic policy'),
}


class OffPolicyWorker(object):
    def __init__(self, policy_cls, env_id, args, worker_id, device='cuda'):
        self.worker_id = worker_id
        self.args = args
        self.device = torch.device(device)
        self.num_agent = int(args.num_agent)
        seed = int(getattr(args, 'seed', 0)) * 1000003 + int(worker_id)
        # PathTracking-v0, or InvertedPendulumConti-v0 (the reference wraps the single MuJoCo env in DummyVecEnv with
        # num_agent 1, train_script4mujoco.py:328; here `num_agent` pendulums step in one launch)
        # args.env_on_model = True: the env is the differentiable MODEL of env_id made an env (envs.make_model_env: InvertedDoublePendulum-v2,
        # whose real env is not provided; args.max_episode_steps, default 1000, is its episode limit)
        if getattr(args, 'env_on_model', False):
            self.env = make_model_env(env_id, num_agent=self.num_agent, device=device, seed=seed,
                                      max_episode_steps=getattr(args, 'max_episode_steps', 1000))
        else:
            self.env = make_env(env_id, num_agent=self.num_agent, num_future_data=getattr(args, 'num_future_data', 0), device=device, seed=seed)
        self.policy_with_value = policy_cls(**vars(args), device=device)
        self.batch_size = int(args.batch_size)
        self.obs = self.env.reset()
        self.explore_sigma = args.explore_sigma
        self.seed = seed
        self.iteration = 0
        self.num_sample = 0
        self.sample_times = 0
        self.nan_check_interval = int(getattr(args, 'nan_check_interval', 100))
        self._noise_ctr = 0
        self.stats = {}

    def get_stats(self):
        self.stats.update(dict(worker_id=self.worker_id, num_sample=self.num_sample))
        return self.stats

    def get_weights(self):
        return self.policy_with_value.get_weights()

    def set_weights(self, weights):
        return self.policy_with_value.set_weights(weights)

    def save_weights(self, save_dir, iteration):
        self.policy_with_value.save_weights(save_dir, iteration)

    def load_weights(self, load_dir, iteration):
        self.policy_with_value.load_weights(load_dir, iteration)

    def apply_gradients(self, iteration, grads):
        self.iteration = iteration
        self.policy_with_value.apply_gradients(iteration, grads)

    def get_ppc_params(self):
        return {}

    def set_ppc_params(self, params):
        pass

    def sample(self):
        """-> (obs, act, RAW reward, obs', done) stacked over batch_size/num_agent env steps (worker.py:91-119)."""
        iters = max(1, self.batch_size // self.num_agent)
        if not getattr(self.args, 'one_launch_sample', False):
            batch = self._sample_loop(iters)
        else:       # (an env kind without a row of its own: _sample_one_launch, which refuses it)
            stochastic = not getattr(self.policy_with_value, 'deterministic_policy', True)
            batch = getattr(self, ONE_LAUNCH.get((self.env.kind, stochastic), ONE_LAUNCH[0, False])[0])(iters)
        self.num_sample += batch[0].shape[0]
        self.sample_times += 1
        # judge_is_nan (worker.py:95-107) runs inside the policy kernel: a NaN observation or action sets MPG_STATUS_NAN in the
        # policy's status word; it is read (one host synchronisation) every `nan_check_interval` calls, not per step
        if self.sample_times % self.nan_check_interval == 0:
            self.policy_with_value.check_status()
        return batch

    def _sample_loop(self, iters):
        pw = self.policy_with_value
        out = [[], [], [], [], []]
        for _ in range(iters):
            obs = self.obs
            if getattr(pw, 'deterministic_policy', True):
                action = ops.policy_action(pw.cfg, pw.net('policy'), obs, explore_sigma=float(self.explore_sigma or 0.),
                                           seed=self.seed, ctr=self._noise_ctr)
            else:
                # stochastic policy: the action IS the sample (worker.py:96), un-clipped; explore_sigma noise only if it is set (:97-98)
                n = obs.shape[0] * pw.act_dim
                action, _ = pw.compute_action(obs, ops.normal_fill(n, self.seed, self._noise_ctr, self.device).view(obs.shape[0], pw.act_dim))
                if self.explore_sigma is not None:
                    action.add_(ops.normal_fill(n, self.seed + 1, self._noise_ctr, self.device).view_as(action), alpha=float(self.explore_sigma))
            self._noise_ctr += 1
            obs_tp1, reward, done, _ = self.env.step(action)          # fresh tensors every call (never aliased later)
            for lst, x in zip(out, (obs, action, reward, obs_tp1, done)):
                lst.append(x)
            self.obs = self.env.reset()          # PathTracking: done is always 1, every agent is re-drawn; the pendulum
                                                 # re-draws the agents that fell (inverted_pendulum_conti.py:17-18)
        return tuple(x[0] for x in out) if iters == 1 else tuple(torch.cat(x, 0) for x in out)

    def _sample_one_launch(self, iters):
        """args.one_launch_sample = True: the same batch, observations, env state and counters as _sample_loop, bit for bit, from ONE
        launch (mpg_worker_rollout) instead of three per iteration - the five output arrays [iters * n, .] are the launch's ring of
        capacity iters * n at position 0.  Deterministic policy on PathTracking-v0 only.  env.done_intended is NOT refreshed on this
        path (the launch does not form it; env.step does).  The three methods below keep this contract over consecutive calls."""
        return self._one_launch_checked(0, False, iters)

    def _sample_one_launch_pendulum(self, iters):
        """_sample_one_launch for InvertedPendulumConti-v0: mpg_worker_rollout_pendulum (the reference's pendulum worker: one agent, 512
        iterations).  Deterministic policy only, at most 1024 iterations."""
        return self._one_launch_checked(1, False, iters)

    def _sample_one_launch_model(self, iters):
        """_sample_one_launch for the model-backed InvertedDoublePendulum-v2 env (args.env_on_model): mpg_worker_rollout_model (the
        reference-shaped defaults make a sample one agent's 512 iterations).  Deterministic policy only, at most 1024 iterations."""
        return self._one_launch_checked(2, False, iters)

    def _sample_one_launch_stochastic_pendulum(self, iters):
        """_sample_one_launch_pendulum for the tanh-squashed Gaussian policy (squashed_head=True: SAC with an action range, the one
        stochastic head built for this env): mpg_worker_sample_rollout_pendulum instead of the loop's launches per iteration (the draw,
        the policy pass, the head's row sums, env.step, env.reset).  No explore_sigma (the loop adds that noise with a torch op, which
        has no place in the launch), at most 1024 iterations."""
        return self._one_launch_checked(1, True, iters)

    def _sample_one_launch_stochastic(self, iters):
        """_sample_one_launch for a stochastic policy on PathTracking-v0 (SAC: the Gaussian head, or with squashed_head=True the
        tanh-squashed one): mpg_worker_sample_rollout.  No explore_sigma, at most 1024 iterations."""
        return self._one_launch_checked(0, True, iters)

    def _one_launch_checked(self, kind, stochastic, iters):
        """the one-launch contract of ONE_LAUNCH[kind, stochastic]: its refusals - the policy kind, the head, explore_sigma, the env, the
        iteration count, in that order, each a ValueError before anything touches the device - and then the launch"""
        _, wrong_policy, wrong_env, too_many = ONE_LAUNCH[kind, stochastic]
        pw, env = self.policy_with_value, self.env
        if stochastic == bool(getattr(pw, 'deterministic_policy', True)):
            raise ValueError(wrong_policy)
        if stochastic and kind == 1 and not getattr(pw, 'squashed_head', False):
            raise ValueError('one_launch_sample on the pendulum serves the tanh-squashed head only (squashed_head=True): a stochastic '
                             'policy without an action range is not built for this env')
        if stochastic and self.explore_sigma is not None:
            raise ValueError('one_launch_sample with a stochastic policy takes no explore_sigma (got %r): the action is the sample'
                             % (self.explore_sigma,))
        if env.kind != kind:
            raise ValueError(wrong_env % type(env).__name__)
        if too_many and iters > 1024:
            raise ValueError('one_launch_sample %s takes at most 1024 iterations per launch (batch_size / num_agent = %d)' % (too_many, iters))
        return self._one_launch(iters, sampled=stochastic)

    def _one_launch(self, iters, sampled=False):
        """ops.worker_rollout (sampled: ops.worker_sample_rollout, the draw keyed as the loop keys it: (seed, _noise_ctr)) on a fresh
        ring of capacity iters * n at position 0, then the bookkeeping of `iters` loop iterations"""
        pw, env, n, dev = self.policy_with_value, self.env, self.num_agent, self.device
        rows, od = iters * n, env.obs_dim
        f = dict(dtype=torch.float32, device=dev)
        ring = (torch.empty(rows, od, **f), torch.empty(rows, pw.act_dim, **f), torch.empty(rows, **f), torch.empty(rows, od, **f),
                torch.empty(rows, dtype=torch.uint8, device=dev))
        obs_io = self.obs.clone()               # never write into a tensor already handed to the caller
        done = torch.empty(n, dtype=torch.uint8, device=dev)
        if sampled:
            ops.worker_sample_rollout(pw.cfg, pw.net('policy'), iters, env._state, obs_io, self.seed, self._noise_ctr, ring, rows, 0, env.seed,
                                      env._ctr, done_out=done)
        else:
            ops.worker_rollout(pw.cfg, pw.net('policy'), iters, env._state, obs_io, float(self.explore_sigma or 0.), self.seed, self._noise_ctr,
                               ring, rows, 0, env.seed, env._ctr, done_out=done, max_steps=getattr(env, 'max_episode_steps', 0))
        self._noise_ctr += iters
        env._ctr += iters
        env.obs, env.done, env.reward = obs_io, done, ring[2][rows - n:]
        self.obs = obs_io
        return ring

    def sample_with_count(self):
        batch = self.sample()
        return batch, batch[0].shape[0]
