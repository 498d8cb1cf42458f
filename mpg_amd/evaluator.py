"""Evaluator - device mirror of evaluator.py:25-236: deterministic fixed-length episodes on the HIP env -
parallel ones (run_n_episodes_parallel) or serial ones (run_n_episodes) - and the reference's per-episode metrics
(evaluator.py:160-211), averaged over the episodes.  Not on the throughput path; it is the learning-curve check that the fast path
still learns (the reference's plots use a base score of -30, ploter.py:85).

`args.one_launch_eval = True` (named like args.one_launch_sample; off by default): all steps of an evaluation are ONE launch
(ops.eval_rollout: mpg_eval_rollout on PathTracking-v0, mpg_eval_rollout_pendulum on InvertedPendulumConti-v0, bit-identical to the
2 * fixed_steps launches of the loop), the metrics a second one (ops.eval_metrics, float64 on the device) and ONE copy brings them to
the host; run_evaluation then follows evaluator.py:222-225 (one eval agent: num_eval_episode serial episodes).

ModelEvaluator (below) runs the same episodes on the differentiable MODEL - the only evaluation InvertedDoublePendulum-v2 has here -
and measures the model's gap to the env where both exist."""
import torch

from . import ops
from .envs import ENV_KIND, make_env

MAX_ONE_LAUNCH_STEPS = 1024      # what mpg_eval_rollout accepts (it bounds one launch's run time)


class Evaluator(object):
    def __init__(self, policy_cls, env_id, args, device='cuda'):
        self.env_id = env_id
        self.args = args
        self.device = torch.device(device)
        self.num_eval_agent = int(getattr(args, 'num_eval_agent', 5))
        self.num_eval_episode = int(getattr(args, 'num_eval_episode', 5))
        self.fixed_steps = int(getattr(args, 'fixed_steps', 200))
        self.one_launch_eval = bool(getattr(args, 'one_launch_eval', False))
        self._check_one_launch_steps()
        self.env = make_env(env_id, num_agent=self.num_eval_agent, num_future_data=getattr(args, 'num_future_data', 0), device=device,
                            seed=int(getattr(args, 'seed', 0)) + 424242)
        self.policy_with_value = policy_cls(**vars(args), device=device)
        self.iteration = 0
        self.stats = {}

    def _check_one_launch_steps(self):
        if self.one_launch_eval and self.fixed_steps > MAX_ONE_LAUNCH_STEPS:
            raise ValueError('one_launch_eval takes at most %d steps per launch (fixed_steps = %d)' % (MAX_ONE_LAUNCH_STEPS, self.fixed_steps))

    def set_weights(self, weights):
        if weights is self.policy_with_value:
            return
        self.policy_with_value.set_weights(weights)

    def share_policy(self, policy):
        self.policy_with_value = policy

    def set_ppc_params(self, params):
        pass

    def _reset(self, init_obs=None):
        if init_obs is not None:
            return self.env.reset(init_obs=init_obs)
        self.env._initialised = False                      # fresh draw of every agent
        return self.env.reset()

    def _episodes_by_the_loop(self, obses):
        """evaluator.py:132-152 from the observations `obses` of the env's current state: `fixed_steps` times compute_mode and env.step,
        then the metrics of every agent's episode, as float64 device tensors [num_eval_agent]"""
        pw = self.policy_with_value
        obs_l, act_l, rew_l = [], [], []
        for _ in range(self.fixed_steps):
            actions = ops.policy_action(pw.cfg, pw.net('policy'), obses)      # compute_mode, policy.py:173-177
            obs_l.append(obses)
            act_l.append(actions)
            obses, rewards, _, _ = self.env.step(actions)
            rew_l.append(rewards)
        # the reference accumulates in numpy: np.mean / python sum() promote to float64 (evaluator.py:141-142,172-178)
        obs, act, rew = torch.stack(obs_l).double(), torch.stack(act_l).double(), torch.stack(rew_l).double()   # [T, N, .]
        rms = lambda x: torch.sqrt(torch.mean(torch.square(x), 0))
        per_episode = dict(episode_return=rew.sum(0), episode_len=torch.full_like(rew[0], float(self.fixed_steps)))
        if self.env_id == 'PathTracking-v0':               # metrics_for_an_episode, evaluator.py:160-184
            per_episode.update(
                delta_y_mse=rms(obs[:, :, 3]), delta_phi_mse=rms(obs[:, :, 4]), delta_v_mse=rms(obs[:, :, 0]),
                stationary_rew_mean=rew[20:].mean(0), steer_mse=rms(act[:, :, 0] * (1.2 * 3.141592653589793 / 9)),
                acc_mse=rms(act[:, :, 1] * 3.))
        else:                                              # InvertedPendulumConti-v0, evaluator.py:185-211
            for j, nm in enumerate(('x', 'theta', 'xdot', 'thetadot')):
                per_episode[nm + '_mean'] = obs[:, :, j].mean(0)
                per_episode[nm + '_var'] = obs[:, :, j].var(0, unbiased=False)
                per_episode[nm + '_mse'] = rms(obs[:, :, j])
                per_episode[nm + '_mse_25'] = rms(obs[:25, :, j])
        return per_episode

    def _episodes_in_one_launch(self, state, obs):
        """The same episodes from (state [8, rows], obs [rows, obs_dim]) by ops.eval_rollout and ops.eval_metrics: two launches and one
        copy to the host.  `state` is advanced in place.  Returns (per_episode, mean, last_obs, the done flags of the last step, the
        rewards [steps, rows]): per_episode's values are float64 HOST tensors [rows], in the reference's key order."""
        self._check_one_launch_steps()
        pw = self.policy_with_value
        out = ops.eval_rollout(pw.cfg, pw.net('policy'), state, obs, self.fixed_steps)
        obs_traj, act_traj, rew_traj, last_obs = out[:4]
        keys, rows = ops.EVAL_METRIC_KEYS[self.env.kind], obs.shape[0]
        host = ops.eval_metrics_flat(self.env.kind, obs_traj, act_traj, rew_traj).cpu()     # ONE device-to-host copy: [K * rows | K]
        per_episode = {k: host[j * rows:(j + 1) * rows] for j, k in enumerate(keys)}
        mean = {k: float(host[len(keys) * rows + j]) for j, k in enumerate(keys)}
        pw.check_status()          # NaN observations / actions, the engine's envelope: an evaluation on invalid numbers raises
        return per_episode, mean, last_obs, out[4:], rew_traj

    def _leave_env(self, last_obs, done, reward):
        """what `fixed_steps` env.step calls leave in the env's attributes (the state block was advanced in place)"""
        env = self.env
        env.obs, env.reward, env.done = last_obs, reward, done[0]
        # (the pendulum's step writes `done` into both flags)
        env.done_intended = done[1] if len(done) > 1 else done[0].clone()

    def run_n_episodes_parallel(self, n=None, init_obs=None):
        """evaluator.py:118-156: reset, `fixed_steps` deterministic steps (done is ignored), metrics per episode.
        init_obs (optional, [num_eval_agent, obs_dim]): start from these observations instead of a fresh reset() draw
        (the parity test starts from the states the reference's own env drew).
        With args.one_launch_eval the per-episode values are float64 HOST tensors (they came over in the one copy); without, float64
        device tensors as before."""
        pw = self.policy_with_value
        obses = self._reset(init_obs)
        if self.one_launch_eval:
            per_episode, mean, last_obs, done, rew = self._episodes_in_one_launch(self.env._state, obses)
            self._leave_env(last_obs, done, rew[-1])
            return per_episode, mean
        per_episode = self._episodes_by_the_loop(obses)
        mean = {k: float(v.mean().item()) for k, v in per_episode.items()}
        pw.check_status()          # NaN observations / actions, the engine's envelope: an evaluation on invalid numbers raises
        return per_episode, mean

    def run_n_episodes(self, n):
        """evaluator.py:112-122: `n` serial episodes of `fixed_steps` steps on the evaluator's env, each from a fresh reset() of every
        agent (the env's draw counter advances per episode), and the mean of every metric over the n * num_eval_agent episodes (episode
        e's agent a is entry e * num_eval_agent + a).
        With args.one_launch_eval the n resets come first, their states and observations are concatenated and ONE rollout launch and one
        metrics launch serve all rows: the rows are independent, so the trajectories equal the serial ones bit for bit.  The env is left
        holding the last episode's state, observation and done flags either way."""
        n = int(n)
        assert n >= 1, n
        pw, env, A = self.policy_with_value, self.env, self.num_eval_agent
        if self.one_launch_eval:
            self._check_one_launch_steps()
            states, obs = [], []
            for _ in range(n):
                obs.append(self._reset())
                states.append(env._state.clone())
            state = torch.cat(states, 1).contiguous() if n > 1 else states[0]
            per_episode, mean, last_obs, done, rew = self._episodes_in_one_launch(state, torch.cat(obs, 0) if n > 1 else obs[0])
            env._state.copy_(state[:, (n - 1) * A:])
            self._leave_env(last_obs[(n - 1) * A:].clone(), [d[(n - 1) * A:].clone() for d in done], rew[-1, (n - 1) * A:].clone())
            return per_episode, mean
        episodes = [self._episodes_by_the_loop(self._reset()) for _ in range(n)]
        per_episode = {k: torch.cat([e[k] for e in episodes]) for k in episodes[0]}
        mean = {k: float(v.mean().item()) for k, v in per_episode.items()}
        pw.check_status()
        return per_episode, mean

    def run_evaluation(self, iteration):
        self.iteration = iteration
        if self.one_launch_eval and self.num_eval_agent == 1:      # evaluator.py:222-223
            _, mean = self.run_n_episodes(self.num_eval_episode)
        else:
            _, mean = self.run_n_episodes_parallel()
        self.stats = dict(iteration=iteration, **mean)
        return mean



class ModelEvaluator(object):
    """The evaluator on the differentiable MODEL instead of the env (inverted_double_pendulum_model.py:245-265: model.reset(obs), then
    compute_action -> rollout_out in a loop): `fixed_steps` deterministic steps of every episode in ONE launch (ops.model_rollout).
    It serves the three models, InvertedDoublePendulum-v2 included, whose real env does not exist here - there the start observations
    have to be given, and the metrics are the two the reference gives an env id it has no branch for.  On PathTracking-v0 and
    InvertedPendulumConti-v0 the record has eval_rollout's layout and the metrics are ops.eval_metrics on it: one more launch, one copy."""

    def __init__(self, policy_cls, env_id, args, device='cuda'):
        self.env_id = env_id
        self.args = args
        self.device = torch.device(device)
        self.kind = ENV_KIND[env_id]
        self.num_eval_agent = int(getattr(args, 'num_eval_agent', 5))
        self.fixed_steps = int(getattr(args, 'fixed_steps', 200))
        if not 1 <= self.fixed_steps <= MAX_ONE_LAUNCH_STEPS:
            raise ValueError('a model evaluation takes 1 .. %d steps per launch (fixed_steps = %d)' % (MAX_ONE_LAUNCH_STEPS, self.fixed_steps))
        # the two envs that exist: the start observations' reset law, and the env side of gap_to_env
        self.env = None
        if self.kind != ENV_KIND[ops.DOUBLE_PENDULUM]:
            self.env = make_env(env_id, num_agent=self.num_eval_agent, num_future_data=getattr(args, 'num_future_data', 0), device=device,
                                seed=int(getattr(args, 'seed', 0)) + 424242)
        self.policy_with_value = policy_cls(**vars(args), device=device)

    def set_weights(self, weights):
        if weights is self.policy_with_value:
            return
        self.policy_with_value.set_weights(weights)

    def share_policy(self, policy):
        self.policy_with_value = policy

    def _start(self, init_obs):
        if init_obs is None:
            if self.env is None:
                raise ValueError('%s: init_obs is required - there is no env for this id here (the real one is MuJoCo), hence no reset law '
                                 'to draw start observations from' % self.env_id)
            self.env._initialised = False                  # fresh draw of every agent
            return self.env.reset()
        return init_obs.to(self.device, torch.float32).contiguous()

    def run_n_episodes_parallel(self, init_obs=None, eps=None):
        """One episode per row of init_obs ([rows, obs_dim]; default: a reset() draw of num_eval_agent rows) on the model, eps
        [fixed_steps, rows] its standard-normal noise (None: the noise terms at their means).  Returns (per_episode, mean) in the
        reference's key order, per_episode's values float64 HOST tensors [rows]."""
        pw = self.policy_with_value
        obs = self._start(init_obs)
        rows = obs.shape[0]
        obs_traj, act_traj, rew_traj, _ = ops.model_rollout(pw.cfg, pw.net('policy'), obs, self.fixed_steps, eps)
        if self.env is None:
            ret = rew_traj.double().sum(0).cpu()           # python's sum() over an episode's rewards promotes to float64
            per_episode = dict(episode_return=ret, episode_len=torch.full((rows,), float(self.fixed_steps), dtype=torch.float64))
            mean = {k: float(v.mean().item()) for k, v in per_episode.items()}
        else:
            keys = ops.EVAL_METRIC_KEYS[self.kind]
            host = ops.eval_metrics_flat(self.kind, obs_traj, act_traj, rew_traj).cpu()     # ONE device-to-host copy: [K * rows | K]
            per_episode = {k: host[j * rows:(j + 1) * rows] for j, k in enumerate(keys)}
            mean = {k: float(host[len(keys) * rows + j]) for j, k in enumerate(keys)}
        pw.check_status()          # NaN observations / actions, the engine's envelope: an evaluation on invalid numbers raises
        return per_episode, mean

    @staticmethod
    def gap_of_records(env_record, model_record):
        """(obs_traj, act_traj, rew_traj) of the env and of the model from one start: per step the mean over the episodes of the
        absolute difference of every observation column (obs_gap [steps, obs_dim]) and of the reward (rew_gap [steps]), and the two mean
        returns - float64 host tensors and floats.  A measurement: no threshold is attached."""
        (eo, _, er), (mo, _, mr) = [[x.double() for x in r] for r in (env_record, model_record)]
        return dict(obs_gap=(eo - mo).abs().mean(1).cpu(), rew_gap=(er - mr).abs().mean(1).cpu(),
                    env_return=float(er.sum(0).mean().item()), model_return=float(mr.sum(0).mean().item()))

    def gap_to_env(self, init_obs=None, eps=None):
        """The env's closed loop (ops.eval_rollout) and the model's (ops.model_rollout) under the same policy from the same start
        observations ([num_eval_agent, obs_dim]; default: a reset() draw), step by step (inverted_double_pendulum_model.py:203-242):
        gap_of_records of the two records.  For the two envs that exist."""
        if self.env is None:
            raise ValueError('%s: gap_to_env compares with the env, and there is none for this id here' % self.env_id)
        pw = self.policy_with_value
        obs = self.env.reset(init_obs=init_obs) if init_obs is not None else self._start(None)
        env_record = ops.eval_rollout(pw.cfg, pw.net('policy'), self.env._state, obs, self.fixed_steps)[:3]
        model_record = ops.model_rollout(pw.cfg, pw.net('policy'), obs, self.fixed_steps, eps)[:3]
        pw.check_status()
        return self.gap_of_records(env_record, model_record)

    def gap_to_mpc(self, init_obs=None, horizon=None, iters=200, tol=0.):
        """How far the policy's horizon cost on the model is from what is attainable there, per start row of init_obs ([rows, obs_dim];
        default: a reset() draw where an env exists), noise terms at their means.  horizon None: the stack's
        num_rollout_list_for_policy_update[-1], the horizon the policy is trained on.
          policy_cost: the policy's closed loop (ops.model_rollout, `horizon` steps), its actions clamped to the box [-1, 1] and costed
            by mpc.model_mpc_cost_grad - so that both sides are one function's output; rollout_cost is - sum rew_traj of the loop itself
            (on the double pendulum the loop re-reads atan2 at every step, the cost carries the state: equal in exact arithmetic).
          mpc_cost: the lower of two solves (mpc.model_mpc_solve), one from zeros and one from the policy's own clamped actions; the
            second can only improve on its start point, so mpc_cost <= policy_cost for every row.
          gap = policy_cost - mpc_cost; mean_* the means over the rows.  Beside them the two device tensors policy_u and mpc_u [rows, horizon,
            act_dim], from_policy_won [rows] (which solve gave mpc_cost) and the two solves' info.
        The box is the tanh range: a policy whose action range is wider (the pendulum's default of 3) is measured at its clamped actions.
        float64 host tensors [rows] and floats.  A measurement: no threshold is attached."""
        from . import mpc as MPC
        pw = self.policy_with_value
        obs = self._start(init_obs)
        if horizon is None:
            horizon = int(self.args.num_rollout_list_for_policy_update[-1])
        _, act_traj, rew_traj, _ = ops.model_rollout(pw.cfg, pw.net('policy'), obs, int(horizon))
        u_pi = act_traj.permute(1, 0, 2).clamp(-1., 1.).contiguous()                      # [rows, horizon, act_dim]
        policy_cost = MPC.model_mpc_cost_grad(pw.cfg, obs, u_pi, want_grad=False)[0]
        from_zeros = MPC.model_mpc_solve(pw.cfg, obs, None, iters, tol, horizon=horizon)
        from_policy = MPC.model_mpc_solve(pw.cfg, obs, u_pi, iters, tol)
        better = from_policy[1] < from_zeros[1]
        mpc_cost = torch.where(better, from_policy[1], from_zeros[1])
        mpc_u = torch.where(better[:, None, None], from_policy[0], from_zeros[0])
        pw.check_status()
        out = dict(policy_cost=policy_cost.double().cpu(), mpc_cost=mpc_cost.double().cpu(), rollout_cost=-rew_traj.double().sum(0).cpu())
        out['gap'] = out['policy_cost'] - out['mpc_cost']
        for k in ('policy_cost', 'mpc_cost', 'gap'):
            out['mean_' + k] = float(out[k].mean().item())
        out.update(policy_u=u_pi, mpc_u=mpc_u, from_policy_won=better.cpu(), info_from_zeros=from_zeros[3].cpu(),
                   info_from_policy=from_policy[3].cpu())
        return out

    def gap_to_mpc_closed_loop(self, init_obs=None, steps=None, horizon=None, iters=200, tol=1e-3, warm_start=True, eps=None):
        """How the policy DRIVES on the model against what MPC attains there in closed loop, per start row of init_obs ([rows, obs_dim];
        default: a reset() draw where an env exists): the policy's closed loop (ops.model_rollout) and MPC's receding-horizon loop
        (mpc.run_model_mpc(one_launch=True): one solve per step at the noise means over `horizon` steps, the plan's first action applied)
        from the same start rows, `steps` steps each (None: fixed_steps) under the same plant noise eps [steps, rows] (None: the noise
        terms at their means).  horizon None: the stack's num_rollout_list_for_policy_update[-1].
          policy_return, mpc_return [rows]: the two sums of raw rewards; gap = mpc_return - policy_return; mean_* the means over the rows.
          mean_iters: the mean accepted iterations per solve (|info|, a failed search's -(k + 1) counted as k); failed_share: the share
            of solves whose info is negative.  Beside them the two records policy_record and mpc_record (device tensors).
        The policy acts in its own range and MPC in the box [-1, 1], the tanh range: a policy whose action range is wider (the
        pendulum's default of 3) can reach what MPC cannot.  The two loops' steps are the same model step under two compilation rules
        (run_model_mpc says how they differ).  float64 host tensors [rows] and floats.  A measurement: no threshold is attached."""
        from . import mpc as MPC
        pw = self.policy_with_value
        obs = self._start(init_obs)
        steps = self.fixed_steps if steps is None else int(steps)
        if horizon is None:
            horizon = int(self.args.num_rollout_list_for_policy_update[-1])
        eps = ops._model_eps(eps, (steps, obs.shape[0]), 'gap_to_mpc_closed_loop')
        obs_traj, act_traj, rew_traj, last_obs = ops.model_rollout(pw.cfg, pw.net('policy'), obs, steps, eps)
        rec = MPC.run_model_mpc(pw.cfg, obs, steps, int(horizon), iters, tol, warm_start, one_launch=True, eps=eps)
        pw.check_status()
        info = rec['info']
        accepted = torch.where(info < 0, -info - 1, info).double()
        out = dict(policy_return=rew_traj.double().sum(0).cpu(), mpc_return=rec['rew_traj'].double().sum(0).cpu())
        out['gap'] = out['mpc_return'] - out['policy_return']
        for k in ('policy_return', 'mpc_return', 'gap'):
            out['mean_' + k] = float(out[k].mean().item())
        out.update(mean_iters=float(accepted.mean().item()), failed_share=float((info < 0).double().mean().item()),
                   policy_record=dict(obs_traj=obs_traj, act_traj=act_traj, rew_traj=rew_traj, last_obs=last_obs), mpc_record=rec)
        return out
