"""The reference's MPC baseline, SLSQP form (mpc/main.py), on the device: the horizon cost, its gradient and a batched solver, and the
closed loop that measures a policy against it.  Names follow the reference.

Where mpc/main.py runs one scipy SLSQP solve with finite-difference gradients per env step (about 2 s each), ModelPredictiveControl
here holds B start states and solves all of them in ONE launch (mpg_mpc_solve: spectral projected gradient on the hand adjoint of the
25-step rollout; include/mpg_hip.h states the problem, the method and its constants), and the closed loop's MPC side runs as ONE launch
per chunk of steps (mpg_mpc_rollout).  The IPOPT form (mpc/mpc_ipopt.py) needs casadi and is not provided.

Below those, the same on the models the LEARNERS optimise through (model_mpc_cost_grad, model_mpc_solve, ModelMPC, run_model_mpc:
mpg_model_mpc_*): the reference's baseline solves main.py's own problem, which is not the model AMPC's objective is taken on."""
import ctypes

import torch

from . import _lib as L
from . import ops
from .envs import PathTrackingEnv

MAX_HORIZON, MAX_ITERS = 31, 1000        # MPG_MPC_MAX_HORIZON, MPG_MPC_MAX_ITERS
# MPG_MODEL_MPC_MAX_ITERS_PATH_TRACKING, _PENDULUM, _DOUBLE_PENDULUM by env kind: what mpg_model_mpc_solve accepts (a launch's run time)
MODEL_MAX_ITERS = {0: 1000, 1: 1000, 2: 400}
MAX_ROLLOUT_STEPS, MAX_ROLLOUT_WORK = 1024, 2048      # MPG_MPC_ROLLOUT_MAX_STEPS, MPG_MPC_ROLLOUT_MAX_WORK (steps * iters of one launch)
# MPG_MODEL_MPC_ROLLOUT_MAX_STEPS and MPG_MODEL_MPC_ROLLOUT_MAX_WORK_PATH_TRACKING, _PENDULUM, _DOUBLE_PENDULUM by env kind: steps * iters
# of one mpg_model_mpc_rollout launch
MODEL_MAX_ROLLOUT_STEPS = 1024
MODEL_MAX_ROLLOUT_WORK = {0: 2048, 1: 2048, 2: 400}


def _f32(t):
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.to(torch.float32).contiguous()


def mpc_cost_grad(x0, u, want_grad=True, want_traj=False):
    """mpg_mpc_cost_grad: x0 [B, 6], u [B, H, 2] -> (cost [B], grad [B, H, 2] or None, traj [B, H + 1, 6] or None), one launch"""
    rows, horizon = u.shape[0], u.shape[1]
    assert x0.shape == (rows, 6) and u.shape == (rows, horizon, 2), (x0.shape, u.shape)
    cost = torch.empty(rows, dtype=torch.float32, device=x0.device)
    grad = torch.empty(rows, horizon, 2, dtype=torch.float32, device=x0.device) if want_grad else None
    traj = torch.empty(rows, horizon + 1, 6, dtype=torch.float32, device=x0.device) if want_traj else None
    L.call('mpg_mpc_cost_grad', L.c_int(rows), L.c_int(horizon), L.ptr(_f32(x0)), L.ptr(_f32(u)), L.ptr(cost), L.ptr(grad), L.ptr(traj),
           L.stream())
    return cost, grad, traj


def mpc_solve(x0, u_init, iters=200, tol=0.):
    """mpg_mpc_solve: x0 [B, 6], u_init [B, H, 2] (left as it is) -> (u [B, H, 2], cost [B], pgnorm [B], info [B] int32), one launch"""
    rows, horizon = u_init.shape[0], u_init.shape[1]
    assert x0.shape == (rows, 6) and u_init.shape == (rows, horizon, 2), (x0.shape, u_init.shape)
    u = u_init.to(torch.float32).contiguous().clone()
    cost = torch.empty(rows, dtype=torch.float32, device=x0.device)
    pgnorm = torch.empty(rows, dtype=torch.float32, device=x0.device)
    info = torch.empty(rows, dtype=torch.int32, device=x0.device)
    L.call('mpg_mpc_solve', L.c_int(rows), L.c_int(horizon), L.c_int(int(iters)), L.c_float(float(tol)), L.ptr(_f32(x0)), L.ptr(u),
           L.ptr(cost), L.ptr(pgnorm), L.ptr(info), L.stream())
    return u, cost, pgnorm, info


class ModelPredictiveControl(object):
    """mpc/main.py:111-165.  init_x: [6] or [B, 6] on the device, [v_x, v_y, r, delta_y, delta_phi, x] with entry 0 the speed in m/s
    (compute_rew :133 reads it against expected_vs = 20).  Controls are normalised, [horizon, 2] (flat accepted) or [B, horizon, 2]."""

    def __init__(self, init_x, horizon):
        self.horizon = int(horizon)
        self.base_frequency = 10.
        self.num_future_data = 0
        self.expected_vs = 20.
        self.reset_init_x(init_x)

    def reset_init_x(self, init_x):
        self.single = init_x.dim() == 1
        self.init_x = _f32(init_x.reshape(-1, 6))

    def _u(self, u):
        return _f32(u.to(self.init_x.device).reshape(self.init_x.shape[0], self.horizon, 2))

    def cost_function(self, u):
        """:156-165.  A Python float for one row (as the reference returns; this reads the device), a tensor [B] for a batch."""
        cost = mpc_cost_grad(self.init_x, self._u(u), want_grad=False)[0]
        return float(cost[0]) if self.single else cost

    def cost_and_gradient(self, u):
        """(cost, d cost / d u) with respect to the normalised controls, in the shape of u; tensors in both forms"""
        cost, grad, _ = mpc_cost_grad(self.init_x, self._u(u))
        return (cost[0], grad[0].reshape(u.shape)) if self.single else (cost, grad.reshape(u.shape))

    def solve(self, u_init=None, iters=200, tol=0.0):
        """minimise over [-1, 1]^(2 horizon) from u_init (zeros, main.py:184) -> (u, cost, pgnorm, info); info: the accepted iterations,
        negative for a row whose line search failed.  Tensors [B, ...]; for one row u is [horizon, 2] and the rest are 0-d tensors."""
        rows = self.init_x.shape[0]
        u0 = torch.zeros(rows, self.horizon, 2, dtype=torch.float32, device=self.init_x.device) if u_init is None else self._u(u_init)
        u, cost, pgnorm, info = mpc_solve(self.init_x, u0, iters, tol)
        return (u[0], cost[0], pgnorm[0], info[0]) if self.single else (u, cost, pgnorm, info)


def mpc_rollout(env, u, steps, horizon, iters=200, tol=0., warm_start=False):
    """mpg_mpc_rollout: `steps` steps of the MPC side of the closed loop - solve from the observation (+ 20 in column 0), step `env` (a
    PathTrackingEnv with num_future_data 0) with the plan's first pair - in ONE launch, bit-identical to the chain of mpc_solve, env.step
    and the torch ops between them.  u [n, horizon, 2]: the start point of the first solve (left as it is).  Advances env._state and
    env.obs (env.done and env.done_intended: the last step's).  Returns (obs_traj [steps, n, 6] - the observations BEFORE each step -,
    plan_traj [steps, n, horizon, 2], rew_traj [steps, n] raw, cost_traj, pgnorm_traj [steps, n], info_traj [steps, n] int32, u_next
    [n, horizon, 2]: the start point of the solve after the last one - with warm_start the last plan moved up by one pair, its last pair
    repeated (main.py:214); without, u)."""
    assert isinstance(env, PathTrackingEnv) and env.num_future_data == 0, 'mpc_rollout: a PathTrackingEnv with num_future_data 0'
    n, dev, steps, horizon = env.num_agent, env.obs.device, int(steps), int(horizon)
    assert u.shape == (n, horizon, 2), (u.shape, n, horizon)
    u_io = u.to(dev, torch.float32).contiguous().clone()
    obs_io = env.obs.contiguous().clone()        # never write into a tensor already handed to the caller
    rows = max(steps, 0)
    obs_traj = torch.empty(rows, n, 6, dtype=torch.float32, device=dev)
    plan_traj = torch.empty(rows, n, horizon, 2, dtype=torch.float32, device=dev)
    rew_traj, cost_traj, pgnorm_traj = (torch.empty(rows, n, dtype=torch.float32, device=dev) for _ in range(3))
    info_traj = torch.empty(rows, n, dtype=torch.int32, device=dev)
    done, done_intended = torch.empty_like(env.done), torch.empty_like(env.done_intended)
    L.call('mpg_mpc_rollout', L.c_int(n), L.c_int(steps), L.c_int(horizon), L.c_int(int(iters)), L.c_float(float(tol)),
           L.c_int(1 if warm_start else 0), L.ptr(env._state), L.ptr(obs_io), L.ptr(u_io), L.ptr(obs_traj), L.ptr(plan_traj), L.ptr(rew_traj),
           L.ptr(cost_traj), L.ptr(pgnorm_traj), L.ptr(info_traj), L.ptr(done), L.ptr(done_intended), L.stream())
    env.obs, env.reward, env.done, env.done_intended = obs_io, rew_traj[-1], done, done_intended
    return obs_traj, plan_traj, rew_traj, cost_traj, pgnorm_traj, info_traj, u_io


def _shifted(plan):
    """main.py:214, concatenate([mpc_action[2:], mpc_action[-2:]]): the plan one step later, its last pair repeated"""
    return torch.cat([plan[:, 1:], plan[:, -1:]], 1)


def run_mpc(policy, num_agent=1, steps=90, horizon=25, seed=0, iters=200, device='cuda', one_launch=False, warm_start=False, tol=0.):
    """The closed loop of mpc/main.py:168-223 for `num_agent` start states at once: two PathTrackingEnv (num_future_data 0) from the same
    start, one driven by the first control pair of a fresh MPC solve per step (from zeros, :184), one by `policy` (PolicyWithQs), and the
    policy's action on the MPC env's observations beside them.

    The solve starts from the MPC env's observation with 20 ADDED to column 0.  main.py:185,221 hands the observation over as it is, and
    its cost reads column 0 as the speed against expected_vs = 20 (:133); that fits the env its recording mpc/mpc_rl.npy was made with,
    whose column 0 was the speed - today's PathTrackingEnv (and this project's) returns v_x - 20, which is why the fixture made from
    that recording subtracts 20 from it ("subtract 20 from obs[0]").  Unshifted, the baseline would drive to 40 m/s.

    warm_start: every solve but the first starts from the plan of the step before, moved up by one pair (:214, commented out there),
    not from zeros.  tol: the solver's stopping tolerance (0: every solve runs all `iters`); the warm start only saves work with one.
    one_launch: the same record, bit for bit, from a launch per chunk of steps instead of a launch per operation: the MPC side as
    mpc_rollout (mpg_mpc_rollout, max(1, MAX_ROLLOUT_WORK // iters) steps per launch), the policy's side as ops.eval_rollout for a
    deterministic policy, and rl_action_mpc from one policy pass over the recorded observations.  The defaults are the loop as it was.
    Measured on one MI355X, 90 steps at horizon 25: at equal settings one launch is at the loop's time for one
    agent and 1 - 2.5 % SLOWER for 256 agents cold (3.20 against 3.17 s: that loop is device-bound, 35 ms of solve per step), and 9 - 11 %
    faster for 256 agents with warm_start and tol = 1e-3 (0.140 against 0.157 s; 14.7 accepted iterations per solve against 137).  The
    warm start changes the closed loop: 12 of those 256 agents end with a reward sum below -20 where one does from zeros (mean -9.3
    against -4.4, median unchanged) - it is the start point, not the tolerance.

    Returns the reference's record keys as stacked device tensors over the steps: mpc_obs, rl_obs [steps, n, 6], mpc_action [steps, n,
    horizon, 2] (the whole plan), rl_action, rl_action_mpc [steps, n, 2], mpc_rew, rl_rew [steps, n] (the reward that led to the recorded
    observation: zeros first).  Nothing in the loop synchronises or copies to the host, so timing is the caller's: synchronise around the
    call."""
    env4mpc = PathTrackingEnv(num_future_data=0, num_agent=num_agent, device=device, seed=seed)
    env4rl = PathTrackingEnv(num_future_data=0, num_agent=num_agent, device=device, seed=seed)
    obs = env4mpc.reset()
    obs4rl = env4rl.reset(init_obs=obs.clone())
    if one_launch:
        return _run_mpc_one_launch(policy, env4mpc, env4rl, int(steps), int(horizon), iters, tol, warm_start)
    shift = torch.zeros(6, dtype=torch.float32, device=obs.device)
    shift[0] = 20.
    mpc = ModelPredictiveControl(obs + shift, horizon)
    rew = torch.zeros(num_agent, dtype=torch.float32, device=obs.device)
    rew4rl = torch.zeros_like(rew)
    keys = ('mpc_obs', 'rl_obs', 'mpc_action', 'rl_action', 'rl_action_mpc', 'mpc_rew', 'rl_rew')
    rec = {k: [] for k in keys}
    u_init = None
    for _ in range(steps):
        mpc_action = mpc.solve(u_init=u_init, iters=iters, tol=tol)[0]
        if warm_start:
            u_init = _shifted(mpc_action)
        rl_action_mpc = policy.compute_action(obs)[0]
        rl_action = policy.compute_action(obs4rl)[0]
        for k, v in zip(keys, (obs, obs4rl, mpc_action, rl_action, rl_action_mpc, rew, rew4rl)):
            rec[k].append(v)
        obs, rew, _, _ = env4mpc.step(mpc_action[:, 0, :].contiguous())
        obs4rl, rew4rl, _, _ = env4rl.step(rl_action)
        mpc.reset_init_x(obs + shift)
    return {k: torch.stack(v) for k, v in rec.items()}


def _run_mpc_one_launch(policy, env4mpc, env4rl, steps, horizon, iters, tol, warm_start):
    """run_mpc's record from both envs behind their resets"""
    from . import ops
    n, dev = env4mpc.num_agent, env4mpc.obs.device
    # the MPC side: chunks of steps, each one launch; state, observation and start point carry over (two calls of s1 and s2 steps are
    # one call of s1 + s2)
    chunk = max(1, MAX_ROLLOUT_WORK // max(int(iters), 1))
    u = torch.zeros(n, horizon, 2, dtype=torch.float32, device=dev)
    parts = []
    for t0 in range(0, steps, chunk):
        out = mpc_rollout(env4mpc, u, min(chunk, steps - t0), horizon, iters, tol, warm_start)
        u = out[6]
        parts.append(out[:3])
    mpc_obs, mpc_action, mpc_rew = (torch.cat([p[k] for p in parts]) for k in range(3))
    zeros = torch.zeros(1, n, dtype=torch.float32, device=dev)
    if policy.deterministic_policy:
        # the policy's side: mpg_eval_rollout is policy_action and env.step per step; rl_action_mpc in ONE pass over all recorded
        # observations - a row's action does not depend on the rows beside it (tests/test_mpc_rollout_gpu.py holds both to the loop's bits)
        state = env4rl._state
        rl_obs, rl_action, rl_rew, last_obs, done, done_intended = ops.eval_rollout(policy.cfg, policy.net('policy'), state, env4rl.obs, steps)
        env4rl.obs, env4rl.reward, env4rl.done, env4rl.done_intended = last_obs, rl_rew[-1], done, done_intended
        rl_action_mpc = policy.compute_action(mpc_obs.reshape(steps * n, 6))[0].reshape(steps, n, 2)
    else:
        # a sampling policy draws from its own stream, twice per step in the loop's order: the same calls in the same order
        obs4rl, rew4rl = env4rl.obs, zeros[0]
        rl_obs, rl_action, rl_action_mpc, rl_rew = [], [], [], []
        for t in range(steps):
            rl_action_mpc.append(policy.compute_action(mpc_obs[t])[0])
            rl_action.append(policy.compute_action(obs4rl)[0])
            rl_obs.append(obs4rl)
            obs4rl, rew4rl, _, _ = env4rl.step(rl_action[-1])
            rl_rew.append(rew4rl)
        rl_obs, rl_action, rl_action_mpc, rl_rew = (torch.stack(v) for v in (rl_obs, rl_action, rl_action_mpc, rl_rew))
    # the reward that LED to the recorded observation: zeros first, the last step's is not recorded
    return dict(mpc_obs=mpc_obs, rl_obs=rl_obs, mpc_action=mpc_action, rl_action=rl_action, rl_action_mpc=rl_action_mpc,
                mpc_rew=torch.cat([zeros, mpc_rew[:-1]]), rl_rew=torch.cat([zeros, rl_rew[:-1]]))


def mpc_rl_summary(rec):
    """What plot_mpc_rl prints of a record (mpc/mpc_ipopt.py:303-311; the two timer lines apart), per agent and for both controllers:
    the root mean squares over the steps of delta_y, delta_v and delta_phi - under the reference's names, which say "mse" - and the
    reward sums.  rec: run_mpc's record; its observations hold v_x - 20 in column 0 already, so nothing is subtracted again (:286 reads a
    recording whose column 0 was the speed).  Returns a dict of [n] float64 tensors."""
    out = {}
    for who in ('mpc', 'rl'):
        obs = rec[who + '_obs'].double()
        for name, col in (('delta_y', 3), ('delta_v', 0), ('delta_phi', 4)):
            out['%s_%s_mse' % (who, name)] = obs[:, :, col].square().mean(0).sqrt()
        out[who + '_rew_sum'] = rec[who + '_rew'].double().sum(0)
    return out


# ---- MPC on the learners' own models (include/mpg_hip.h, "MPC on the learners' OWN models") -----------------------------------------
def _model_rows(name, cfg, obs0, u):
    rows = obs0.shape[0]
    if tuple(obs0.shape) != (rows, cfg.obs_dim) or u.dim() != 3 or (u.shape[0], u.shape[2]) != (rows, cfg.act_dim):
        raise ValueError('%s: obs0 %s and u %s are not [rows, %d] and [rows, horizon, %d]'
                         % (name, tuple(obs0.shape), tuple(u.shape), cfg.obs_dim, cfg.act_dim))
    return rows, u.shape[1]


def model_mpc_cost_grad(cfg, obs0, u, eps=None, want_grad=True, want_traj=False):
    """mpg_model_mpc_cost_grad on the model cfg names: obs0 [B, obs_dim], u [B, H, act_dim] in the policy's tanh range (taken as given),
    eps [H, B] standard-normal model noise (None: the noise terms at their means) -> (cost [B] = - sum of the raw rewards, grad [B, H,
    act_dim] or None, obs_traj [B, H + 1, obs_dim] or None, rew_traj [B, H] or None; the two records come together), one launch"""
    rows, horizon = _model_rows('model_mpc_cost_grad', cfg, obs0, u)
    dev = obs0.device
    eps = ops._model_eps(eps, (horizon, rows), 'model_mpc_cost_grad')
    cost = torch.empty(rows, dtype=torch.float32, device=dev)
    grad = torch.empty(rows, horizon, cfg.act_dim, dtype=torch.float32, device=dev) if want_grad else None
    obs_traj = torch.empty(rows, horizon + 1, cfg.obs_dim, dtype=torch.float32, device=dev) if want_traj else None
    rew_traj = torch.empty(rows, horizon, dtype=torch.float32, device=dev) if want_traj else None
    L.call('mpg_model_mpc_cost_grad', ctypes.byref(cfg), L.c_int(rows), L.c_int(horizon), L.ptr(_f32(obs0)), L.ptr(_f32(u)), L.ptr(eps),
           L.ptr(cost), L.ptr(grad), L.ptr(obs_traj), L.ptr(rew_traj), L.stream())
    return cost, grad, obs_traj, rew_traj


def model_mpc_solve(cfg, obs0, u_init=None, iters=200, tol=0., eps=None, horizon=None):
    """mpg_model_mpc_solve: obs0 [B, obs_dim], u_init [B, H, act_dim] (left as it is; None: zeros, then `horizon` says how many steps) ->
    (u [B, H, act_dim] in the box [-1, 1], cost [B], pgnorm [B], info [B] int32), one launch.  cost <= the cost of the clamped start
    point, for every row."""
    if u_init is None:
        if horizon is None:
            raise ValueError('model_mpc_solve: a start point u_init or a horizon')
        u_init = torch.zeros(obs0.shape[0], int(horizon), cfg.act_dim, dtype=torch.float32, device=obs0.device)
    rows, horizon = _model_rows('model_mpc_solve', cfg, obs0, u_init)
    dev = obs0.device
    eps = ops._model_eps(eps, (horizon, rows), 'model_mpc_solve')
    u = u_init.to(torch.float32).contiguous().clone()
    cost = torch.empty(rows, dtype=torch.float32, device=dev)
    pgnorm = torch.empty(rows, dtype=torch.float32, device=dev)
    info = torch.empty(rows, dtype=torch.int32, device=dev)
    L.call('mpg_model_mpc_solve', ctypes.byref(cfg), L.c_int(rows), L.c_int(horizon), L.c_int(int(iters)), L.c_float(float(tol)),
           L.ptr(_f32(obs0)), L.ptr(eps), L.ptr(u), L.ptr(cost), L.ptr(pgnorm), L.ptr(info), L.stream())
    return u, cost, pgnorm, info


def _model_cfg(env_id_or_cfg):
    return ops.make_cfg(env_id_or_cfg) if isinstance(env_id_or_cfg, str) else env_id_or_cfg


class ModelMPC(object):
    """ModelPredictiveControl's interface on the model the learners optimise through: env_id_or_cfg an env id (the project's default cfg
    of it) or a cfg; init_obs [obs_dim] or [B, obs_dim] START observations on the device, read the way the rollout sweeps read them;
    controls are actions in the policy's tanh range, [horizon, act_dim] (flat accepted) or [B, horizon, act_dim].  eps [horizon, B]: the
    model noise every cost of this object is taken under (None: the noise terms at their means)."""

    def __init__(self, env_id_or_cfg, init_obs, horizon, eps=None):
        self.cfg = _model_cfg(env_id_or_cfg)
        self.horizon = int(horizon)
        self.eps = eps
        self.reset_init_obs(init_obs)

    def reset_init_obs(self, init_obs):
        self.single = init_obs.dim() == 1
        self.init_obs = _f32(init_obs.reshape(-1, self.cfg.obs_dim))

    def _u(self, u):
        return _f32(u.to(self.init_obs.device).reshape(self.init_obs.shape[0], self.horizon, self.cfg.act_dim))

    def cost_function(self, u):
        """A Python float for one row (this reads the device), a tensor [B] for a batch."""
        cost = model_mpc_cost_grad(self.cfg, self.init_obs, self._u(u), self.eps, want_grad=False)[0]
        return float(cost[0]) if self.single else cost

    def cost_and_gradient(self, u):
        """(cost, d cost / d u), the gradient in the shape of u; tensors in both forms"""
        cost, grad = model_mpc_cost_grad(self.cfg, self.init_obs, self._u(u), self.eps)[:2]
        return (cost[0], grad[0].reshape(u.shape)) if self.single else (cost, grad.reshape(u.shape))

    def solve(self, u_init=None, iters=200, tol=0.0):
        """minimise over the box from u_init (None: zeros) -> (u, cost, pgnorm, info); info: the accepted iterations, negative for a row
        whose line search failed.  Tensors [B, ...]; for one row u is [horizon, act_dim] and the rest are 0-d tensors."""
        u0 = None if u_init is None else self._u(u_init)
        u, cost, pgnorm, info = model_mpc_solve(self.cfg, self.init_obs, u0, iters, tol, self.eps, horizon=self.horizon)
        return (u[0], cost[0], pgnorm[0], info[0]) if self.single else (u, cost, pgnorm, info)


def model_mpc_rollout(cfg, obs, u, steps, iters=200, tol=0., warm_start=False, eps=None):
    """mpg_model_mpc_rollout: `steps` steps of MPC's closed loop ON THE MODEL cfg names - solve from the row at the noise means, step the
    plant with the plan's first action under eps - in ONE launch, bit-identical to the chain of model_mpc_solve (eps None), _shifted and
    model_mpc_cost_grad at horizon 1 (include/mpg_hip.h writes it out).  obs [n, obs_dim] the start rows, u [n, horizon, act_dim] the
    start point of the first solve, eps [steps, n] the PLANT's standard-normal model noise (None: zeros; the planner never sees it).
    Nothing handed in is written.  Returns (obs_traj [steps, n, obs_dim] - the rows BEFORE each step -, plan_traj [steps, n, horizon,
    act_dim], rew_traj [steps, n] raw, cost_traj, pgnorm_traj [steps, n], info_traj [steps, n] int32, last_obs [n, obs_dim], u_next
    [n, horizon, act_dim]: the start point of the solve after the last one - with warm_start the last plan moved up by one action, its
    last action repeated; without, u)."""
    n, horizon = _model_rows('model_mpc_rollout', cfg, obs, u)
    dev, steps = obs.device, int(steps)
    eps = ops._model_eps(eps, (steps, n), 'model_mpc_rollout')
    obs_io = obs.to(torch.float32).contiguous().clone()          # never write into a tensor the caller handed in
    u_io = u.to(dev, torch.float32).contiguous().clone()
    rows = max(steps, 0)
    obs_traj = torch.empty(rows, n, cfg.obs_dim, dtype=torch.float32, device=dev)
    plan_traj = torch.empty(rows, n, horizon, cfg.act_dim, dtype=torch.float32, device=dev)
    rew_traj, cost_traj, pgnorm_traj = (torch.empty(rows, n, dtype=torch.float32, device=dev) for _ in range(3))
    info_traj = torch.empty(rows, n, dtype=torch.int32, device=dev)
    L.call('mpg_model_mpc_rollout', ctypes.byref(cfg), L.c_int(n), L.c_int(steps), L.c_int(horizon), L.c_int(int(iters)), L.c_float(float(tol)),
           L.c_int(1 if warm_start else 0), L.ptr(obs_io), L.ptr(u_io), L.ptr(eps), L.ptr(obs_traj), L.ptr(plan_traj), L.ptr(rew_traj),
           L.ptr(cost_traj), L.ptr(pgnorm_traj), L.ptr(info_traj), L.stream())
    return obs_traj, plan_traj, rew_traj, cost_traj, pgnorm_traj, info_traj, obs_io, u_io


def model_rollout_chunk(steps, iters, work_cap, max_steps=MODEL_MAX_ROLLOUT_STEPS):
    """the steps of one mpg_model_mpc_rollout launch of a loop of `steps` steps with `iters` iterations per solve: as many as the work
    cap allows (steps * iters <= work_cap; no iterations are no work), at least one, at most max_steps and the loop's own length"""
    steps, iters, work_cap, max_steps = int(steps), int(iters), int(work_cap), int(max_steps)
    fit = work_cap // iters if iters > 0 else max_steps
    return max(1, min(fit, max_steps, steps))


def _run_model_mpc_one_launch(cfg, obs, steps, horizon, iters, tol, warm_start, eps, work_cap=None):
    """run_model_mpc's record from chunks of model_mpc_rollout: the row, the start point and the eps slice carry over (two calls of s1 and
    s2 steps are one call of s1 + s2).  work_cap None: the kind's MODEL_MAX_ROLLOUT_WORK."""
    n, dev = obs.shape[0], obs.device
    chunk = model_rollout_chunk(steps, iters, MODEL_MAX_ROLLOUT_WORK[int(cfg.env_kind)] if work_cap is None else work_cap)
    u = torch.zeros(n, int(horizon), cfg.act_dim, dtype=torch.float32, device=dev)
    parts = []
    for t0 in range(0, steps, chunk):
        s = min(chunk, steps - t0)
        out = model_mpc_rollout(cfg, obs, u, s, iters, tol, warm_start, None if eps is None else eps[t0:t0 + s])
        obs, u = out[6], out[7]
        parts.append(out[:6])
    obs_traj, plan, rew, cost, pgnorm, info = (torch.cat([p[k] for p in parts]) for k in range(6))
    return dict(obs_traj=obs_traj, act_traj=plan[:, :, 0, :].contiguous(), rew_traj=rew, cost=cost, pgnorm=pgnorm, info=info, last_obs=obs)


def run_model_mpc(env_id_or_cfg, init_obs, steps, horizon, iters=200, tol=0., warm_start=False, one_launch=False, eps=None):
    """The receding-horizon closed loop ON THE MODEL from init_obs [n, obs_dim]: per step one solve from the current observation
    (model_mpc_solve, noise terms at their means) and one ops.model_step with the plan's first action - a Python loop of two launches per
    step.  warm_start: every solve but the first starts from the plan of the step before moved up by one action, its last one repeated;
    otherwise from zeros.  eps [steps, n]: the PLANT's standard-normal model noise (None: zeros), eps[t] handed to step t; the planner
    plans at the noise means either way - the setting the learners' rollouts see.
    one_launch: the same dict from model_mpc_rollout (mpg_model_mpc_rollout), one launch per chunk of model_rollout_chunk(steps, iters,
    the kind's MODEL_MAX_ROLLOUT_WORK) steps.  The two forms' STEPS differ: the loop's is mpg_model_step, compiled with contraction in
    the rollouts' unit; the launch's is the one-step horizon cost of the solver's unit, compiled without (one kernel cannot hold both
    forms of the model bodies).  They are the same model step in the same row format, equal in exact arithmetic and different by
    rounding, so the first step's obs_traj, act_traj, cost, pgnorm and info are the loop's bit for bit and everything behind it agrees
    to rounding as far as the closed loop keeps rounding small.  The default is the loop as it was.
    Returns a dict: mpg_model_rollout's record - obs_traj [steps, n, obs_dim] (the observations BEFORE each step),
    act_traj [steps, n, act_dim], rew_traj [steps, n] RAW, last_obs [n, obs_dim], as ops.eval_metrics and ModelEvaluator's metric code
    read it - plus cost, pgnorm [steps, n] and info [steps, n] int32 of every step's solve."""
    cfg = _model_cfg(env_id_or_cfg)
    obs = _f32(init_obs)
    steps = int(steps)
    if steps < 1:
        raise ValueError('run_model_mpc: steps >= 1 (got %d)' % steps)
    eps = ops._model_eps(eps, (steps, obs.shape[0]), 'run_model_mpc')
    if one_launch:
        return _run_model_mpc_one_launch(cfg, obs, steps, horizon, iters, tol, warm_start, eps)
    keys = ('obs_traj', 'act_traj', 'rew_traj', 'cost', 'pgnorm', 'info')
    rec = {k: [] for k in keys}
    u_init = None
    for t in range(steps):
        plan, cost, pgnorm, info = model_mpc_solve(cfg, obs, u_init, iters, tol, horizon=horizon)
        if warm_start:
            u_init = _shifted(plan)
        act = plan[:, 0, :].contiguous()
        nxt, rew = ops.model_step(cfg, obs, act, None if eps is None else eps[t])
        for k, v in zip(keys, (obs, act, rew, cost, pgnorm, info)):
            rec[k].append(v)
        obs = nxt
    out = {k: torch.stack(v) for k, v in rec.items()}
    out['last_obs'] = obs
    return out
