"""Device-resident vectorised environments - mirrors of PathTrackingEnv
(envs_and_models/path_tracking_env.py:356-487) and of the vectorised InvertedPendulumContiEnv
(envs_and_models/inverted_pendulum_conti.py:5-30 behind utils/dummy_vec_env.py): same method names, argument meaning
and quirks (PathTracking's done is always True); arrays are torch tensors on the GPU instead of numpy.
InvertedDoublePendulum-v2 has no real env here (MuJoCo); InvertedDoublePendulumModelEnv makes the reference authors' differentiable
model of it an env (make_model_env) - make_env keeps refusing that id."""
import ctypes

import torch

from . import _lib as L

ENV_KIND = {'PathTracking-v0': 0, 'InvertedPendulumConti-v0': 1, 'InvertedDoublePendulum-v2': 2}     # MPG_ENV_* (include/mpg_hip.h)


class _DeviceVecEnv(object):
    """gym-style vector env: `num_agent` agents stepped by ONE HIP launch (mpg_env_step)."""
    kind, obs_dim, act_dim = 0, 6, 2

    def __init__(self, num_agent=1, device='cuda', seed=0):
        self.num_agent = num_agent
        self.device = torch.device(device)
        self.seed, self._ctr = int(seed), 0
        n = num_agent
        self._state = torch.zeros(8, n, dtype=torch.float32, device=self.device)       # MPG_ENV_STATE_DIM rows, opaque
        self.obs = torch.zeros(n, self.obs_dim, dtype=torch.float32, device=self.device)
        self.reward = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.done = torch.ones(n, dtype=torch.uint8, device=self.device)
        self.done_intended = torch.zeros(n, dtype=torch.uint8, device=self.device)
        self._initialised = False

    def reset(self, **kwargs):
        """reset(init_obs=obs) rebuilds the state from obs (path_tracking_env.py:411-421); reset() re-draws agents with
        done==1 (:423-454) - every agent on the first call."""
        if 'init_obs' in kwargs:
            init_obs = kwargs['init_obs'].to(self.device, torch.float32).contiguous()
            assert init_obs.shape == (self.num_agent, self.obs_dim), (init_obs.shape, self.obs_dim)
            L.call('mpg_env_reset_from_obs', L.c_int(self.kind), L.c_int(self.num_agent), L.c_int(self.obs_dim),
                   L.ptr(self._state), L.ptr(init_obs), L.stream())
            self.obs = init_obs
            self._initialised = True
            return self.obs
        mask = self.done if self._initialised else None
        obs = torch.empty_like(self.obs)        # never write into a tensor already handed to the caller
        L.call('mpg_env_reset', L.c_int(self.kind), L.c_int(self.num_agent), L.c_int(self.obs_dim), L.ptr(self._state),
               L.ptr(mask), L.c_u64(self.seed), L.c_u64(self._ctr), L.ptr(obs), L.stream())
        self._ctr += 1
        self._initialised = True
        self.obs = obs
        return self.obs

    def step(self, action):
        """action [num_agent, act_dim] -> (obs, reward, done, info)."""
        if not (action.dtype == torch.float32 and action.device == self.device and action.is_contiguous()):
            action = action.to(self.device, torch.float32).contiguous()
        assert action.shape == (self.num_agent, self.act_dim)
        obs = torch.empty_like(self.obs)
        reward = torch.empty_like(self.reward)
        done = torch.empty_like(self.done)      # fresh outputs: callers keep them (replay batches)
        L.call('mpg_env_step', L.c_int(self.kind), L.c_int(self.num_agent), L.c_int(self.obs_dim), L.ptr(self._state),
               L.ptr(action), L.ptr(obs), L.ptr(reward), L.ptr(done), L.ptr(self.done_intended), L.stream())
        self.obs, self.reward, self.done = obs, reward, done
        return self.obs, self.reward, self.done, {}


class PathTrackingEnv(_DeviceVecEnv):
    """PathTrackingEnv(num_future_data, num_agent) - path_tracking_env.py:356-487.  Observations have 6 + num_future_data
    entries: the six base entries and the look-ahead delta-y terms of :385-402.  The env, worker, learner and evaluator
    serve 0 <= num_future_data <= 10 (policy inputs up to 16 wide, critic inputs up to 18: the 16- and 24-wide network kernels; the
    shipped parser default is 0, train_script.py:90; with look-ahead entries the learner takes the launch-per-stage path, the
    fused kernels are built for the base widths)."""
    kind, act_dim = 0, 2
    MAX_FUTURE = 10                            # MPG_ENV_MAX_FUTURE

    def __init__(self, num_future_data=0, num_agent=1, device='cuda', seed=0, **kwargs):
        assert 0 <= int(num_future_data) <= self.MAX_FUTURE, 'num_future_data in [0, %d]' % self.MAX_FUTURE
        self.num_future_data = int(num_future_data)
        self.obs_dim = 6 + self.num_future_data
        super().__init__(num_agent, device, seed)

    # veh_full_state / veh_state views in the reference's column order (for tests and evaluators)
    @property
    def veh_full_state(self):
        return self._state[:6].t().contiguous()

    @property
    def veh_state(self):
        s = self._state
        return torch.stack([s[0], s[1], s[2], s[6], s[7], s[5]], 1)


class InvertedPendulumContiEnv(_DeviceVecEnv):
    """The pendulum's REAL environment (the reference: MuJoCo behind DummyVecEnv, inverted_pendulum_conti.py:5-30) as an
    analytic RK4 cart-pole kernel (csrc/env_cart_pole.hip).  Parity with MuJoCo is unpinned (it cannot be installed here);
    the kernel is tested against the float64 restatement of the same equations in oracle/."""
    kind, obs_dim, act_dim = 1, 4, 1

    def __init__(self, num_agent=1, device='cuda', seed=0, **kwargs):
        super().__init__(num_agent, device, seed)


class InvertedDoublePendulumModelEnv(_DeviceVecEnv):
    """InvertedDoublePendulum-v2 on the reference authors' MODEL of it (inverted_double_pendulum_model.py; mpg_model_env_*,
    include/mpg_hip.h): step() is mpg_model_step's row step, done = the model's tip height <= 1 or `max_episode_steps` steps (gym's
    registered limit for this id is 1000; 0: none), reset() re-draws the done agents from a law of the shape of gym's reset_model.
    The env is stateless in the observation: `_state` is the per-agent step count (int32 [num_agent]).  Beside the dynamics it differs
    from MuJoCo's env in that theta2 is an absolute angle and nothing bounds the cart position."""
    kind, obs_dim, act_dim = 2, 11, 1

    def __init__(self, num_agent=1, device='cuda', seed=0, max_episode_steps=1000, **kwargs):
        super().__init__(num_agent, device, seed)
        if int(max_episode_steps) < 0:
            raise ValueError('max_episode_steps >= 0, 0 for no episode limit (got %r)' % (max_episode_steps,))
        self.max_episode_steps = int(max_episode_steps)
        self._state = torch.zeros(num_agent, dtype=torch.int32, device=self.device)
        from .ops import make_cfg
        self.cfg = make_cfg('InvertedDoublePendulum-v2')       # (the env entry points read the kind and the widths of it, nothing else)

    def reset(self, **kwargs):
        """reset(init_obs=obs) takes obs as the agents' rows and zeroes their step counts; reset() re-draws agents with done==1 - every
        agent on the first call."""
        if 'init_obs' in kwargs:
            init_obs = kwargs['init_obs'].to(self.device, torch.float32).contiguous()
            assert init_obs.shape == (self.num_agent, self.obs_dim), (init_obs.shape, self.obs_dim)
            self._state.zero_()
            self.obs = init_obs
            self._initialised = True
            return self.obs
        mask = self.done if self._initialised else None
        obs = self.obs.clone()                  # never write into a tensor already handed to the caller
        L.call('mpg_model_env_reset', ctypes.byref(self.cfg), L.c_int(self.num_agent), L.ptr(obs), L.ptr(self._state), L.ptr(mask),
               L.c_u64(self.seed), L.c_u64(self._ctr), L.stream())
        self._ctr += 1
        self._initialised = True
        self.obs = obs
        return self.obs

    def step(self, action):
        """action [num_agent, 1] -> (obs, RAW reward, done, info)."""
        if not (action.dtype == torch.float32 and action.device == self.device and action.is_contiguous()):
            action = action.to(self.device, torch.float32).contiguous()
        assert action.shape == (self.num_agent, self.act_dim)
        obs = torch.empty_like(self.obs)
        reward = torch.empty_like(self.reward)
        done = torch.empty_like(self.done)      # fresh outputs: callers keep them (replay batches)
        L.call('mpg_model_env_step', ctypes.byref(self.cfg), L.c_int(self.num_agent), L.ptr(self.obs), L.ptr(action),
               L.c_int(self.max_episode_steps), L.ptr(self._state), L.ptr(obs), L.ptr(reward), L.ptr(done), L.stream())
        self.obs, self.reward, self.done = obs, reward, done
        return self.obs, self.reward, self.done, {}


def make_model_env(env_id, num_agent=1, device='cuda', seed=0, max_episode_steps=1000):
    """the env of `env_id` on its differentiable MODEL, for the one id whose real env is not provided (args.env_on_model of
    OffPolicyWorker); the other two ids have real envs: make_env"""
    if env_id == 'InvertedDoublePendulum-v2':
        return InvertedDoublePendulumModelEnv(num_agent=num_agent, device=device, seed=seed, max_episode_steps=max_episode_steps)
    raise ValueError('no model-backed environment for %r: it is built for InvertedDoublePendulum-v2 only (PathTracking-v0 and '
                     'InvertedPendulumConti-v0 have real envs: make_env)' % (env_id,))


def make_env(env_id, num_agent=1, num_future_data=0, device='cuda', seed=0):
    """gym.make(env_id, ...) of the reference's worker / evaluator (worker.py:40-44, evaluator.py:33-36) for the two
    environments of the hot path."""
    if env_id == 'PathTracking-v0':
        return PathTrackingEnv(num_future_data=num_future_data, num_agent=num_agent, device=device, seed=seed)
    if env_id == 'InvertedPendulumConti-v0':
        return InvertedPendulumContiEnv(num_agent=num_agent, device=device, seed=seed)
    if env_id == 'InvertedDoublePendulum-v2':
        # only the differentiable MODEL of this env exists here (the rollout sweeps, NADPLearner): the real env is gym's MuJoCo
        # InvertedDoublePendulum-v2, which is not provided, so there is nothing for a worker or an evaluator to step
        raise ValueError('no device environment for %r: the real env is MuJoCo and not provided; only its differentiable model '
                         'is (model rollouts, NADPLearner)' % (env_id,))
    raise ValueError('no device environment for %r (PathTracking-v0, InvertedPendulumConti-v0)' % (env_id,))
