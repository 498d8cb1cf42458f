"""The model step and the policy's closed loop on the model - what mpg_model_step and mpg_model_rollout compute - restated from the
oracles of the three differentiable models (oracle.mpg_oracle: PathTrackingModelOracle, InvertedPendulumModelOracle, Nets.compute_action,
process_obses; tests/dp_oracle.py: DoublePendulumModelOracle), in float32 or float64.  A plain helper module shared by
tests/test_model_rollout.py (CPU) and tests/test_model_rollout_gpu.py; mpg_amd never imports it.

Every step takes its observation the way the reference's closed loop does (inverted_double_pendulum_model.py:245-265): model.reset(obs),
then rollout_out - so PathTracking reads the six base entries unwrapped, and the double pendulum's state is the atan2 of the row's sines
and cosines at EVERY step, as in the chain of mpg_model_step calls."""
import functools

import numpy as np
import torch

from oracle import mpg_oracle as O
from tests import dp_oracle as DP
from tests import model_edge_inputs as E
from tests.golden_inputs import mlp_weights_flat

PT, PD, DPEND = 'PathTracking-v0', 'InvertedPendulumConti-v0', DP.ENV_ID
FIXTURES = {PT: 'model_rollout_ref.npz', PD: 'pendulum_model_ref.npz', DPEND: 'double_pendulum_model_ref.npz'}
VARIANTS = {'no clamp': dict(clamp='none'), 'no wrap': dict(wrap=False)}       # PathTracking steps that miss a branch


def ocfg_of(env_id, K=0):
    """the oracle's Cfg of an env id under the project's defaults (K look-ahead entries on PathTracking)"""
    if env_id == PT:
        return O.Cfg(obs_dim=6 + K, obs_scale=list(O.OBS_SCALE_PT) + [1.] * K)
    return O.Cfg(env=PD) if env_id == PD else DP.make_cfg()


def model_of(ocfg, variant=None):
    if ocfg.env == PT:
        return E.EdgePathTrackingModel(ocfg.obs_dim - 6, **VARIANTS[variant]) if variant else O.PathTrackingModelOracle(ocfg.obs_dim - 6)
    assert variant is None
    return O.InvertedPendulumModelOracle() if ocfg.env == PD else DP.DoublePendulumModelOracle()


def _t(x, dtype):
    return torch.as_tensor(np.asarray(x)).to(dtype)


def step(ocfg, obs, act, eps=None, dtype=torch.float64, variant=None):
    """one rollout_out from the observation rows obs [rows, obs_dim]: (obs_next [rows, obs_dim], rew [rows] RAW), numpy in `dtype`;
    eps None: the noise terms at their means"""
    m = model_of(ocfg, variant)
    obs = _t(obs, dtype)
    m.reset(obs)
    e = torch.zeros(obs.shape[0], dtype=dtype) if eps is None else _t(eps, dtype)
    o, r = m.rollout_out(_t(act, dtype), e)
    return o.detach().numpy(), r.detach().numpy()


def nets_of(ocfg, wp, dtype):
    return O.Nets(ocfg, {'policy': wp}, dtype=dtype)


def closed_loop(ocfg, wp, obs0, steps, eps=None, dtype=torch.float64, actions=None, variant=None):
    """`steps` times: the policy's action on the processed observation (or actions[t], teacher-forced), then step().  Returns
    (obs_traj [steps, n, obs_dim] - the observations BEFORE each step -, act_traj [steps, n, act_dim], rew_traj [steps, n], last_obs),
    numpy in `dtype`."""
    nets = nets_of(ocfg, wp, dtype) if actions is None else None
    obs = np.asarray(obs0).astype(np.float64 if dtype == torch.float64 else np.float32)
    obs_l, act_l, rew_l = [], [], []
    for t in range(steps):
        if actions is None:
            with torch.no_grad():
                act = nets.compute_action(O.process_obses(ocfg, _t(obs, dtype))).numpy()
        else:
            act = np.asarray(actions[t])
        obs_l.append(obs), act_l.append(act)
        obs, rew = step(ocfg, obs, act, None if eps is None else eps[t], dtype, variant)
        rew_l.append(rew)
    return np.stack(obs_l), np.stack(act_l), np.stack(rew_l), obs


def teacher_forced(g, ocfg, dtype, step_fn=None):
    """the fixture g's chain one step at a time from ITS float32 observations: obs[t - 1] (obs0 at t = 0), actions[t], eps[t] ->
    (obs [25, 64, obs_dim], reward [25, 64]); step_fn(obs, act, eps) stands for the oracle's step (the device's in the GPU test)"""
    step_fn = step_fn or (lambda o, a, e: step(ocfg, o, a, e, dtype))
    obs_l, rew_l = [], []
    for t in range(g['actions'].shape[0]):
        o, r = step_fn(g['obs0'] if t == 0 else g['obs'][t - 1], g['actions'][t], g['eps'][t] if 'eps' in g else None)
        obs_l.append(o), rew_l.append(r)
    return np.stack(obs_l), np.stack(rew_l)


def free_running(g, ocfg, dtype, step_fn=None):
    """the same chain from obs0 on the chain's OWN observations"""
    step_fn = step_fn or (lambda o, a, e: step(ocfg, o, a, e, dtype))
    obs, obs_l, rew_l = g['obs0'], [], []
    for t in range(g['actions'].shape[0]):
        obs, r = step_fn(obs, g['actions'][t], g['eps'][t] if 'eps' in g else None)
        obs_l.append(obs), rew_l.append(r)
    return np.stack(obs_l), np.stack(rew_l)


# ---- the cases both test files run ------------------------------------------------------------------------------------------------
EDGE_STEP_CASES = [(PT, 0, 48), (PT, 3, 17), (PD, 0, 48), (PD, 0, 17)]       # (env, look-ahead K, rows)
FAR_ACC = 7.                # |acceleration action| of the clamp blocks: 2.1 m/s per step, beyond the policy's range - the model takes it
LOOP_CASES = [(PT, 0), (PT, 3), (PD, 0), (DPEND, 0)]                          # (env, look-ahead K): 48 trajectories x 25 steps
LOOP_ROWS, LOOP_STEPS = 48, 25


@functools.lru_cache(maxsize=None)
def edge_step_case(env_id, K, rows):
    """(ocfg, obs [rows, obs_dim], act, eps [rows]) of a single step at the models' edges.  PathTracking: E.edge_obs, steering
    U(-1.2, 1.2), acceleration +FAR_ACC on the block below the upper clamp and -FAR_ACC on the block above the lower one (one step
    moves v_x by 0.3 * action: every row of the two blocks is clamped), U(-1.2, 1.2) elsewhere.  Pendulum: E.pendulum_wide_obs with
    every fourth angle moved to within 0.04 rad inside +-pi and a velocity of 3 .. 6 rad/s outwards: one step takes it beyond."""
    rng = np.random.Generator(np.random.PCG64(700 + 10 * K + rows))
    ocfg = ocfg_of(env_id, K)
    if env_id == PT:
        obs = E.edge_obs(rng, rows, K)
        act = rng.uniform(-1.2, 1.2, (rows, 2)).astype(np.float32)
        q = rows // 4
        act[:q, 1], act[q:2 * q, 1] = FAR_ACC, -FAR_ACC
    else:
        obs = E.pendulum_wide_obs(rng, rows)
        sign = np.where(np.arange(rows) % 8 < 4, 1., -1.)[::4]
        obs[::4, 1] = (sign * (np.pi - rng.uniform(0.005, 0.04, sign.size))).astype(np.float32)
        obs[::4, 3] = (sign * rng.uniform(3., 6., sign.size)).astype(np.float32)
        act = rng.uniform(-1., 1., (rows, 1)).astype(np.float32)
    return ocfg, obs, act, rng.standard_normal(rows).astype(np.float32)


@functools.lru_cache(maxsize=None)
def edge_step_reference(env_id, K, rows, f64=True):
    ocfg, obs, act, eps = edge_step_case(env_id, K, rows)
    return step(ocfg, obs, act, eps, torch.float64 if f64 else torch.float32)


@functools.lru_cache(maxsize=None)
def loop_case(env_id, K=0):
    """(ocfg, policy weights, obs0 [48, obs_dim], eps [25, 48]) of a closed loop.  PathTracking and the pendulum: the inputs of the
    sweeps' edge cases (tests/model_edge_inputs.py: their seeds keep every raw value 1e-3 away from a threshold along exactly this
    closed loop).  Double pendulum: the start law of its fixtures; eps is there for the interface and not read."""
    if env_id != DPEND:
        env = E.PT if env_id == PT else E.PD
        ocfg, wp, _, obs, eps = E.inputs(env, LOOP_ROWS, 1, LOOP_STEPS, K, E.seed_of(env, LOOP_ROWS, 1, LOOP_STEPS, K))
        return ocfg, wp, obs, eps
    rng = np.random.Generator(np.random.PCG64(1))
    wp = mlp_weights_flat(rng, 11, 2)
    return DP.make_cfg(), wp, DP.start_obs(rng, LOOP_ROWS), rng.standard_normal((LOOP_STEPS, LOOP_ROWS)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def loop_reference(env_id, K=0, f64=True):
    ocfg, wp, obs, eps = loop_case(env_id, K)
    return closed_loop(ocfg, wp, obs, LOOP_STEPS, eps, torch.float64 if f64 else torch.float32)


def processed_return_sum(ocfg, rew_traj):
    """sum over rows and steps of the processed rewards (rew + rew_shift) * rew_scale, float64: mpg_ampc_pg's ret_sum"""
    return float(((np.asarray(rew_traj, np.float64) + ocfg.rew_shift) * ocfg.rew_scale).sum())
