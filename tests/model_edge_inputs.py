"""Start states that drive the rollout sweeps through the branches of the differentiable models, and the oracle variants that say
what a wrong branch would cost.  Shared by tests/test_model_edges.py (CPU: the conditions that make the device test worth running)
and tests/test_model_edges_gpu.py (the kernels against float64 autograd on these inputs).  A plain helper module.

PathTracking (mpg_amd/csrc/rollout_common.h): finish() clamps the new v_x to [1, 35], pre() wraps the new heading error into
(-pi, pi], vjp() zeroes the adjoint of v_x where the raw value left [1, 35].  One model step moves v_x by at most 0.3 and the reset
law starts it in [15, 25] with a heading error of N(0, pi / 9), so inputs drawn from that law alone reach none of the three.
The pendulum model has no branch; its start states here cover the whole circle instead of +-0.1 rad around upright."""
import functools

import numpy as np
import torch

from oracle import mpg_oracle as O
from tests import ampc_oracle as A
from tests.golden_inputs import mlp_weights_flat, reset_law_obs

PT, PD = 'pt', 'pd'
PD_ENV = 'InvertedPendulumConti-v0'
STEP0, ALL = False, True
H = 256
VARIANTS = ('no clamp', 'no wrap', 'ungated adjoint')


# ---- models ------------------------------------------------------------------------------------------------------------------
class EdgePathTrackingModel(O.PathTrackingModelOracle):
    """PathTrackingModelOracle.rollout_out restated with its two branches switchable, and a log of what enters them:
      clamp = 'true'      torch.clamp(v_x, 1, 35), as the reference (path_tracking_env.py:289);
              'none'      the raw v_x goes on;
              'straight'  the clamped VALUE with the adjoint of the raw one, x + (clamp(x) - x).detach(): a reverse sweep that
                          does not gate the adjoint of v_x;
      wrap = False        the heading error is not brought back into (-pi, pi] (:290-291).
    log: a list that receives (raw v_x [R], raw heading error [R]) of every step, before the clamp and the wrap."""

    def __init__(self, num_future_data=0, clamp='true', wrap=True, log=None):
        super().__init__(num_future_data)
        assert clamp in ('true', 'none', 'straight')
        self.clamp, self.wrap, self.log = clamp, wrap, log

    def rollout_out(self, actions, eps):
        dt = self.veh_states.dtype
        actions = torch.stack([actions[:, 0] * 1.2 * np.pi / 9, actions[:, 1] * 3.], 1)
        rewards = O.compute_rewards_pt(self.veh_states, actions)
        noise = 0.5 * torch.ones_like(eps) + 0.01 * eps
        vs, _ = O.f_xu(self.veh_states, actions, 1 / 10., noise=noise.to(dt))
        raw_vx, raw_dphi = vs[:, 0], vs[:, 4]
        if self.log is not None:
            self.log.append((raw_vx.detach().numpy().astype(np.float64), raw_dphi.detach().numpy().astype(np.float64)))
        if self.clamp == 'true':
            v_xs = torch.clamp(raw_vx, 1, 35)
        elif self.clamp == 'straight':
            v_xs = raw_vx + (torch.clamp(raw_vx, 1, 35) - raw_vx).detach()
        else:
            v_xs = raw_vx
        dphi = raw_dphi
        if self.wrap:
            dphi = torch.where(dphi > np.pi, dphi - 2 * np.pi, dphi)
            dphi = torch.where(dphi <= -np.pi, dphi + 2 * np.pi, dphi)
        self.veh_states = torch.stack([v_xs, vs[:, 1], vs[:, 2], vs[:, 3], dphi, vs[:, 5]], 1)
        obses = torch.stack([v_xs - O.EXPECTED_VS] + [self.veh_states[:, i] for i in range(1, 6)] +
                            [self.veh_states[:, 3] for _ in range(self.num_future_data)], 1)
        return obses, rewards


class LoggingPendulumModel(O.InvertedPendulumModelOracle):
    """the pendulum model with a log of the angle every step is taken FROM (what the kernel's sincosf sees)"""

    def __init__(self, log):
        self.log = log

    def rollout_out(self, actions, eps):
        self.log.append(self.obses[:, 1].detach().numpy().astype(np.float64))
        return super().rollout_out(actions, eps)


def model_of(ocfg, variant=None, log=None):
    """the model of a case: the true one (variant None) or one of VARIANTS; PathTracking only for a variant"""
    if ocfg.env == PD_ENV:
        assert variant is None
        return LoggingPendulumModel(log) if log is not None else None
    kw = {None: {}, 'no clamp': dict(clamp='none'), 'no wrap': dict(wrap=False), 'ungated adjoint': dict(clamp='straight')}[variant]
    return EdgePathTrackingModel(ocfg.obs_dim - 6, log=log, **kw)


# ---- start states ------------------------------------------------------------------------------------------------------------
def edge_obs(rng, rows, K=0):
    """Start observations [rows][6 + K]: a reset-law draw with three quarter-blocks overwritten and two more rows after them.
      block 0  v_x - 20 ~ U(13.0, 14.9): the upper clamp is one to seven steps of full throttle away;
      block 1  v_x - 20 ~ U(-18.9, -17.5), v_y scaled by 0.1 (the law draws it proportional to v_x): the lower clamp;
      block 2  heading error +-U(2.9, 3.13), signs alternating, with a yaw rate of that sign and U(0.3, 1.0) in size, so that
               half of the block runs up into the wrap at +pi and half down into the one at -pi;
      then two rows OUTSIDE the principal range, heading error +U(3.3, 3.5) and -U(3.3, 3.5): the reference does not wrap a start
               observation, so the kernel's sine and cosine meet |x| > pi there (and the first step wraps them).
    The last quarter (minus those two rows) stays as the law drew it.  Look-ahead entries as tests/test_slices_gpu.inputs forms
    them: near delta_y, not equal to it."""
    obs = reset_law_obs(rng, rows)
    q = rows // 4
    assert q >= 2 and rows >= 3 * q + 2
    obs[:q, 0] = rng.uniform(13.0, 14.9, q)
    obs[q:2 * q, 0] = rng.uniform(-18.9, -17.5, q)
    obs[q:2 * q, 1] *= np.float32(0.1)
    sign = np.where(np.arange(q) % 2 == 0, 1., -1.)
    obs[2 * q:3 * q, 4] = sign * rng.uniform(2.9, 3.13, q)
    obs[2 * q:3 * q, 2] = sign * rng.uniform(0.3, 1.0, q)
    obs[3 * q:3 * q + 2, 4] = np.array([1., -1.]) * rng.uniform(3.3, 3.5, 2)
    if K:
        obs = np.concatenate([obs, obs[:, 3:4] + 0.3 * rng.standard_normal((rows, K)).astype(np.float32)], 1)
    return np.ascontiguousarray(obs, np.float32)


def pendulum_wide_obs(rng, rows):
    """[p, theta, pdot, thetadot]: p and pdot ~ U(-1, 1), theta ~ U(-pi, pi), thetadot ~ U(-3, 3)"""
    return np.stack([rng.uniform(-1, 1, rows), rng.uniform(-np.pi, np.pi, rows), rng.uniform(-1, 1, rows),
                     rng.uniform(-3, 3, rows)], 1).astype(np.float32)


PHILOX = (4242, (3 << 32) + 17)         # (noise_seed, noise_ctr) of the case that draws its noise in the kernel


@functools.lru_cache(maxsize=None)
def inputs(env, rows, M, n, K, seed, philox=False):
    """(ocfg, policy weights, Q1 weights, start observations, eps [n][rows * M]); draw order: policy, Q1, observations, eps.
    Computed once per set of arguments and shared: nothing in it is written to later.
    philox: eps is what the sweeps draw themselves for PHILOX (O.model_noise_philox) instead of a PCG64 draw."""
    rng = np.random.Generator(np.random.PCG64(seed))
    if env == PT:
        ocfg = O.Cfg(M=M, n=n, obs_dim=6 + K, obs_scale=list(O.OBS_SCALE_PT) + [1.] * K)
        wp, wq = mlp_weights_flat(rng, 6 + K, 4), mlp_weights_flat(rng, 8 + K, 1)
        obs = edge_obs(rng, rows, K)
    else:
        ocfg = O.Cfg(env=PD_ENV, M=M, n=n)
        wp, wq = mlp_weights_flat(rng, 4, 2), mlp_weights_flat(rng, 5, 1)
        obs = pendulum_wide_obs(rng, rows)
    eps = O.model_noise_philox(n, rows * M, *PHILOX) if philox else rng.standard_normal((n, rows * M)).astype(np.float32)
    return ocfg, wp, wq, obs, eps


@functools.lru_cache(maxsize=None)
def extras(rows, seed):
    """what the entry points with a replay batch need beside inputs(): first actions U(-1.2, 1.2), a second critic, raw rewards and
    next observations (a stream of its own, so that inputs() stays what the rollout cases use)"""
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    out = dict(act=rng.uniform(-1.2, 1.2, (rows, 2)).astype(np.float32), wq2=mlp_weights_flat(rng, 8, 1),
               rew=rng.uniform(-30, 0, rows).astype(np.float32), obs2=reset_law_obs(rng, rows))
    return out


def weights(select):
    return np.linspace(0.2, 0.5, len(select)).astype(np.float32)


# ---- the oracle on a case ----------------------------------------------------------------------------------------------------
def pg_arrays(ocfg, wp, wq, obs, eps, select, w, all_steps, dtype=torch.float64, variant=None, log=None):
    """mpg_rollout_pg's outputs by the oracle: the six gradient arrays of -sum_k w_k * reduced[select_k], the selected mean returns,
    the selected sums of squared returns"""
    nets = O.Nets(ocfg, {'policy': wp, 'Q1': wq}, dtype=dtype)
    reduced, _, allret = O.model_rollout_for_policy_update(ocfg, nets, torch.as_tensor(obs).to(dtype), torch.as_tensor(eps).to(dtype),
                                                           rollout_policy='policy' if all_steps else 'policy_rollout',
                                                           model=model_of(ocfg, variant, log))
    loss = -sum(float(wk) * reduced[k] for wk, k in zip(w, select))
    grads = [x.numpy().astype(np.float64) for x in torch.autograd.grad(loss, nets.w['policy'])]
    sel = list(select)
    return grads, reduced[sel].detach().numpy().astype(np.float64), (allret[sel] ** 2).sum(1).detach().numpy().astype(np.float64)


def ampc_arrays(ocfg, wp, obs, eps, dtype=torch.float64, variant=None, log=None):
    """mpg_ampc_pg's outputs by tests/ampc_oracle.py: the six arrays of the un-clipped gradient of -mean(reward sums), the reward
    sum of every trajectory"""
    acfg = A.make_cfg(K=ocfg.obs_dim - 6, n=ocfg.n, M=ocfg.M)
    nets = O.Nets(acfg, {'policy': wp}, dtype=dtype)
    grads, st = A.compute_gradient(acfg, nets, obs, eps, clip=False, model=model_of(acfg, variant, log))
    return [np.asarray(g, np.float64) for g in grads], st['rewards_sum'].astype(np.float64)


def q_values(ocfg, wp, wq, obs, act, eps, select, M, dtype=torch.float64, variant=None, log=None):
    """mpg_rollout_q_estimation's output by the oracle (select = [n]: mpg_rollout_q_target's n-step target); the critic handed in
    stands for Q1_target"""
    nets = O.Nets(ocfg, {'policy': wp, 'Q1': wq}, target_scale=1.0, dtype=dtype)
    t = lambda x: torch.as_tensor(x).to(dtype)
    return O.model_rollout_for_q_estimation(ocfg, nets, t(obs), t(act), t(eps), list(select), M=M,
                                            model=model_of(ocfg, variant, log)).numpy().astype(np.float64)


# ---- what a trajectory log holds ---------------------------------------------------------------------------------------------
def branch_counts(log):
    """log of an EdgePathTrackingModel -> dict: clamped (trajectory, step) pairs at either end, wraps in either direction,
    trajectories that are clamped at some step and not at the last one, the nearest raw value to a threshold"""
    vx = np.stack([a for a, _ in log])            # [n][R]
    dphi = np.stack([b for _, b in log])
    hi, lo = vx > 35., vx < 1.
    clamped = hi | lo
    return dict(clamp_hi=int(hi.sum()), clamp_lo=int(lo.sum()), wrap_down=int((dphi > np.pi).sum()), wrap_up=int((dphi <= -np.pi).sum()),
                leave=int((clamped.any(0) & ~clamped[-1]).sum()),
                near_vx=float(np.minimum(np.abs(vx - 1.), np.abs(vx - 35.)).min()), near_dphi=float(np.abs(np.abs(dphi) - np.pi).min()),
                max_abs_dphi=float(np.abs(dphi).max()))


# ---- the cases of tests/test_model_edges_gpu.py ------------------------------------------------------------------------------
# mpg_rollout_pg: (env, rows, M, n, select, look-ahead K, all-steps mode, packed weight image, noise drawn in the kernel)
PG_CASES = [
    (PT, 48, 1, 25, (0, 5, 25), 0, STEP0, False, False), (PT, 48, 1, 25, (0, 5, 25), 0, STEP0, True, False),
    (PT, 48, 1, 25, (0, 5, 25), 0, ALL, False, False), (PT, 48, 1, 25, (0, 5, 25), 0, ALL, True, False),       # packed + all: THIN
    (PT, 48, 1, 25, (0, 5, 25), 3, STEP0, False, False), (PT, 48, 1, 25, (0, 5, 25), 3, STEP0, True, False),  # K = 3: the WIDE forms
    (PT, 48, 1, 25, (0, 5, 25), 3, ALL, False, False), (PT, 48, 1, 25, (0, 5, 25), 3, ALL, True, False),
    (PT, 33, 2, 31, (0, 16, 31), 0, STEP0, False, False),                                                     # ragged, the longest horizon
    (PT, 48, 1, 25, (0, 5, 25), 0, STEP0, False, True),                                                       # eps = NULL
    (PD, 48, 1, 25, (0, 5, 25), 0, STEP0, False, False), (PD, 48, 1, 25, (0, 5, 25), 0, STEP0, True, False),
    (PD, 48, 1, 25, (0, 5, 25), 0, ALL, False, False), (PD, 48, 1, 25, (0, 5, 25), 0, ALL, True, False),
]
# the PCG64 seed of every distinct set of inputs (env, rows, M, n, K, philox): chosen by tests/test_model_edges.py's conditions -
# a seed whose float64 trajectory comes within 1e-3 of a threshold, or that leaves a branch untaken, is not used
SEEDS = {(PT, 48, 1, 25, 0, False): 1, (PT, 48, 1, 25, 3, False): 8, (PT, 33, 2, 31, 0, False): 1, (PT, 48, 1, 25, 0, True): 1,
         (PT, 48, 2, 25, 0, False): 1, (PD, 48, 1, 25, 0, False): 1}


def seed_of(env, rows, M, n, K, philox=False):
    return SEEDS[(env, rows, M, n, K, philox)]


def pg_id(c):
    return '%s-rows%d-M%d-n%d-sel%s-K%d-%s-%s%s' % (c[0], c[1], c[2], c[3], '_'.join(str(k) for k in c[4]), c[5], 'all' if c[6] else 'step0',
                                                     'packed' if c[7] else 'plain', '-philox' if c[8] else '')


def pg_inputs(case):
    env, rows, M, n, select, K, all_steps, packed, philox = case
    return inputs(env, rows, M, n, K, seed_of(env, rows, M, n, K, philox), philox)


@functools.lru_cache(maxsize=None)
def pg_reference(env, rows, M, n, select, K, all_steps, philox, dtype=torch.float64):
    """(flat gradient, mean returns, sums of squared returns) of a mpg_rollout_pg case - the same for both weight-image forms"""
    ocfg, wp, wq, obs, eps = inputs(env, rows, M, n, K, seed_of(env, rows, M, n, K, philox), philox)
    grads, red, m2 = pg_arrays(ocfg, wp, wq, obs, eps, select, weights(select), all_steps, dtype)
    return np.concatenate([g.ravel() for g in grads]), red, m2


# mpg_ampc_pg, mpg_rollout_q_estimation / mpg_rollout_q_target and mpg_mpg_gradients run on the inputs of the first case above
# (48 rows, n = 25, K = 0; q-estimation with M = 2 on a set of its own: twice the trajectories)
BASE = (PT, 48, 1, 25, 0)
Q_SELECT = (0, 5, 25)
Q_CASES = [('estimation', 1), ('estimation', 2), ('target', 1)]           # (entry point, M)
MG_SELECT, MG_ITERATION = (0, 25), 4500          # iteration 4500: lam = 1, the rule gives both slices the same weight


def q_inputs(M):
    env, rows, _, n, K = BASE
    ocfg, wp, wq, obs, eps = inputs(env, rows, M, n, K, seed_of(env, rows, M, n, K))
    return ocfg, wp, wq, obs, extras(rows, seed_of(env, rows, M, n, K))['act'], eps


@functools.lru_cache(maxsize=None)
def q_reference(kind, M, dtype=torch.float64):
    ocfg, wp, wq, obs, act, eps = q_inputs(M)
    return q_values(ocfg, wp, wq, obs, act, eps, Q_SELECT if kind == 'estimation' else (ocfg.n,), M, dtype)


@functools.lru_cache(maxsize=None)
def ampc_reference(dtype=torch.float64):
    """(flat gradient, reward sum of every trajectory) of the mpg_ampc_pg case"""
    ocfg, wp, wq, obs, eps = inputs(*BASE, seed_of(*BASE))
    grads, rsum = ampc_arrays(ocfg, wp, obs, eps, dtype)
    return np.concatenate([g.ravel() for g in grads]), rsum


def mg_inputs():
    """the mpg_mpg_gradients case: the networks, start rows and noise of BASE (the batch observations ARE the edge rows), a second
    critic and the rest of a replay batch from extras()"""
    ocfg, wp, wq, obs, eps = inputs(*BASE, seed_of(*BASE))
    x = extras(obs.shape[0], seed_of(*BASE))
    return {'Q1': wq, 'Q2': x['wq2'], 'policy': wp}, obs, x['act'], x['rew'], x['obs2'], eps


@functools.lru_cache(maxsize=None)
def mg_reference():
    """O.mpg_compute_gradient in float64 with a clip so large that nothing is scaled -> (flat gradient in the order Q1, Q2, policy,
    the oracle's stats, mean returns and sums of squared returns of MG_SELECT, the weights as the learners hand them over)"""
    w, obs, act, rew, obs2, eps = mg_inputs()
    mcfg = O.Cfg(select=list(MG_SELECT), clip=1e30)
    ws = O.rule_based_weights(MG_ITERATION, mcfg.total_ite, mcfg.eta, mcfg.select).numpy()
    nets = O.Nets(mcfg, w, target_scale=0.97, dtype=torch.float64)
    grads, st = O.mpg_compute_gradient(mcfg, nets, [np.array(obs), np.array(act), np.array(rew), np.array(obs2), None], np.array(eps), MG_ITERATION)
    _, red, m2 = pg_arrays(mcfg, w['policy'], w['Q1'], obs, eps, MG_SELECT, ws, STEP0)
    return np.concatenate([g.ravel() for g in grads]), st, red, m2, ws
