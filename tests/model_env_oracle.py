"""The double pendulum's model as an environment - what mpg_model_env_reset, mpg_model_env_step, mpg_model_env_step_store_reset and
mpg_worker_rollout_model compute (include/mpg_hip.h) - restated in float32 and float64 on the step of
tests/model_rollout_oracle.py and the Philox restatement of oracle/mpg_oracle.py.  A plain helper module shared by tests/test_model_env.py
(CPU) and tests/test_model_env_gpu.py; mpg_amd never imports it.

  step   obs_next, RAW rew = model_rollout_oracle.step on the double pendulum's cfg (atan2 of the row, five Euler sub-steps, the reward)
  done   fell = not (tip_y > 1), tip_y = 0.6 obs_next[3] + 0.6 obs_next[4]; truncated = max_steps > 0 and age + 1 >= max_steps
  reset  p, theta1, theta2 ~ U(-0.1, 0.1) from words 0 .. 2 of Philox(counter = (agent, ctr_lo, ctr_hi, 'dpme'), key = seed); pdot,
         theta1dot, theta2dot = 0.1 x (r0 cos, r0 sin, r1 cos) by Box-Muller from the word pairs of the block with counter word 'dpme' + 1
"""
import numpy as np
import torch

from oracle import mpg_oracle as O
from tests import dp_oracle as DP
from tests import model_rollout_oracle as M

ENV_ID = DP.ENV_ID
OD, AD = 11, 1
RESET_TAG = 0x64706d65
MAX_STEPS = 1000                # gym's registered limit for the id: the Python side's default
F32 = np.float32


def np_dtype(dtype):
    return np.float64 if dtype == torch.float64 else np.float32


def tip_y(obs_next, dtype=torch.float32):
    """the done law's tip height of the rows obs_next [n, 11]: in float32 two rounded products and one rounded sum, as the kernel forms
    it (no contraction); in float64 the same expression on the doubles"""
    t = np_dtype(dtype)
    o = np.asarray(obs_next).astype(t)
    c = t(0.6) if t is np.float64 else F32(0.6)
    return (c * o[:, 3]).astype(t) + (c * o[:, 4]).astype(t)


def fell(obs_next, dtype=torch.float32):
    """negated, so that a NaN row is done"""
    with np.errstate(invalid='ignore'):
        return ~(tip_y(obs_next, dtype) > 1.0)


def truncated(age, max_steps):
    age = np.asarray(age, np.int64)
    return np.full(age.shape, False) if max_steps <= 0 else (age + 1 >= max_steps)


def step(obs, act, age, max_steps=MAX_STEPS, dtype=torch.float64):
    """-> (obs_next [n, 11], rew [n] RAW, done [n] uint8, age + 1); nothing is reset here"""
    with np.errstate(invalid='ignore'):
        o, r = M.step(DP.make_cfg(), obs, act, None, dtype)
    done = fell(o, dtype) | truncated(age, max_steps)
    return o, r, done.astype(np.uint8), np.asarray(age, np.int32) + 1


def reset_rows(n, seed, ctr, dtype=torch.float32):
    """the rows the reset law draws for agents 0 .. n - 1 keyed (seed, ctr): [n, 11].  The uniforms u01 are float32 values in either
    precision (24 random bits); everything behind them is computed in `dtype`."""
    t = np_dtype(dtype)
    k0, k1 = O._key(seed)
    c_lo, c_hi = O._key(ctr)
    i = np.arange(n, dtype=np.uint64)
    a = O.philox4x32_10(i, c_lo, c_hi, RESET_TAG, k0, k1)
    b = O.philox4x32_10(i, c_lo, c_hi, RESET_TAG + 1, k0, k1)
    u = [O.u01(x).astype(t) for x in a]
    v = [O.u01(x).astype(t) for x in b]
    p, t1, t2 = [(t(0.2) * u[k] - t(0.1)).astype(t) for k in range(3)]
    two_pi = t(6.283185307179586)
    r0, r1 = np.sqrt(t(-2.) * np.log(v[0])).astype(t), np.sqrt(t(-2.) * np.log(v[2])).astype(t)
    a0, a1 = two_pi * v[1], two_pi * v[3]
    pd, t1d, t2d = t(0.1) * (r0 * np.cos(a0)), t(0.1) * (r0 * np.sin(a0)), t(0.1) * (r1 * np.cos(a1))
    z = np.zeros(n, t)
    return np.stack([p, np.sin(t1), np.sin(t2), np.cos(t1), np.cos(t2), pd, t1d, t2d, z, z, z], 1).astype(t)


def reset_state(n, seed, ctr):
    """the float64 state [p, theta1, theta2, pdot, theta1dot, theta2dot] behind reset_rows: what the ranges of the law are asserted on"""
    k0, k1 = O._key(seed)
    c_lo, c_hi = O._key(ctr)
    i = np.arange(n, dtype=np.uint64)
    a = O.philox4x32_10(i, c_lo, c_hi, RESET_TAG, k0, k1)
    b = O.philox4x32_10(i, c_lo, c_hi, RESET_TAG + 1, k0, k1)
    u = [O.u01(x).astype(np.float64) for x in a]
    v = [O.u01(x).astype(np.float64) for x in b]
    r0, r1 = np.sqrt(-2. * np.log(v[0])), np.sqrt(-2. * np.log(v[2]))
    return np.stack([0.2 * u[0] - 0.1, 0.2 * u[1] - 0.1, 0.2 * u[2] - 0.1, 0.1 * r0 * np.cos(2 * np.pi * v[1]),
                     0.1 * r0 * np.sin(2 * np.pi * v[1]), 0.1 * r1 * np.cos(2 * np.pi * v[3])], 1)


def reset(obs, age, mask, seed, ctr, dtype=torch.float32):
    """mpg_model_env_reset: -> (obs, age) with the agents of `mask` (None: all) re-drawn and their age 0; the others as they were"""
    obs, age = np.array(obs, np_dtype(dtype)), np.array(age, np.int32)
    m = np.ones(obs.shape[0], bool) if mask is None else np.asarray(mask).astype(bool)
    obs[m] = reset_rows(obs.shape[0], seed, ctr, dtype)[m]
    age[m] = 0
    return obs, age


def sample_loop(obs, age, iters, max_steps, env_seed, env_ctr, dtype=torch.float64, wp=None, actions=None, sigma=0., noise_seed=0,
                noise_ctr=0):
    """OffPolicyWorker._sample_loop on the model env, `iters` iterations: the policy's action on the processed observation plus the
    exploration noise as the policy kernel draws it (or actions[it], teacher-forced), step, the transition, reset of the done agents
    keyed (env_seed, env_ctr + it).  -> dict(obs, act, rew, obs2, done: [iters, n, .] in iteration order; obs_io, age_io: what is
    left)"""
    ocfg = DP.make_cfg()
    nets = M.nets_of(ocfg, wp, dtype) if actions is None else None
    t = np_dtype(dtype)
    obs, age = np.asarray(obs).astype(t), np.asarray(age, np.int32)
    n = obs.shape[0]
    out = dict(obs=[], act=[], rew=[], obs2=[], done=[])
    for it in range(iters):
        if actions is None:
            with torch.no_grad(), np.errstate(invalid='ignore'):
                act = nets.compute_action(O.process_obses(ocfg, torch.as_tensor(obs).to(dtype))).numpy().astype(t)
            if sigma > 0.:
                act = (act + O.explore_noise_philox(n, AD, sigma, noise_seed, noise_ctr + it).astype(t)).astype(t)
        else:
            act = np.asarray(actions[it]).astype(t)
        o2, r, d, age = step(obs, act, age, max_steps, dtype)
        for k, x in zip(('obs', 'act', 'rew', 'obs2', 'done'), (obs, act, r, o2, d)):
            out[k].append(x)
        obs, age = reset(o2, age, d, env_seed, env_ctr + it, dtype)
    out = {k: np.stack(v) for k, v in out.items()}
    out.update(obs_io=obs, age_io=age)
    return out


def first_done(done):
    """done [iters, n] -> per agent the first iteration with done = 1 (iters where there is none)"""
    done = np.asarray(done).astype(bool)
    return np.where(done.any(0), done.argmax(0), done.shape[0])


def leaning_rows(n, theta, rng=None, spread=0.):
    """start rows at rest with both rods at `theta` (+ U(-spread, spread) per row): tip_y = 1.2 cos(theta), so theta near 0.55 (tip_y
    1.023) falls below 1 within a few steps whatever a bounded action does"""
    th = np.full((n, 2), theta, np.float64)
    if rng is not None and spread:
        th += rng.uniform(-spread, spread, (n, 2))
    z = np.zeros((n, 1))
    return np.concatenate([z, np.sin(th), np.cos(th), np.zeros((n, 3)), np.zeros((n, 3))], 1).astype(F32)


def seam_theta():
    """the angle theta (both rods, at rest, action 0) from which ONE step ends at tip_y = 1 in the float64 oracle, by bisection"""
    lo, hi = 0.3, 0.7

    def f(th):
        o, _, _, _ = step(_row64(th), np.zeros((1, 1)), np.zeros(1, np.int32), 0)
        return tip_y(o, torch.float64)[0] - 1.
    assert f(lo) > 0 > f(hi)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid) > 0 else (lo, mid)
    return 0.5 * (lo + hi)


def _row64(th):
    return np.array([[0., np.sin(th), np.sin(th), np.cos(th), np.cos(th), 0., 0., 0., 0., 0., 0.]])


def seam_rows(n=4096):
    """n start rows at rest: rod 2 at seam_theta(), rod 1 stepping through consecutive float32 values of sin(theta1) around it.  One
    step takes their tip_y through the float32 values next to 1 - a row moves it by about a third of an ulp of 1, so 1, the value
    above and the value below are all reached (asserted where the rows are used)."""
    th0 = seam_theta()
    s = F32(np.sin(th0))
    for _ in range(n // 2):
        s = np.nextafter(s, F32(0))
    sines = np.empty(n, F32)
    for k in range(n):
        sines[k] = s
        s = np.nextafter(s, F32(1))
    cos = np.sqrt(1. - sines.astype(np.float64) ** 2).astype(F32)
    z = np.zeros(n, F32)
    s2, c2 = np.full(n, F32(np.sin(th0))), np.full(n, F32(np.cos(th0)))
    return np.stack([z, sines, s2, cos, c2, z, z, z, z, z, z], 1)
