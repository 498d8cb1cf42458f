"""MPC's closed loop on the learners' models, on the CPU: the oracle (tests/model_mpc_rollout_oracle.py) against its own properties, the
input sets of tests/test_model_mpc_rollout_gpu.py - built HERE: start rows, start points and plant noise, rows being independent the GPU
test takes the leading rows - with the reasons they are worth running, and the chunking arithmetic of run_model_mpc(one_launch=True).

 1. The oracle: two calls of s1 and s2 steps are one call of s1 + s2; the warm start is the plan one action later; a cold solve does not
    depend on the step before.
 2. The input sets, in float64: warm and cold loops differ; with tol = 1e-3 some rows of a wave stop early and others do not; a
    PathTracking row reaches the v_x clamp within the steps run; a double-pendulum row passes +-pi.
 3. mpc.model_rollout_chunk for iters 0, 1, the cap and cap + 1."""
import functools

import numpy as np
import pytest
import torch

from tests import model_mpc_rollout_oracle as RO
from tests import model_rollout_oracle as R
from tests.test_model_mpc import MODEL_IDS, MODELS, POOL, input_set

ITERS = 20                      # the GPU test's iterations per solve
ALL = range(len(MODELS))


# ---- the input sets -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def start_rows(mi):
    """POOL start rows of model MODELS[mi]: tests/test_model_mpc.input_set's at horizon 25 (PathTracking: the 16 rows of
    tests/model_edge_inputs.edge_obs first).  Double pendulum: rows 4 .. 7 are overwritten with a first rod 0.05 .. 0.2 rad short of
    hanging straight down on either side and turning towards it at 3 .. 6 rad/s, so that the angle the step re-reads by atan2 passes
    +-pi within a few steps."""
    obs = input_set(mi, 25)[1].copy()
    if MODELS[mi][0] == R.DPEND:
        rng = np.random.Generator(np.random.PCG64(31))
        sign = np.array([1., -1., 1., -1.])
        th = sign * (np.pi - rng.uniform(0.05, 0.2, 4))
        obs[4:8, 1], obs[4:8, 3] = np.sin(th), np.cos(th)
        obs[4:8, 6] = sign * rng.uniform(3., 6., 4)
    return obs


@functools.lru_cache(maxsize=None)
def start_point(mi, h, kind):
    """POOL start points [POOL, h, act_dim]: 'zeros'; 'outside', uniform in [-1.25, 1.25] - a fifth of the entries outside the box;
    'throttle', the last action entry +1.25 on even rows and -1.25 on odd ones at every step, the rest zeros - on PathTracking full
    throttle and full braking once the solver's setup has clamped them"""
    ad = R.ocfg_of(*MODELS[mi]).act_dim
    if kind == 'zeros':
        return np.zeros((POOL, h, ad), np.float32)
    if kind == 'throttle':
        u = np.zeros((POOL, h, ad), np.float32)
        u[0::2, :, -1], u[1::2, :, -1] = 1.25, -1.25
        return u
    u = np.random.default_rng(40 + mi + h).uniform(-1.25, 1.25, (POOL, h, ad)).astype(np.float32)
    assert 0.1 < (np.abs(u) > 1).mean() < 0.3
    return u


@functools.lru_cache(maxsize=None)
def plant_noise(mi, steps):
    """[steps, POOL] standard normal"""
    return np.random.default_rng(70 + mi).standard_normal((steps, POOL)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def loop64(mi, n, steps, h, iters, tol, warm, start, with_eps):
    """the float64 closed loop on the leading n rows of a set"""
    ocfg = R.ocfg_of(*MODELS[mi])
    eps = plant_noise(mi, steps)[:, :n] if with_eps else None
    return RO.closed_loop(ocfg, start_rows(mi)[:n], start_point(mi, h, start)[:n], steps, iters, tol, warm, eps)


# ---- 1: the oracle's own properties -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('warm', [False, True], ids=['cold', 'warm'])
@pytest.mark.parametrize('mi', [0, 2], ids=['pt', 'pendulum'])
def test_oracle_split_shift_and_cold_independence(mi, warm, dtype):
    ocfg = R.ocfg_of(*MODELS[mi])
    n, h, steps = 6, 4, 4
    obs, u0, eps = start_rows(mi)[16:16 + n], start_point(mi, h, 'outside')[:n], plant_noise(mi, steps)[:, :n]
    whole = RO.closed_loop(ocfg, obs, u0, steps, 8, 1e-3, warm, eps, dtype)
    a = RO.closed_loop(ocfg, obs, u0, 1, 8, 1e-3, warm, eps[:1], dtype)
    b = RO.closed_loop(ocfg, a['last_obs'], a['u_next'], 3, 8, 1e-3, warm, eps[1:], dtype)
    for k in ('obs_traj', 'plan_traj', 'rew_traj', 'cost_traj', 'pgnorm_traj', 'info_traj'):
        assert whole[k].dtype == (np.int32 if k == 'info_traj' else RO.NP[dtype])
        assert np.array_equal(np.concatenate([a[k], b[k]]), whole[k]), k
    assert np.array_equal(b['last_obs'], whole['last_obs']) and np.array_equal(b['u_next'], whole['u_next'])
    assert np.array_equal(whole['obs_traj'][0], obs.astype(RO.NP[dtype]))
    assert np.abs(whole['plan_traj']).max() <= 1.
    if warm:      # the next start point is the plan one action later, its last action repeated
        last = whole['plan_traj'][-1]
        assert np.array_equal(whole['u_next'][:, :-1], last[:, 1:]) and np.array_equal(whole['u_next'][:, -1], last[:, -1])
    else:         # a cold solve depends on its row alone: solved again from the recorded row, it gives the recorded plan
        assert np.array_equal(whole['u_next'], u0.astype(RO.NP[dtype]))
        again = RO.closed_loop(ocfg, whole['obs_traj'][2], u0, 1, 8, 1e-3, False, None, dtype)
        assert np.array_equal(again['plan_traj'][0], whole['plan_traj'][2]) and np.array_equal(again['cost_traj'][0], whole['cost_traj'][2])
    # the planner plans at the noise means: the first plan does not see the plant's noise, the second row does (models with noise)
    quiet = RO.closed_loop(ocfg, obs, u0, 2, 8, 1e-3, warm, None, dtype)
    assert np.array_equal(quiet['plan_traj'][0], whole['plan_traj'][0]) and not np.array_equal(quiet['obs_traj'][1], whole['obs_traj'][1])


# ---- 2: the input sets are worth running --------------------------------------------------------------------------------------------
def _sizes(mi):
    """(rows, steps, horizon, iterations) of the float64 loops below: the GPU test's 20 iterations at horizon 25 on the 16 leading rows
    (PathTracking's edge rows) for 3 steps; the double pendulum's at horizon 10 on 8 rows, those near +-pi among them"""
    return (8, 3, 10, ITERS) if MODELS[mi][0] == R.DPEND else (16, 3, 25, ITERS)


@pytest.mark.parametrize('mi', ALL, ids=MODEL_IDS)
def test_warm_and_cold_loops_differ(mi):
    n, steps, h, iters = _sizes(mi)
    warm = loop64(mi, n, steps, h, iters, 0., True, 'zeros', True)
    cold = loop64(mi, n, steps, h, iters, 0., False, 'zeros', True)
    assert np.array_equal(warm['plan_traj'][0], cold['plan_traj'][0])          # the first solve sees the same inputs
    d = np.abs(warm['plan_traj'][1:] - cold['plan_traj'][1:]).max(axis=(0, 2, 3))
    print('   %s: rows whose later plans differ between warm and cold %d of %d (largest difference %.3g)' % (MODEL_IDS[mi], (d > 0).sum(), n, d.max()))
    assert (d > 1e-6).sum() >= n // 2
    assert not np.array_equal(warm['obs_traj'][2:], cold['obs_traj'][2:])


@pytest.mark.parametrize('mi', [0, 1, 2], ids=MODEL_IDS[:3])
def test_a_tolerance_stops_some_rows_of_a_wave_early_and_not_others(mi):
    """200 iterations from zeros at tol = 1e-3, the setting of the GPU test's wave-split case, on 8 rows of its first wave and the first step
    (the double pendulum's 20 iterations stop no row: its case there runs for the bits alone)"""
    rec = loop64(mi, 8, 1, 25, 200, 1e-3, True, 'zeros', False)
    k = np.abs(rec['info_traj'])
    print('   %s: accepted iterations per step, min %s max %s' % (MODEL_IDS[mi], k.min(1), k.max(1)))
    assert (k.min(1) < k.max(1)).any()
    assert ((rec['pgnorm_traj'] <= 1e-3) & (rec['info_traj'] >= 0) & (k < 200)).any()


@pytest.mark.parametrize('mi', [0, 1], ids=MODEL_IDS[:2])
def test_a_path_tracking_row_reaches_the_speed_clamp(mi):
    """the GPU test's iters = 0 case: no iterations from the 'throttle' start point, so the plant takes +-1 of acceleration at every
    step - the edge rows one to seven full-throttle steps below 35 m/s and at most five braking steps above 1 m/s reach both bounds
    within the 5 steps"""
    rec = loop64(mi, 16, 5, 2, 0, 0., True, 'throttle', True)
    assert (rec['info_traj'] == 0).all() and (np.abs(rec['plan_traj'][:, :, :, 1]) == 1.).all()
    vx = np.concatenate([rec['obs_traj'][1:, :, 0], rec['last_obs'][None, :, 0]]) + 20.
    print('   %s: (step, row) pairs at the upper bound %d, at the lower %d' % (MODEL_IDS[mi], (vx == 35.).sum(), (vx == 1.).sum()))
    assert (vx == 35.).any() and (vx == 1.).any()


def test_a_double_pendulum_row_passes_pi():
    mi = 3
    n, steps, h, iters = _sizes(mi)
    rec = loop64(mi, n, steps, h, iters, 0., True, 'zeros', True)
    rows = np.concatenate([rec['obs_traj'], rec['last_obs'][None]])
    th1 = np.arctan2(rows[:, :, 1], rows[:, :, 3])
    jumped = np.abs(np.diff(th1, axis=0)) > np.pi
    print('   rows whose first angle passes +-pi: %s' % np.nonzero(jumped.any(0))[0])
    assert jumped[:, 4:8].any() and not jumped[:, 8:].any()
    assert (rows[1:, :, 8:] == 0).all() and (rows[0, :, 8:] != 0).any()


# ---- 3: the chunks of run_model_mpc(one_launch=True) --------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', [0, 1, 2])
def test_chunk_sizes(kind):
    from mpg_amd import mpc
    cap, iters_cap, max_steps = mpc.MODEL_MAX_ROLLOUT_WORK[kind], mpc.MODEL_MAX_ITERS[kind], mpc.MODEL_MAX_ROLLOUT_STEPS
    chunk = mpc.model_rollout_chunk
    # no iterations and one: the step bound alone, or the loop's own length
    assert chunk(5000, 0, cap) == max_steps and chunk(90, 0, cap) == 90
    assert chunk(5000, 1, cap) == min(cap, max_steps) and chunk(90, 1, cap) == min(cap, 90)
    # the cap: one step; cap + 1: still one step - the library refuses that launch by name, the chunk size is never 0
    assert chunk(90, cap, cap) == 1 and chunk(90, cap + 1, cap) == 1
    assert chunk(90, iters_cap, cap) == cap // iters_cap >= 1
    for steps in (1, 7, 90, 1024, 3000):
        for iters in (0, 1, 3, 20, 200, iters_cap, cap, cap + 1):
            c = chunk(steps, iters, cap)
            assert 1 <= c <= min(max_steps, max(steps, 1))
            assert c * iters <= cap or c == 1
            assert c == min(steps, max_steps) or (c + 1) * iters > cap          # as many steps as fit
            starts = list(range(0, steps, c))                                      # run_model_mpc's chunks cover the loop exactly once
            assert sum(min(c, steps - t0) for t0 in starts) == steps
    assert chunk(90, 200, 2048) == 10 and chunk(90, 200, 400) == 2 and chunk(5, 20, 40) == 2 and chunk(0, 20, 40) == 1
