"""The model-backed InvertedDoublePendulum-v2 env by the oracle alone (CPU; tests/model_env_oracle.py restates what mpg_model_env_* and
mpg_worker_rollout_model compute):

  * pinned to the UNMODIFIED reference: the env loop fed the actions of double_pendulum_model_ref.npz reproduces the fixture's obs and
    reward for every row up to and including its first done step - and every row has one (all 64 start at tip_y >= 1.1947 and fall at
    steps 3 .. 14), so the fixture alone exercises the done law on every row;
  * the seam of the done law: tip_y one ulp above 1, exactly 1, one ulp below 1 and NaN; truncation at age + 1 == max_steps, and not at
    all with max_steps = 0;
  * the ranges and moments of the reset law, the mask, the age;
  * the float32 oracle sits inside tests/yardstick.check_values' allowance against the float64 one, on the fixture's loop and on the
    policy-driven loops the GPU test compares the launch with - and those loops hold a fall and a truncation in both precisions;
  * the Python side without a device: make_model_env serves one id, make_env and the native driver keep refusing the double pendulum,
    ONE_LAUNCH names the model env's method.

Every figure is printed before anything is asserted."""
import numpy as np
import pytest
import torch

from tests import model_env_oracle as V
from tests import yardstick as Y
from tests.test_model_rollout import allowance_used

FIXTURE = 'double_pendulum_model_ref.npz'
ONE, UP, DOWN = np.float32(1.), np.nextafter(np.float32(1.), np.float32(2.)), np.nextafter(np.float32(1.), np.float32(0.))


def fixture_loop(g, dtype, max_steps=V.MAX_STEPS):
    return V.sample_loop(g['obs0'], np.zeros(64, np.int32), 25, max_steps, 9, 0, dtype, actions=g['actions'])


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['float64', 'float32'])
def test_env_loop_reproduces_the_fixture_up_to_each_rows_first_done_step(golden, dtype):
    """float64 at the restatements' bar of 1e-9 relative L2 per row, float32 under check_values on the rows' joined records"""
    g = golden(FIXTURE)
    f64 = dtype == torch.float64
    ref_o, ref_r = (g['obs_f64'], g['reward_f64']) if f64 else (g['obs'], g['reward'])
    tip0 = V.tip_y(g['obs0'], torch.float64)
    r = fixture_loop(g, dtype)
    fd = V.first_done(r['done'])
    print('start tip_y >= %.4f, first done steps %d .. %d' % (tip0.min(), fd.min(), fd.max()))
    assert tip0.min() >= 1.1947 and fd.min() == 3 and fd.max() == 14
    # the fixture's own chain says the same: its row's tip height is above 1 before that step and not above it at that step
    ty = np.stack([V.tip_y(o, torch.float64) for o in g['obs_f64']])
    assert all((ty[:fd[i], i] > 1.).all() and not ty[fd[i], i] > 1. for i in range(64))
    keep = np.arange(25)[:, None] <= fd[None, :]
    if f64:
        worst = max(max(Y.rel_l2(r['obs2'][:fd[i] + 1, i], ref_o[:fd[i] + 1, i]), Y.rel_l2(r['rew'][:fd[i] + 1, i], ref_r[:fd[i] + 1, i]))
                    for i in range(64))
        print('float64 env loop vs the reference\'s chain, worst row: %.2e' % worst)
        assert worst <= 1e-9, worst
    else:
        Y.check_values(r['obs2'][keep], g['obs'][keep], g['obs_f64'][keep], 'obs')
        Y.check_values(r['rew'][keep], g['reward'][keep], g['reward_f64'][keep], 'reward')
    # behind its first done step a row is a re-drawn agent at age 0: upright again, and no longer the fixture's falling one
    after = [(fd[i] + 1, i) for i in range(64) if fd[i] + 1 < 25]
    assert len(after) == 64
    for t, i in after:
        assert V.tip_y(r['obs'][t, i:i + 1], dtype)[0] > 1.19 and not r['obs'][t, i, 8:].any()
    assert (r['age_io'] == 24 - np.array([np.flatnonzero(r['done'][:, i])[-1] for i in range(64)])).all()


def test_done_law_at_its_seam():
    row = np.zeros((6, 11), np.float32)
    # cos2 = 0 puts tip_y = 0.6f * cos1: choose cos1 so that the rounded product is 1, its neighbours, and far values
    vals = {}
    x = np.float32(1.6666)
    while x < np.float32(1.6668):
        vals.setdefault(np.float32(np.float32(0.6) * x), x)
        x = np.nextafter(x, np.float32(2.))
    assert ONE in vals and UP in vals and DOWN in vals, len(vals)
    row[0, 3], row[1, 3], row[2, 3] = vals[UP], vals[ONE], vals[DOWN]
    row[3, 3] = np.nan
    row[4, 3], row[4, 4] = 1., 1.                  # upright: 1.2
    row[5, 3], row[5, 4] = 0.5, np.nan
    ty = V.tip_y(row)
    print('tip_y of the seam rows:', ty)
    assert ty[0] == UP and ty[1] == ONE and ty[2] == DOWN and np.isnan(ty[3]) and ty[4] == np.float32(0.6) + np.float32(0.6)
    assert list(V.fell(row)) == [False, True, True, True, False, True]
    assert list(V.fell(row, torch.float64)) == [False, True, True, True, False, True]
    # two rounded products and ONE rounded sum: a pair whose exact sum lies above 1 and rounds to 1 is done
    pair = np.zeros((1, 11), np.float32)
    pair[0, 3], pair[0, 4] = vals[ONE], np.float32(1e-9)
    p1, p2 = np.float32(np.float32(0.6) * pair[0, 3]), np.float32(np.float32(0.6) * pair[0, 4])
    assert float(p1) + float(p2) > 1. and V.tip_y(pair)[0] == ONE and V.fell(pair)[0]


def test_truncation_and_age():
    obs = V.leaning_rows(4, 0.05)
    act = np.zeros((4, 1), np.float32)
    age = np.array([0, 1, 2, 5], np.int32)
    for dtype in (torch.float32, torch.float64):
        _, _, done, age2 = V.step(obs, act, age, 3, dtype)
        assert list(done) == [0, 0, 1, 1] and list(age2) == [1, 2, 3, 6]          # age + 1 == max_steps, and beyond it
        _, _, done, _ = V.step(obs, act, age, 0, dtype)
        assert not done.any()                                                        # 0: no limit
        _, _, done, _ = V.step(obs, act, np.array([998, 999, 1000, 2 ** 31 - 2], np.int32), V.MAX_STEPS, dtype)
        assert list(done) == [0, 1, 1, 1]
        _, _, done, _ = V.step(obs, act, np.array([2 ** 31 - 2] * 4, np.int32), 0, dtype)
        assert not done.any()
    # a fallen row is done whatever its age; the reset of the done rows zeroes their age and leaves the others
    low = V.leaning_rows(4, 0.7)
    o2, _, done, age2 = V.step(low, act, age, 0, torch.float32)
    assert done.all()
    mask = np.array([1, 0, 1, 0], np.uint8)
    o3, age3 = V.reset(o2, age2, mask, 4, 9)
    assert list(age3) == [0, 2, 0, 6] and np.array_equal(o3[1::2], o2[1::2]) and not np.array_equal(o3[0], o2[0])
    assert np.array_equal(o3[0::2], V.reset_rows(4, 4, 9)[0::2])                     # the draw is keyed by the AGENT, not by its rank in the mask
    o4, age4 = V.reset(o2, age2, None, 4, 9)
    assert np.array_equal(o4, V.reset_rows(4, 4, 9)) and not age4.any()


def test_reset_law_ranges_and_moments():
    n = 200000
    st = V.reset_state(n, 1234, 0)
    print('min', st.min(0), '\nmax', st.max(0), '\nmean', st.mean(0), '\nstd', st.std(0))
    assert (np.abs(st[:, :3]) < 0.1).all() and np.abs(st[:, :3]).max() > 0.0999
    np.testing.assert_allclose(st[:, :3].mean(0), 0., atol=6e-4)                     # 4.6 sigma of a mean of 200 000 U(-0.1, 0.1)
    np.testing.assert_allclose(st[:, :3].std(0), 0.2 / np.sqrt(12.), rtol=5e-3)
    np.testing.assert_allclose(st[:, 3:].mean(0), 0., atol=1.1e-3)
    np.testing.assert_allclose(st[:, 3:].std(0), 0.1, rtol=1e-2)
    assert np.abs(st[:, 3:]).max() < 0.1 * np.sqrt(-2. * np.log(2. ** -25)) + 1e-12   # Box-Muller on 24-bit uniforms: |z| < 5.9
    assert np.abs(np.corrcoef(st.T) - np.eye(6)).max() < 0.01
    # the rows are the 11 features of that state; float32 within a few ulp of float64
    r64, r32 = V.reset_rows(n, 1234, 0, torch.float64), V.reset_rows(n, 1234, 0)
    assert r32.dtype == np.float32 and r64.dtype == np.float64 and not r64[:, 8:].any() and not r32[:, 8:].any()
    np.testing.assert_allclose(r64[:, :8], np.stack([st[:, 0], np.sin(st[:, 1]), np.sin(st[:, 2]), np.cos(st[:, 1]), np.cos(st[:, 2]),
                                                     st[:, 3], st[:, 4], st[:, 5]], 1), rtol=0, atol=1e-15)
    print('reset rows, float32 vs float64: %.2e' % np.abs(r32 - r64).max())
    np.testing.assert_allclose(r32, r64, rtol=2e-6, atol=2e-7)
    assert (V.tip_y(r32) > 1.19).all()                                               # every start is upright: far from done
    # another counter, another seed, the high words: other draws
    for other in (V.reset_rows(64, 1234, 1), V.reset_rows(64, 1235, 0), V.reset_rows(64, 1234 + 2 ** 32, 0), V.reset_rows(64, 1234, 2 ** 32)):
        assert not np.isclose(other[:, 0], r32[:64, 0]).any()


def loop_case(n, sigma=0.1, max_steps=3, iters=25):
    """the policy-driven loop of the GPU test's launch cases: fixture starts for the first rows (they fall at steps 3 .. 14 under the
    fixture's actions; under this policy's, asserted below), rows leaning at theta near 0.55 behind them, ages 0 .. 2"""
    from tests.golden_inputs import mlp_weights_flat
    rng = np.random.Generator(np.random.PCG64(77))
    wp = mlp_weights_flat(rng, 11, 2)
    obs = V.leaning_rows(n, 0.55, rng, 0.02)
    age = (np.arange(n) % 3).astype(np.int32)
    return dict(wp=wp, obs=obs, age=age, iters=iters, max_steps=max_steps, sigma=sigma, noise_seed=11, noise_ctr=7, env_seed=4, env_ctr=3)


def run_loop(c, dtype):
    return V.sample_loop(c['obs'], c['age'], c['iters'], c['max_steps'], c['env_seed'], c['env_ctr'], dtype, wp=c['wp'], sigma=c['sigma'],
                         noise_seed=c['noise_seed'], noise_ctr=c['noise_ctr'])


def falls_and_truncations(r, max_steps):
    """(falls, truncations that are not falls) of a loop's record"""
    n = r['done'].shape[1]
    f = np.stack([V.fell(o) for o in r['obs2']])
    return int(f.sum()), int((r['done'].astype(bool) & ~f).sum()), n


@pytest.mark.parametrize('sigma', [0., 0.1], ids=['no_noise', 'sigma_0.1'])
@pytest.mark.parametrize('n', [1, 15, 16, 17, 33])
def test_float32_loop_is_inside_the_allowance_and_holds_a_fall_and_a_truncation(n, sigma):
    c = loop_case(n, sigma)
    r64, r32 = run_loop(c, torch.float64), run_loop(c, torch.float32)
    for r in (r64, r32):
        falls, truncs, _ = falls_and_truncations(r, c['max_steps'])
        assert falls >= 1 and truncs >= 1, (falls, truncs)
    print('n %d: falls / truncations %s; done flags equal in both precisions: %s' %
          (n, falls_and_truncations(r64, 3)[:2], np.array_equal(r64['done'], r32['done'])))
    used = {k: allowance_used(r32[k], r32[k], r64[k]) for k in ('obs2', 'rew')}
    e = {k: Y.rel_l2(r32[k], r64[k]) for k in ('obs', 'act', 'rew', 'obs2')}
    print('   float32 vs float64: %s' % '  '.join('%s %.1e' % kv for kv in e.items()))
    assert np.array_equal(r64['done'], r32['done']) and np.array_equal(r64['age_io'], r32['age_io'])
    assert max(e.values()) <= 1e-4 / 4., e
    assert max(used.values()) <= 1., used


def test_fixture_loop_float32_is_inside_the_allowance(golden):
    """the whole 25 x 64 record, resets included (the reset rows are float32 restatements of the same draws)"""
    g = golden(FIXTURE)
    r64, r32 = fixture_loop(g, torch.float64), fixture_loop(g, torch.float32)
    assert np.array_equal(r64['done'], r32['done'])
    for k in ('obs2', 'rew', 'obs'):
        e = Y.rel_l2(r32[k], r64[k])
        print('%s float32 vs float64 %.2e' % (k, e))
        assert e <= 1e-4 / 4., (k, e)


# ---- the Python side, without a device ----------------------------------------------------------------------------------------------
def test_make_model_env_serves_one_id_and_make_env_keeps_refusing_it():
    from mpg_amd import envs
    for env_id in ('PathTracking-v0', 'InvertedPendulumConti-v0', 'Pendulum-v1'):
        with pytest.raises(ValueError, match='no model-backed environment for .%s.' % env_id):
            envs.make_model_env(env_id, device='cpu')
    with pytest.raises(ValueError, match='no device environment for .InvertedDoublePendulum-v2.'):
        envs.make_env(V.ENV_ID, device='cpu')
    env = envs.make_model_env(V.ENV_ID, num_agent=5, device='cpu', seed=3)
    assert (env.kind, env.obs_dim, env.act_dim, env.max_episode_steps) == (2, 11, 1, 1000)
    assert env._state.dtype == torch.int32 and env._state.shape == (5,) and env.obs.shape == (5, 11)
    assert (env.cfg.env_kind, env.cfg.obs_dim, env.cfg.act_dim) == (2, 11, 1)
    assert envs.make_model_env(V.ENV_ID, device='cpu', max_episode_steps=0).max_episode_steps == 0
    with pytest.raises(ValueError, match='max_episode_steps >= 0'):
        envs.make_model_env(V.ENV_ID, device='cpu', max_episode_steps=-1)
    # reset(init_obs=) takes the rows and zeroes the ages, without a launch
    env._state += 7
    obs = env.reset(init_obs=torch.ones(5, 11))
    assert obs.shape == (5, 11) and not env._state.any() and env._initialised


def test_one_launch_table_names_the_model_envs_method():
    from mpg_amd.worker import ONE_LAUNCH, OffPolicyWorker
    name, wrong_policy, wrong_env, too_many = ONE_LAUNCH[2, False]
    assert name == '_sample_one_launch_model' and callable(getattr(OffPolicyWorker, name))
    assert 'deterministic policy only' in wrong_policy and '%s' in wrong_env and too_many == 'on the model env'
    assert (2, True) not in ONE_LAUNCH


def test_native_stack_leaves_the_model_env_to_the_method_path():
    from types import SimpleNamespace as NS
    from mpg_amd.fused import native_stack
    from mpg_amd.learners import AMPCLearner, NADPLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer as Opt
    rb = object()
    for cls, attrs in ((NADPLearner, dict(n_q=25, n_pi=25, num_batch_reuse=1)), (AMPCLearner, dict(n=25, M=1, batch_size=64))):
        ln = cls.__new__(cls)
        ln.__dict__.update(attrs, args=NS(buffer_type='normal'))
        real = NS(env=NS(kind=1), explore_sigma=None)
        model = NS(env=NS(kind=2), explore_sigma=None)
        assert native_stack(real, ln, rb) is not None and native_stack(model, ln, rb) is None
    ln = AMPCLearner.__new__(AMPCLearner)
    ln.__dict__.update(n=25, M=1, batch_size=64)
    reason = Opt._native_refusal('native_ampc', NS(env=NS(kind=2)), ln, rb, NS(buffer_type='normal'))
    assert reason and 'model-backed env' in reason
    assert Opt._native_refusal('native_ampc', NS(env=NS(kind=1)), ln, rb, NS(buffer_type='normal')) is None
