"""mpg_model_step and mpg_model_rollout on the device, both engines (tests/model_rollout_oracle.py restates them; tests/test_model_rollout.py
says on the CPU why these comparisons are worth running).

 1. mpg_model_step against the chains of the UNMODIFIED reference (model_rollout_ref.npz, pendulum_model_ref.npz,
    double_pendulum_model_ref.npz), 64 rows per step: teacher-forced from the fixture's float32 observations, and free-running over the
    25 steps - gated for the models of tests/test_model_rollout.FREE_RUNNING_GATED (there: all three; the float32 oracle run the same
    way stays 4 x inside the rule), printed otherwise - under tests/yardstick.check_values.
 2. mpg_model_step at the models' edges (v_x clamped at both ends, the heading error wrapped both ways, a pendulum angle beyond +-pi)
    against the float64 oracle step under check_values; rows 48 and 17.
 3. One launch == the chain of mpg_policy_action + mpg_model_step, bit for bit, the status word included: n in {1, 16, 17, 40} x steps in
    {1, 2, 25}, PathTracking K = 0 and K = 3, pendulum, double pendulum, packed and strided weights, eps given and NULL; 272
    trajectories x 60 steps (17 workgroups, and the one step count here beyond the 32 steps of model noise a workgroup holds at a
    time); a NaN start row; 20 repeated launches.
 4. One launch against the float64 oracle loop, 48 trajectories x 25 steps, each model, under check_values.
 5. The anchor to the sweeps: the processed rewards of rew_traj sum to mpg_ampc_pg's ret_sum (ret_sum / rows: rtol 5e-5, atol 1e-6, the
    bars of tests/test_slices_gpu.py).
 6. ModelEvaluator: the metrics against the float64 restatement of evaluator.py:160-211 on the record (tests/test_eval_rollout_gpu.py's
    bar), the double pendulum's two keys and a shared stack's current weights, gap_to_env.
Every figure is printed before it is asserted.

Measured on the MI355X, share of the check_values allowance used (split engine | exact-fp32 engine; <= 1 passes):
  step on the fixtures, teacher-forced obs / reward   PathTracking 0.066 / 0.116, pendulum 0.111 / 0.113, double pendulum 0.227 / 0.209 (both engines)
  step on the fixtures, free-running obs / reward     PathTracking 0.068 / 0.152, pendulum 0.093 / 0.115, double pendulum 0.217 / 0.203 (both engines)
  step at the edges, worst of obs and reward          PathTracking K = 0: 0.055, K = 3: 0.062, pendulum 48 rows 0.048, 17 rows 0.045 (both engines)
  launch against the float64 loop, obs_traj / rew_traj PathTracking K = 0: 0.070 / 0.164 | 0.069 / 0.162, K = 3: 0.062 / 0.110 | 0.062 / 0.116,
                                                      pendulum 0.124 / 0.140 | 0.126 / 0.157, double pendulum 0.225 / 0.214 | 0.288 / 0.286
  anchor, |rew_traj sum / ret_sum - 1|                PathTracking 2.9e-8 | 7.8e-8, pendulum 6.5e-9 | 3.5e-8 (bar 5e-5)
  evaluator metrics                                   every metric below 1e-3 of its bar
(The step kernels do not touch the network engine: their figures are the same under both libraries.)"""
import ctypes

import numpy as np
import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops
from tests import dp_oracle as DP
from tests import model_edge_inputs as E
from tests import model_rollout_oracle as M
from tests import yardstick as Y
from tests.golden_inputs import mlp_weights_flat, reset_law_obs
from tests.test_model_rollout import FREE_RUNNING_GATED, allowance_used
from tests.test_sac_gpu import engine  # noqa: F401  (the fixture: both builds of the library)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MODELS = [(M.PT, 0), (M.PT, 3), (M.PD, 0), (M.DPEND, 0)]
MODEL_IDS = ['pt', 'pt-K3', 'pendulum', 'double-pendulum']


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def device_cfg(env_id, K=0):
    if env_id == M.PT:
        return ops.make_cfg(M.PT, obs_dim=6 + K, obs_scale=list(M.ocfg_of(M.PT, K).obs_scale))
    return ops.make_cfg(env_id)


def start_rows(rng, env_id, K, n):
    """start observations of n trajectories under each model's own start law (PathTracking's look-ahead entries near delta_y)"""
    if env_id == M.PT:
        obs = reset_law_obs(rng, n)
        return np.concatenate([obs, obs[:, 3:4] + 0.3 * rng.standard_normal((n, K)).astype(np.float32)], 1) if K else obs
    return E.pendulum_wide_obs(rng, n) if env_id == M.PD else DP.start_obs(rng, n)


def device_step(cfg):
    def fn(o, a, e):
        on, r = ops.model_step(cfg, dev(o), dev(a), None if e is None else dev(e))
        return on.cpu().numpy(), r.cpu().numpy()
    return fn


def report(tag, got, ref32, ref64):
    print('   %-44s vs float64 %.2e (reference float32 %.2e)  vs float32 %.2e  uses %.3f of its allowance'
          % (tag, Y.rel_l2(got, ref64), Y.rel_l2(ref32, ref64), Y.rel_l2(got, ref32), allowance_used(got, ref32, ref64)))


# ---- 1: the step against the unmodified reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize('env_id', [M.PT, M.PD, M.DPEND])
def test_step_against_the_reference_chains(golden, engine, env_id):
    g, cfg = golden(M.FIXTURES[env_id]), device_cfg(env_id)
    assert g['obs0'].shape[0] == 64 and g['actions'].shape[0] == 25
    o, r = M.teacher_forced(g, None, None, device_step(cfg))
    report('%s teacher-forced obs (%s)' % (env_id, engine), o, g['obs'], g['obs_f64'])
    report('%s teacher-forced reward' % env_id, r, g['reward'], g['reward_f64'])
    fo, fr = M.free_running(g, None, None, device_step(cfg))
    report('%s free-running obs' % env_id, fo, g['obs'], g['obs_f64'])
    report('%s free-running reward' % env_id, fr, g['reward'], g['reward_f64'])
    Y.check_values(o, g['obs'], g['obs_f64'], 'teacher-forced obs')
    Y.check_values(r, g['reward'], g['reward_f64'], 'teacher-forced reward')
    if env_id in FREE_RUNNING_GATED:
        Y.check_values(fo, g['obs'], g['obs_f64'], 'free-running obs')
        Y.check_values(fr, g['reward'], g['reward_f64'], 'free-running reward')


# ---- 2: the step at the edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('env_id,K,rows', M.EDGE_STEP_CASES)
def test_step_at_the_models_edges(engine, env_id, K, rows):
    ocfg, obs, act, eps = M.edge_step_case(env_id, K, rows)
    cfg = device_cfg(env_id, K)
    o64, r64 = M.edge_step_reference(env_id, K, rows)
    o32, r32 = M.edge_step_reference(env_id, K, rows, f64=False)
    on, rew = ops.model_step(cfg, dev(obs), dev(act), dev(eps))
    on, rew = on.cpu().numpy(), rew.cpu().numpy()
    report('%s K %d rows %d obs (%s)' % (env_id, K, rows, engine), on, o32, o64)
    report('%s K %d rows %d reward' % (env_id, K, rows), rew, r32, r64)
    Y.check_values(on, o32, o64, 'obs')
    Y.check_values(rew, r32, r64, 'reward')
    if env_id == M.PT:      # the clamp is exact, and the look-ahead entries are copies of delta_y
        assert np.array_equal(on[:, 0] == 15., o64[:, 0] == 15.) and np.array_equal(on[:, 0] == -19., o64[:, 0] == -19.)
        assert (on[:, 6:] == on[:, 3:4]).all() and np.abs(on[:, 4]).max() <= np.float32(np.pi)
    # eps = NULL is eps = zeros
    a = ops.model_step(cfg, dev(obs), dev(act), None)
    b = ops.model_step(cfg, dev(obs), dev(act), torch.zeros(rows, device=DEV))
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))


# ---- 3: one launch == the chain -----------------------------------------------------------------------------------------------------
class Case(object):
    """a cfg with its policy on the device, strided or with the packed image, and a status word"""

    def __init__(self, env_id, K, rng, cache, wp=None):
        self.cfg = device_cfg(env_id, K)
        od, ou = self.cfg.obs_dim, 2 * self.cfg.act_dim
        self.pol = dev(mlp_weights_flat(rng, od, ou) if wp is None else wp)
        self.wc = None
        if cache:                                         # the packed-image instantiation: cfg.wcache[0] -> the policy's images
            self.wc = ops.WeightCache(self.pol, [(od, ou)])
            self.cfg.wcache[0] = self.wc.pointer
        self.st = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.cfg.status = self.st.data_ptr()

    def chain(self, obs0, steps, eps):
        """the sequence the launch replaces, through the two entry points: (obs_traj, act_traj, rew_traj, last_obs, status)"""
        cfg, n, od, ad = self.cfg, obs0.shape[0], self.cfg.obs_dim, self.cfg.act_dim
        self.st.zero_()
        obs = obs0.clone()
        obs_t, act_t = torch.empty(steps, n, od, device=DEV), torch.empty(steps, n, ad, device=DEV)
        rew_t = torch.empty(steps, n, device=DEV)
        for t in range(steps):
            obs_t[t].copy_(obs)
            L.call('mpg_policy_action', ctypes.byref(cfg), L.ptr(self.pol), L.c_int(n), L.ptr(obs), L.c_float(0.), L.c_u64(0), L.c_u64(0),
                   L.ptr(act_t[t]), L.stream())
            nxt = torch.empty_like(obs)
            L.call('mpg_model_step', ctypes.byref(cfg), L.c_int(n), L.ptr(obs), L.ptr(act_t[t]), L.ptr(eps[t] if eps is not None else None),
                   L.ptr(nxt), L.ptr(rew_t[t]), L.stream())
            obs = nxt
        return obs_t, act_t, rew_t, obs, int(self.st.item())

    def launch(self, obs0, steps, eps):
        self.st.zero_()
        before = obs0.clone()
        out = ops.model_rollout(self.cfg, self.pol, obs0, steps, eps)
        assert torch.equal(bits(obs0), bits(before)), 'the start observations are read, not written'
        return out + (int(self.st.item()),)


NAMES = ('obs_traj', 'act_traj', 'rew_traj', 'last obs', 'status')


def assert_same(a, b):
    for nm, x, y in zip(NAMES, a, b):
        if isinstance(x, int):
            assert x == y, (nm, x, y)
        else:
            assert x.shape == y.shape and torch.equal(bits(x), bits(y)), nm


@pytest.mark.parametrize('cache', [False, True], ids=['strided', 'packed'])
@pytest.mark.parametrize('steps', [1, 2, 25])
@pytest.mark.parametrize('env_id,K', MODELS, ids=MODEL_IDS)
def test_launch_equals_the_chain_bit_for_bit(engine, env_id, K, steps, cache):
    """n: one trajectory, a full group, one trajectory into a second group, a partial third; eps given and NULL.
    steps = 1: no hand-over through LDS; 2: the first one."""
    rng = np.random.Generator(np.random.PCG64(5000 + 10 * steps + K))
    c = Case(env_id, K, rng, cache)
    for n in (1, 16, 17, 40):
        obs0 = dev(start_rows(rng, env_id, K, n))
        eps = dev(rng.standard_normal((steps, n)))
        for e in (eps, None):
            a, b = c.chain(obs0, steps, e), c.launch(obs0, steps, e)
            assert all(torch.isfinite(x).all() for x in a[:4]), n
            assert_same(a, b)
            assert a[4] == 0, a[4]
            assert torch.equal(bits(b[0][0]), bits(obs0))
        if env_id != M.DPEND and steps > 1:     # the noise is read: the two runs differ
            assert not torch.equal(bits(a[3]), bits(c.launch(obs0, steps, eps)[3]))


@pytest.mark.parametrize('env_id,K', MODELS, ids=MODEL_IDS)
def test_launch_with_seventeen_workgroups_and_a_second_block_of_noise(engine, env_id, K):
    """272 trajectories x 60 steps.  PathTracking starts from the edge rows (the clamp and the wrap are reached along the loop)."""
    rng = np.random.Generator(np.random.PCG64(5100 + K))
    c = Case(env_id, K, rng, True)
    n, steps = 272, 60
    obs0 = dev(E.edge_obs(rng, n, K) if env_id == M.PT else start_rows(rng, env_id, K, n))
    eps = dev(rng.standard_normal((steps, n)))
    a, b = c.chain(obs0, steps, eps), c.launch(obs0, steps, eps)
    assert all(torch.isfinite(x).all() for x in a[:4])
    assert_same(a, b)
    if env_id == M.PT:      # (where this policy drives the rows is not this test's to say: the edge tests hold the branches)
        vx = b[0][:, :, 0]
        print('   K %d: records at the upper / lower clamp %d / %d' % (K, int((vx == 15.).sum()), int((vx == -19.).sum())))


@pytest.mark.parametrize('cache', [False, True], ids=['strided', 'packed'])
@pytest.mark.parametrize('env_id,K', MODELS, ids=MODEL_IDS)
def test_a_nan_start_row_is_reported_like_the_chain_and_poisons_no_other_row(engine, env_id, K, cache):
    n, row, steps = 40, 21, 12
    rng = np.random.Generator(np.random.PCG64(5200 + K))
    c = Case(env_id, K, rng, cache)
    clean = start_rows(rng, env_id, K, n)
    eps = dev(rng.standard_normal((steps, n)))
    bad = clean.copy()
    bad[row, 2] = np.nan
    a, b = c.chain(dev(bad), steps, eps), c.launch(dev(bad), steps, eps)
    assert a[4] == b[4] and b[4] & ops.STATUS_NAN, (a[4], b[4])
    assert_same(a, b)
    assert torch.isnan(b[2][:, row]).all() and torch.isnan(b[1][:, row]).all()
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[row] = False
    ref = c.launch(dev(clean), steps, eps)
    assert ref[4] == 0
    for nm, x, y in zip(NAMES[:3], b[:3], ref[:3]):
        assert torch.isfinite(x[:, keep]).all() and torch.equal(bits(x[:, keep]), bits(y[:, keep])), nm
    assert torch.equal(bits(b[3][keep]), bits(ref[3][keep]))


@pytest.mark.parametrize('env_id,K', MODELS, ids=MODEL_IDS)
def test_twenty_launches_give_identical_bits(engine, env_id, K):
    rng = np.random.Generator(np.random.PCG64(5300 + K))
    c = Case(env_id, K, rng, True)
    obs0, eps = dev(start_rows(rng, env_id, K, 40)), dev(rng.standard_normal((30, 40)))
    first = c.launch(obs0, 30, eps)
    assert all(torch.isfinite(x).all() for x in first[:4])
    for _ in range(19):
        assert_same(first, c.launch(obs0, 30, eps))


def test_stochastic_stack_acts_with_its_mean_columns(engine):
    """a SAC stack's policy has 2 * act_dim outputs too: the launch reads the mean columns under the cfg's output rule, as the chain"""
    from mpg_amd.config import default_args
    from mpg_amd.policy import PolicyWithQs
    pw = PolicyWithQs(**vars(default_args('SAC', env_id=M.PT)))
    assert not pw.deterministic_policy
    obs0 = dev(start_rows(np.random.Generator(np.random.PCG64(5400)), M.PT, 0, 17))
    out = ops.model_rollout(pw.cfg, pw.net('policy'), obs0, 21)
    assert torch.equal(bits(out[1][0]), bits(pw.compute_mode(obs0)))
    act = ops.policy_action(pw.cfg, pw.net('policy'), out[0][20])
    assert torch.equal(bits(out[1][20]), bits(act))
    pw.check_status()


def test_ops_wrappers_raise_mpg_error(engine):
    c = Case(M.DPEND, 0, np.random.Generator(np.random.PCG64(5500)), False)
    obs0 = dev(start_rows(np.random.Generator(np.random.PCG64(5501)), M.DPEND, 0, 5))
    with pytest.raises(L.MpgError, match='mpg_model_rollout: steps <= 1024'):
        ops.model_rollout(c.cfg, c.pol, obs0, 1025)
    with pytest.raises(L.MpgError, match='mpg_model_rollout: steps >= 1'):
        ops.model_rollout(c.cfg, c.pol, obs0, 0)
    c.cfg.act_dim = 2
    with pytest.raises(L.MpgError, match='mpg_model_step: the double-pendulum model has act_dim 1'):
        ops.model_step(c.cfg, obs0, torch.zeros(5, 2, device=DEV))


# ---- 4: one launch against the float64 oracle loop ----------------------------------------------------------------------------------
@pytest.mark.parametrize('env_id,K', M.LOOP_CASES, ids=MODEL_IDS)
def test_launch_against_the_float64_oracle_loop(engine, env_id, K):
    ocfg, wp, obs0, eps = M.loop_case(env_id, K)
    ref64, ref32 = M.loop_reference(env_id, K), M.loop_reference(env_id, K, f64=False)
    c = Case(env_id, K, None, True, wp=wp)
    out = c.launch(dev(obs0), M.LOOP_STEPS, dev(eps))
    got = [x.cpu().numpy() for x in out[:4]]
    for j, nm in enumerate(NAMES[:4]):
        report('%s K %d %s (%s)' % (env_id, K, nm, engine), got[j], ref32[j], ref64[j])
    assert out[4] == 0
    Y.check_values(got[0], ref32[0], ref64[0], 'obs_traj')
    Y.check_values(got[2], ref32[2], ref64[2], 'rew_traj')


# ---- 5: the anchor to the sweeps ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('env_id', [M.PT, M.PD])
def test_rewards_sum_to_the_sweeps_return(engine, env_id):
    """mpg_ampc_pg on the same rows, noise and policy (n = 25, M = 1): its forward sweep processes every raw reward as
    (r + rew_shift) * rew_scale and sums without a discount (k_ampc_returns); so does processed_return_sum on rew_traj."""
    ocfg, wp, obs0, eps = M.loop_case(env_id, 0)
    rows = obs0.shape[0]
    c = Case(env_id, 0, None, False, wp=wp)
    rew = c.launch(dev(obs0), M.LOOP_STEPS, dev(eps))[2]
    mine = M.processed_return_sum(ocfg, rew.cpu().numpy())
    ret_sum = float(ops.ampc_pg(c.cfg, c.pol, dev(obs0), dev(eps), M=1, n=M.LOOP_STEPS)[0])
    oracle = M.processed_return_sum(ocfg, M.loop_reference(env_id, 0)[2])
    print('   %s (%s): rew_traj %.7g  mpg_ampc_pg ret_sum %.7g  float64 oracle %.7g  relative difference %.2e'
          % (env_id, engine, mine, ret_sum, oracle, abs(mine / ret_sum - 1.)))
    np.testing.assert_allclose(ret_sum / rows, mine / rows, rtol=5e-5, atol=1e-6)
    np.testing.assert_allclose(mine / rows, oracle / rows, rtol=5e-5, atol=1e-6)


# ---- 6: ModelEvaluator --------------------------------------------------------------------------------------------------------------
def model_evaluator(alg, env_id, **kw):
    from mpg_amd.config import default_args
    from mpg_amd.evaluator import ModelEvaluator
    from mpg_amd.policy import PolicyWithQs
    args = default_args(alg, env_id=env_id, **kw)
    return ModelEvaluator(PolicyWithQs, env_id, args)


@pytest.mark.parametrize('env_id,steps', [(M.PT, 200), (M.PD, 26)])
def test_model_evaluator_metrics_against_the_float64_restatement(engine, env_id, steps):
    from tests.test_eval_rollout_gpu import check_metrics
    ev = model_evaluator('MPG-v2', env_id, fixed_steps=steps, num_eval_agent=5)
    pw = ev.policy_with_value
    obs0 = dev(start_rows(np.random.Generator(np.random.PCG64(5600)), env_id, 0, 5))
    eps = dev(np.random.Generator(np.random.PCG64(5601)).standard_normal((steps, 5)))
    per, mean = ev.run_n_episodes_parallel(obs0, eps)
    keys = ops.EVAL_METRIC_KEYS[ev.kind]
    assert tuple(per.keys()) == tuple(mean.keys()) == keys
    assert all(v.dtype == torch.float64 and v.shape == (5,) and not v.is_cuda for v in per.values())
    obs_t, act_t, rew_t, _ = ops.model_rollout(pw.cfg, pw.net('policy'), obs0, steps, eps)       # the record the evaluator measured
    check_metrics(env_id, steps, np.stack([per[k].numpy() for k in keys]), np.array([mean[k] for k in keys]), obs_t.cpu().numpy(),
                  act_t.cpu().numpy(), rew_t.cpu().numpy(), bar=8)
    # without start observations: a reset() draw of num_eval_agent rows
    per2, mean2 = ev.run_n_episodes_parallel()
    assert per2['episode_return'].shape == (5,) and np.isfinite(mean2['episode_return']) and mean2['episode_len'] == steps


def test_model_evaluator_on_the_double_pendulum(engine):
    from mpg_amd.config import default_args
    from mpg_amd.policy import PolicyWithQs
    steps = 50
    ev = model_evaluator('NADP', M.DPEND, fixed_steps=steps)
    assert ev.env is None
    obs0 = dev(DP.start_obs(np.random.Generator(np.random.PCG64(5700)), 7))
    per, mean = ev.run_n_episodes_parallel(obs0)
    assert tuple(per.keys()) == tuple(mean.keys()) == ('episode_return', 'episode_len')
    assert per['episode_return'].dtype == torch.float64 and per['episode_return'].shape == (7,)
    assert (per['episode_len'] == steps).all() and mean['episode_len'] == steps
    # a shared stack: the learner's CURRENT weights are what is evaluated
    pw = PolicyWithQs(**vars(default_args('NADP', env_id=M.DPEND, seed=3)))
    ev.share_policy(pw)
    per_a, _ = ev.run_n_episodes_parallel(obs0)
    pw.net('policy').mul_(0.5)
    pw.refresh_weight_cache()
    per_b, mean_b = ev.run_n_episodes_parallel(obs0)
    rew = ops.model_rollout(pw.cfg, pw.net('policy'), obs0, steps)[2]
    now = rew.double().sum(0).cpu()
    assert torch.equal(per_b['episode_return'], now) and not torch.equal(per_a['episode_return'], per_b['episode_return'])
    assert mean_b['episode_return'] == float(now.mean())
    with pytest.raises(L.MpgError, match='mpg_eval_metrics: env kind 2 has no evaluation metrics'):
        ops.eval_metrics(2, *ops.model_rollout(pw.cfg, pw.net('policy'), obs0, 2)[:3])


def test_gap_to_env(engine):
    """the same record twice: zeros.  PathTracking: the model's delta_y moves by its noise mean of +0.5 per step beside the env's, from
    the first step on; every column and the reward differ, all finite.  The pendulum: finite."""
    from mpg_amd.evaluator import ModelEvaluator
    ev = model_evaluator('MPG-v2', M.PT, fixed_steps=30, num_eval_agent=5)
    pw = ev.policy_with_value
    obs0 = dev(start_rows(np.random.Generator(np.random.PCG64(5800)), M.PT, 0, 5))
    rec = ops.model_rollout(pw.cfg, pw.net('policy'), obs0, 30)[:3]
    same = ModelEvaluator.gap_of_records(rec, rec)
    assert not same['obs_gap'].any() and not same['rew_gap'].any() and same['env_return'] == same['model_return']
    gap = ev.gap_to_env(obs0)
    print('   PathTracking gap, steps 0 .. 3, columns [v_x, v_y, r, delta_y, delta_phi, x]:\n%s\n   reward gap %s   returns env %.4f model %.4f'
          % (gap['obs_gap'][:4].numpy(), gap['rew_gap'][:4].numpy(), gap['env_return'], gap['model_return']))
    assert gap['obs_gap'].shape == (30, 6) and gap['rew_gap'].shape == (30,)
    assert torch.isfinite(gap['obs_gap']).all() and torch.isfinite(gap['rew_gap']).all()
    assert not gap['obs_gap'][0].any(), 'both records start from the same observations'
    assert 0.3 < float(gap['obs_gap'][1, 3]) < 0.7, gap['obs_gap'][1]
    assert (gap['obs_gap'][1:].sum(0) > 0).all() and float(gap['rew_gap'].sum()) > 0
    assert np.isfinite(gap['env_return']) and np.isfinite(gap['model_return']) and gap['env_return'] != gap['model_return']
    pd = model_evaluator('MPG-v2', M.PD, fixed_steps=30, num_eval_agent=5)
    g2 = pd.gap_to_env()
    assert g2['obs_gap'].shape == (30, 4) and torch.isfinite(g2['obs_gap']).all() and float(g2['obs_gap'][1:, 0].sum()) > 0
