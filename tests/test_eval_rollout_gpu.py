"""mpg_eval_rollout, mpg_eval_rollout_pendulum and mpg_eval_metrics on the GPU, and the evaluator that uses them.

The one-launch evaluation rollout against the chain of stand-alone launches it replaces (mpg_env_reset with a seed, then per step
mpg_policy_action without noise and mpg_env_step), from identical inputs, bit for bit - the three trajectories, the final state, the
observations, the done flags and the status word - for both weight forms (packed image and strided), both engines and both envs; with
more workgroups than one resident round; continued from the state an earlier launch left; at the envs' edges (the start states of
tests/env_edge_inputs.py and tests/cart_pole_edge_inputs.py, a policy that saturates the action range, a pendulum that crosses |p| = 2
mid-episode and keeps stepping, a NaN start row); for stochastic stacks; repeated.  mpg_eval_metrics against a float64 restatement of
evaluator.py:160-211 on the launch's own trajectories.  Evaluator with args.one_launch_eval against the method path and against the
reference's fixture.  Floats are compared as their 32-bit patterns where bit-identity is the claim."""
import ctypes

import numpy as np
import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops
from tests import cart_pole_edge_inputs as C
from tests import env_edge_inputs as E
from tests.golden_inputs import mlp_weights_flat

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PT, PEND = 'PathTracking-v0', 'InvertedPendulumConti-v0'
ENVS = [PT, PEND]
KIND = {PT: 0, PEND: 1}
U = 2.0 ** -53               # the unit round-off of float64


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(params=['split', 'f32'])
def engine(request):
    """both builds of the library (mpg_amd/_lib.py ENGINES): the split-fp16 product and the exact-fp32 engine"""
    with L.engine(request.param):
        yield request.param


def policy_weights(rng, cfg, out_gain=1.0):
    w = mlp_weights_flat(rng, cfg.obs_dim, 2 * cfg.act_dim)
    ou = 2 * cfg.act_dim
    w[-(ou * 256 + ou):-ou] *= np.float32(out_gain)     # W3
    return w


def drawn_start(cfg, n, seed, ctr=0):
    """(state [8, n], obs [n, obs_dim]) of mpg_env_reset on every agent"""
    state = torch.zeros(8, n, device=DEV)
    obs = torch.empty(n, cfg.obs_dim, device=DEV)
    L.call('mpg_env_reset', L.c_int(cfg.env_kind), L.c_int(n), L.c_int(cfg.obs_dim), L.ptr(state), L.ptr(None), L.c_u64(seed), L.c_u64(ctr),
           L.ptr(obs), L.stream())
    return state, obs


def start_from_obs(cfg, obs):
    """(state, obs) of mpg_env_reset_from_obs"""
    obs = dev(obs)
    state = torch.zeros(8, obs.shape[0], device=DEV)
    L.call('mpg_env_reset_from_obs', L.c_int(cfg.env_kind), L.c_int(obs.shape[0]), L.c_int(cfg.obs_dim), L.ptr(state), L.ptr(obs), L.stream())
    return state, obs


def chain(cfg, pol, state, obs, steps):
    """the sequence the launch replaces, through the existing entry points, on copies of (state, obs).  Returns what it leaves:
    (obs_traj, act_traj, rew_traj, obs, done, done_intended, state)"""
    n, od, ad = obs.shape[0], cfg.obs_dim, cfg.act_dim
    state, obs = state.clone(), obs.clone()
    obs_t, act_t = torch.empty(steps, n, od, device=DEV), torch.empty(steps, n, ad, device=DEV)
    rew_t = torch.empty(steps, n, device=DEV)
    done, done_i = torch.empty(n, dtype=torch.uint8, device=DEV), torch.empty(n, dtype=torch.uint8, device=DEV)
    for t in range(steps):
        obs_t[t].copy_(obs)
        L.call('mpg_policy_action', ctypes.byref(cfg), L.ptr(pol), L.c_int(n), L.ptr(obs), L.c_float(0.), L.c_u64(0), L.c_u64(0),
               L.ptr(act_t[t]), L.stream())
        L.call('mpg_env_step', L.c_int(cfg.env_kind), L.c_int(n), L.c_int(od), L.ptr(state), L.ptr(act_t[t]), L.ptr(obs), L.ptr(rew_t[t]),
               L.ptr(done), L.ptr(done_i), L.stream())
    return obs_t, act_t, rew_t, obs, done, done_i, state


def launch(cfg, pol, state, obs, steps):
    """the same from ONE launch, in the chain's order of results"""
    state = state.clone()
    before = obs.clone()
    out = ops.eval_rollout(cfg, pol, state, obs, steps)
    assert torch.equal(bits(obs), bits(before)), 'the caller\'s observations are left as they were'
    done_i = out[5] if cfg.env_kind == 0 else out[4]          # (the pendulum's step writes `done` into both flags)
    return out[0], out[1], out[2], out[3], out[4], done_i, state


NAMES = ('obs_traj', 'act_traj', 'rew_traj', 'last obs', 'done', 'done_intended', 'state')


def assert_same(a, b):
    for nm, x, y in zip(NAMES, a, b):
        if x.dtype == torch.uint8:
            assert torch.equal(x, y), nm
        else:
            assert x.shape == y.shape and torch.equal(bits(x), bits(y)), nm


class Case(object):
    """a cfg with its policy on the device, strided or with the packed image, and a status word"""

    def __init__(self, env_id, rng, cache, out_gain=1.0, **cfg_kw):
        self.cfg = ops.make_cfg(env_id, **cfg_kw)
        self.pol = dev(policy_weights(rng, self.cfg, out_gain))
        self.wc = None
        if cache:                                         # the packed-image instantiation: cfg.wcache[0] -> the policy's images
            self.wc = ops.WeightCache(self.pol, [(self.cfg.obs_dim, 2 * self.cfg.act_dim)])
            self.cfg.wcache[0] = self.wc.pointer
        self.st = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.cfg.status = self.st.data_ptr()

    def both(self, state, obs, steps):
        """(chain, launch, [status of the chain, status of the launch])"""
        self.st.zero_()
        a = chain(self.cfg, self.pol, state, obs, steps)
        status = [int(self.st.item())]
        self.st.zero_()
        b = launch(self.cfg, self.pol, state, obs, steps)
        status.append(int(self.st.item()))
        return a, b, status


# ---- 1: bit-identity with the chain -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cache', [False, True], ids=['strided', 'packed'])
@pytest.mark.parametrize('steps', [1, 2, 21, 70])
@pytest.mark.parametrize('n', [1, 5, 15, 16, 17, 40])
@pytest.mark.parametrize('env_id', ENVS)
def test_launch_equals_the_chain_bit_for_bit(engine, env_id, n, steps, cache):
    """n: one agent, the evaluator's five, a group one short of full, exactly full, one agent into a second group, a partial third.
    steps = 1: no hand-over through LDS; 2: the first one."""
    rng = np.random.Generator(np.random.PCG64(9000 + 100 * n + steps))
    c = Case(env_id, rng, cache)
    state, obs = drawn_start(c.cfg, n, seed=77 + n, ctr=steps)
    a, b, status = c.both(state, obs, steps)
    assert all(torch.isfinite(x).all() for x in a[:4])
    assert_same(a, b)
    assert status[0] == status[1] == 0, status
    assert not torch.equal(bits(a[6]), bits(state)), 'the state was advanced'


@pytest.mark.parametrize('cache', [False, True], ids=['strided', 'packed'])
@pytest.mark.parametrize('n', [5, 17])
@pytest.mark.parametrize('obs_dim', [9, 16])
def test_launch_equals_the_chain_with_look_ahead_observations(engine, obs_dim, n, cache):
    rng = np.random.Generator(np.random.PCG64(9100 + obs_dim + n))
    c = Case(PT, rng, cache, obs_dim=obs_dim)
    state, obs = drawn_start(c.cfg, n, seed=5)
    a, b, status = c.both(state, obs, 21)
    assert all(torch.isfinite(x).all() for x in a[:4]) and a[0].shape == (21, n, obs_dim)
    assert_same(a, b)
    assert status[0] == status[1] == 0, status


@pytest.mark.parametrize('env_id', ENVS)
def test_launch_with_more_groups_than_one_round_of_workgroups(engine, env_id):
    """8330 agents = 521 groups of 16: more than two 512-thread workgroups on each of the 256 compute units hold at once"""
    c = Case(env_id, np.random.Generator(np.random.PCG64(9200)), True)
    state, obs = drawn_start(c.cfg, 8330, seed=9)
    a, b, status = c.both(state, obs, 3)
    assert_same(a, b)
    assert status[0] == status[1] == 0, status


# ---- 3: continuity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cache', [False, True], ids=['strided', 'packed'])
@pytest.mark.parametrize('env_id', ENVS)
def test_two_launches_in_a_row_equal_one(engine, env_id, cache):
    """30 steps, then 40 on the state and observations they left = 70 in one launch, in everything"""
    c = Case(env_id, np.random.Generator(np.random.PCG64(9300)), cache)
    state, obs = drawn_start(c.cfg, 17, seed=3)
    whole = launch(c.cfg, c.pol, state, obs, 70)
    first = launch(c.cfg, c.pol, state, obs, 30)
    second = launch(c.cfg, c.pol, first[6], first[3], 40)
    joined = tuple(torch.cat([x, y]) for x, y in zip(first[:3], second[:3])) + second[3:]
    assert_same(whole, joined)
    assert int(c.st.item()) == 0


# ---- 4: the envs' edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cache', [False, True], ids=['strided', 'packed'])
@pytest.mark.parametrize('gain, act', [(1.0, 'tanh'), (8.0, 'tanh'), (8.0, 'linear')], ids=['plain', 'saturated', 'beyond-the-clip'])
def test_path_tracking_edge_states(engine, gain, act, cache):
    """the 146 start rows of tests/env_edge_inputs.py (the v_x clamps, the x and heading wraps, far and negative x, the sincosf branch)
    under the policy; with W3 x 8 the tanh output sits near +-1, and a linear output goes beyond the env's action clip - recorded as the
    policy formed it, clipped by the env for itself"""
    o, _ = E.inputs(0)
    c = Case(PT, np.random.Generator(np.random.PCG64(9400)), cache, out_gain=gain, policy_out_activation=act)
    state, obs = start_from_obs(c.cfg, o)
    a, b, status = c.both(state, obs, E.STEPS)
    assert_same(a, b)
    assert status[0] == status[1], status
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(torch.isfinite(x), torch.isfinite(y))
    assert float(torch.isfinite(a[2]).float().mean()) > 0.5
    if act == 'linear':
        assert int((b[1].abs() > 1).sum().item()) >= 10, 'actions beyond the clip are recorded unclipped'
    if gain > 1 and act == 'tanh':
        assert int((b[1].abs() > 0.99).sum().item()) >= 10


@pytest.mark.parametrize('cache', [False, True], ids=['strided', 'packed'])
@pytest.mark.parametrize('gain', [1.0, 8.0], ids=['plain', 'saturated'])
def test_cart_pole_edge_states(engine, gain, cache):
    """the 130 start rows of tests/cart_pole_edge_inputs.py (angles all round, wound-up and spinning poles, runaway carts, the done
    thresholds) under the policy; with W3 x 8 a = 3 tanh(mean) sits at the control clamp"""
    o, _ = C.inputs()
    c = Case(PEND, np.random.Generator(np.random.PCG64(9500)), cache, out_gain=gain)
    state, obs = start_from_obs(c.cfg, o)
    a, b, status = c.both(state, obs, C.STEPS)
    assert_same(a, b)
    assert status[0] == status[1], status
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(torch.isfinite(x), torch.isfinite(y))
    assert float(torch.isfinite(a[2]).float().mean()) > 0.5
    if gain > 1:
        assert int((b[1].abs() > 2.9).sum().item()) >= 10


@pytest.mark.parametrize('cache', [False, True], ids=['strided', 'packed'])
def test_a_pendulum_that_leaves_the_track_keeps_stepping(engine, cache):
    """carts at |p| = 1.9 moving outwards at 10 m/s are beyond |p| = 2 after their first step (0.04 s), whatever the policy does: the
    motor's 300 N on the 10.5 kg cart alone take 1.2 m/s off per step at the most.  `done` is true from there on, nothing is reset and the episode goes
    on to its last step, as in the chain."""
    n, steps = 20, 6
    o = np.zeros((n, 4), np.float32)
    o[:, 0] = np.where(np.arange(n) % 2 == 0, 1.9, -1.9)
    o[:, 2] = np.where(np.arange(n) % 2 == 0, 10.0, -10.0)
    c = Case(PEND, np.random.Generator(np.random.PCG64(9600)), cache)
    state, obs = start_from_obs(c.cfg, o)
    a, b, status = c.both(state, obs, steps)
    assert_same(a, b)
    p = b[0][:, :, 0].abs()                               # |p| before each step
    assert (p[0] < 2).all() and (p[1:] > 2).all() and torch.isfinite(b[2]).all()
    assert (b[4] == 1).all() and (a[4] == 1).all()
    # no reset: the carts go on outwards from where they were (a redrawn agent would start within 0.01 of the origin)
    assert (p[1:] > p[:-1]).all() and (b[3][:, 0].abs() > p[-1]).all()


# ---- 5: a NaN start row -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cache', [False, True], ids=['strided', 'packed'])
@pytest.mark.parametrize('env_id', ENVS)
def test_a_nan_start_row_is_reported_like_the_chain_and_poisons_no_other_row(engine, env_id, cache):
    n, row, steps = 40, 21, 12
    c = Case(env_id, np.random.Generator(np.random.PCG64(9700)), cache)
    _, clean_obs = drawn_start(c.cfg, n, seed=11)
    o = clean_obs.cpu().numpy().copy()
    clean_state, clean_obs = start_from_obs(c.cfg, o)
    o[row, 2] = np.nan
    state, obs = start_from_obs(c.cfg, o)
    a, b, status = c.both(state, obs, steps)
    assert status[0] == status[1] and status[1] & ops.STATUS_NAN, status
    assert_same(a, b)
    assert torch.isnan(b[2][:, row]).all() and torch.isnan(b[1][:, row]).all()
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[row] = False
    clean = launch(c.cfg, c.pol, clean_state, clean_obs, steps)
    for nm, x, y in zip(NAMES[:3], b[:3], clean[:3]):
        assert torch.isfinite(x[:, keep]).all() and torch.equal(bits(x[:, keep]), bits(y[:, keep])), nm
    assert torch.equal(bits(b[3][keep]), bits(clean[3][keep])) and torch.equal(bits(b[6][:, keep]), bits(clean[6][:, keep]))


# ---- 6: stochastic stacks -----------------------------------------------------------------------------------------------------------
STACKS = [('SAC', PT, {}), ('SAC', PT, dict(squashed_head=True, action_range=1.)), ('SAC', PEND, dict(squashed_head=True))]


@pytest.mark.parametrize('alg, env_id, kw', STACKS, ids=['gaussian-pt', 'squashed-pt', 'squashed-pendulum'])
def test_stochastic_stacks_act_with_their_mode(engine, alg, env_id, kw):
    """the pass reads the mean columns of the 2 * act_dim outputs under the cfg's output rule: compute_mode for the Gaussian head,
    range * tanh(mean) for the squashed one"""
    from mpg_amd.config import default_args
    from mpg_amd.policy import PolicyWithQs
    args = default_args(alg, env_id=env_id, **kw)
    pw = PolicyWithQs(**vars(args))
    assert not pw.deterministic_policy and pw.squashed_head == bool(kw)
    n, steps = 17, 21
    state, obs = drawn_start(pw.cfg, n, seed=13)
    a = chain(pw.cfg, pw.net('policy'), state, obs, steps)
    b = launch(pw.cfg, pw.net('policy'), state, obs, steps)
    assert torch.equal(bits(b[1][0]), bits(pw.compute_mode(obs)))
    assert b[1].shape == (steps, n, pw.act_dim) and torch.isfinite(b[1]).all()
    if kw:
        assert float(b[1].abs().max()) <= float(pw.cfg.action_range)
    assert_same(a, b)
    pw.check_status()


# ---- 7: repeated launches -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('env_id', ENVS)
def test_twenty_launches_from_copies_of_one_state_give_identical_bits(engine, env_id):
    c = Case(env_id, np.random.Generator(np.random.PCG64(9800)), True)
    state, obs = drawn_start(c.cfg, 40, seed=17)
    first = launch(c.cfg, c.pol, state, obs, 30)
    assert all(torch.isfinite(x).all() for x in first[:4])
    for _ in range(19):
        assert_same(first, launch(c.cfg, c.pol, state, obs, 30))


# ---- 8: mpg_eval_metrics against a float64 restatement ------------------------------------------------------------------------------
def running_sum(x):
    """sum over the steps, left to right, for every episode at once: the order in which a python sum() over an episode's list of
    rewards adds them ([T, n] -> [n]; zeros for T = 0)"""
    s = np.zeros(x.shape[1:], np.float64)
    for row in x:
        s = s + row
    return s


def restated_metrics(env_id, obs, act, rew):
    """The evaluation metrics of the reference (evaluator.py:160-211: which columns, which windows, which scales; :153-156: the means
    over the episodes), stated for all episodes at once on float64 copies of the trajectories [T, n, .].  Returns ({key: [n]}, {key:
    mean over the episodes}), keys in the reference's order."""
    obs, act, rew = (np.asarray(x, np.float64) for x in (obs, act, rew))
    T, n = rew.shape
    rms = lambda x: np.sqrt(np.square(x).mean(0))
    m = dict(episode_return=running_sum(rew), episode_len=np.full(n, float(T)))
    if env_id == PT:
        m['delta_y_mse'], m['delta_phi_mse'], m['delta_v_mse'] = rms(obs[:, :, 3]), rms(obs[:, :, 4]), rms(obs[:, :, 0])
        tail = rew[20:]
        with np.errstate(all='ignore'):                    # no step from 20 on: 0 / 0, the mean of nothing
            m['stationary_rew_mean'] = running_sum(tail) / np.float64(tail.shape[0])
        m['steer_mse'] = rms(act[:, :, 0] * 1.2 * np.pi / 9)       # (the reference's order of operations)
        m['acc_mse'] = rms(act[:, :, 1] * 3.)
    else:
        names = ('x', 'theta', 'xdot', 'thetadot')
        for j, nm in enumerate(names):
            m[nm + '_mean'], m[nm + '_var'] = obs[:, :, j].mean(0), obs[:, :, j].var(0)
        for j, nm in enumerate(names):
            m[nm + '_mse'] = rms(obs[:, :, j])
        for j, nm in enumerate(names):
            m[nm + '_mse_25'] = rms(obs[:25, :, j])
    return m, {k: running_sum(v[:, None])[0] / n for k, v in m.items()}


OBS_COLUMN = dict(delta_y=3, delta_phi=4, delta_v=0, x=0, theta=1, xdot=2, thetadot=3)


def metric_scales(env_id, obs, act, rew):
    """what the bar of a metric is relative to, per episode [n]: the mean of |x| for the sums and means, the mean of x^2 for the
    variances, the metric itself for the root mean squares (None here: taken from the reference value)"""
    obs, act, rew = (np.asarray(x, np.float64) for x in (obs, act, rew))
    with np.errstate(all='ignore'):
        s = dict(episode_return=np.abs(rew).mean(0), stationary_rew_mean=np.abs(rew[20:]).mean(0) if rew.shape[0] > 20 else None)
    for nm in ('x', 'theta', 'xdot', 'thetadot'):
        col = obs[:, :, OBS_COLUMN[nm]]
        s[nm + '_mean'], s[nm + '_var'] = np.abs(col).mean(0), np.square(col).mean(0)
    return s


def check_metrics(env_id, steps, per, mean, obs, act, rew, bar=8):
    """|got - ref| <= bar * steps * 2^-53 * scale for every metric of every episode and for the means over the episodes (whose sum over
    n values of one size adds n round-offs of its own)"""
    keys = ops.EVAL_METRIC_KEYS[KIND[env_id]]
    ref_all, ref_mean = restated_metrics(env_id, obs, act, rew)
    assert tuple(ref_all.keys()) == keys
    scales = metric_scales(env_id, obs, act, rew)
    n = rew.shape[1]
    for j, k in enumerate(keys):
        got = np.asarray(per[j], np.float64)
        ref = np.asarray(ref_all[k], np.float64)
        if k == 'episode_len':
            assert (got == steps).all() and (ref == steps).all() and mean[j] == steps
            continue
        if k == 'stationary_rew_mean' and steps <= 20:
            assert np.isnan(got).all() and np.isnan(ref).all() and np.isnan(mean[j]), (k, got)
            continue
        assert np.isfinite(got).all() and np.isfinite(ref).all(), (k, got, ref)
        scale = scales.get(k)
        if scale is None:
            scale = np.abs(ref)                            # the root mean squares: the metric itself
        tol = bar * steps * U * scale
        err = np.abs(got - ref)
        print('%-20s steps %3d n %2d: max err / bar = %.3f' % (k, steps, n, (err / np.maximum(tol, 1e-300)).max()))
        assert (err <= tol).all(), (k, err, tol)
        assert abs(mean[j] - ref_mean[k]) <= tol.mean() + n * U * np.abs(ref).mean(), (k, mean[j], ref_mean[k])


@pytest.mark.parametrize('n', [1, 5, 17])
@pytest.mark.parametrize('steps', [1, 20, 21, 26, 200])
@pytest.mark.parametrize('env_id', ENVS)
def test_metrics_against_the_float64_restatement(engine, env_id, steps, n):
    """both are fed the launch's own recorded trajectory, so they differ in the order of their sums only.  steps: one; the last without
    a stationary step; the first with one; one beyond the 25-step window; the evaluator's own length"""
    c = Case(env_id, np.random.Generator(np.random.PCG64(9900)), True)
    state, obs = drawn_start(c.cfg, n, seed=19)
    obs_t, act_t, rew_t = launch(c.cfg, c.pol, state, obs, steps)[:3]
    per, mean = ops.eval_metrics(c.cfg.env_kind, obs_t, act_t, rew_t)
    K = len(ops.EVAL_METRIC_KEYS[c.cfg.env_kind])
    assert per.shape == (K, n) and mean.shape == (K,) and per.dtype == mean.dtype == torch.float64
    per2, mean2 = ops.eval_metrics(c.cfg.env_kind, obs_t, act_t, rew_t)
    assert torch.equal(per.view(torch.int64), per2.view(torch.int64)) and torch.equal(mean.view(torch.int64), mean2.view(torch.int64))
    check_metrics(env_id, steps, per.cpu().numpy(), mean.cpu().numpy(), obs_t.cpu().numpy(), act_t.cpu().numpy(), rew_t.cpu().numpy())


def test_ops_wrappers_raise_mpg_error(engine):
    """the wrappers themselves: the library's refusal comes back as MpgError with its text and nothing is enqueued"""
    c = Case(PT, np.random.Generator(np.random.PCG64(9950)), False)
    state, obs = drawn_start(c.cfg, 5, seed=1)
    with pytest.raises(L.MpgError, match='mpg_eval_rollout: steps <= 1024'):
        ops.eval_rollout(c.cfg, c.pol, state.clone(), obs, 1025)
    with pytest.raises(L.MpgError, match='mpg_eval_rollout: steps >= 1'):
        ops.eval_rollout(c.cfg, c.pol, state.clone(), obs, 0)
    p = Case(PEND, np.random.Generator(np.random.PCG64(9951)), False)
    pstate, pobs = drawn_start(p.cfg, 5, seed=1)
    with pytest.raises(L.MpgError, match='mpg_eval_rollout_pendulum: steps <= 1024'):
        ops.eval_rollout(p.cfg, p.pol, pstate.clone(), pobs, 1025)
    out = ops.eval_rollout(c.cfg, c.pol, state.clone(), obs, 2)
    with pytest.raises(L.MpgError, match='mpg_eval_metrics: obs_dim 4 on the pendulum'):
        ops.eval_metrics(1, out[0], out[1], out[2])
    with pytest.raises(L.MpgError, match='mpg_eval_metrics: env kind 2 has no evaluation metrics'):
        ops.eval_metrics(2, out[0], out[1], out[2])
    assert torch.isfinite(ops.eval_metrics(0, out[0], out[1], out[2])[1][:5]).all()


# ---- 9: the evaluator ---------------------------------------------------------------------------------------------------------------
def evaluator(alg, one_launch, **kw):
    from mpg_amd.config import default_args
    from mpg_amd.evaluator import Evaluator
    from mpg_amd.policy import PolicyWithQs
    args = default_args(alg, **kw)
    if one_launch is not None:
        args.one_launch_eval = one_launch
    return Evaluator(PolicyWithQs, args.env_id, args)


def test_one_launch_evaluator_vs_reference_fixture(golden, engine):
    """tests/test_learner_gpu.py::test_evaluator_metrics_vs_reference with args.one_launch_eval: the reference's own
    run_n_episodes_parallel / metrics_for_an_episode from the same start states and weights, 200 closed-loop steps, 8 episodes, under
    that test's assertions (allowance per metric: 4x the reference's own float32-vs-float64 gap)"""
    g = golden('evaluator_ref.npz')
    N, T = int(g['N']), int(g['T'])
    ev = evaluator('MPG-v2', True, num_eval_agent=N, fixed_steps=T)
    pw = ev.policy_with_value
    rng = np.random.Generator(np.random.PCG64(0))
    flat = np.concatenate([mlp_weights_flat(rng, 8, 1), mlp_weights_flat(rng, 8, 1), g['w_policy']])
    pw.set_flat(flat)
    per, mean = ev.run_n_episodes_parallel(init_obs=dev(g['init_obs']))
    assert sorted(str(x) for x in g['metric_keys']) == sorted(per.keys()) == sorted(mean.keys())      # (the fixture lists them by name)
    for j, k in enumerate(str(x) for x in g['metric_keys']):
        ref32, ref64 = g['mean'][j], g['mean_f64'][j]
        assert abs(mean[k] - ref64) <= 4 * abs(ref32 - ref64) + 2e-6 * abs(ref64) + 1e-9, (k, mean[k], ref32, ref64)
        e32 = np.abs(g['per_episode'][:, j] - g['per_episode_f64'][:, j]).max()
        got = per[k].cpu().numpy()
        assert (np.abs(got - g['per_episode_f64'][:, j]) <= 4 * e32 + 2e-6 * np.abs(g['per_episode_f64'][:, j]) + 1e-9).all(), k


def loop_trajectories(ev, episodes):
    """what the method path's launches record, through the same calls (env.reset of every agent, ops.policy_action, env.step), on the
    evaluator's env: trajectories [T, episodes * A, .] with episode e's agents at rows e * A .."""
    pw, env = ev.policy_with_value, ev.env
    out = []
    for _ in range(episodes):
        env._initialised = False
        obses = env.reset()
        o, a, r = [], [], []
        for _ in range(ev.fixed_steps):
            act = ops.policy_action(pw.cfg, pw.net('policy'), obses)
            o.append(obses)
            a.append(act)
            obses, rew, _, _ = env.step(act)
            r.append(rew)
        out.append((torch.stack(o), torch.stack(a), torch.stack(r)))
    return tuple(torch.cat([e[j] for e in out], 1) for j in range(3))


def assert_metrics_agree(env_id, steps, per_a, mean_a, per_b, mean_b, traj, bar=8):
    """two evaluations of the same trajectories - the method path's torch ops and the metrics launch - under the bar of the metrics
    test, each against the other; the means over the n episodes under the mean of their bars and the n round-offs of their own sum"""
    obs, act, rew = (x.cpu().numpy() for x in traj)
    scales = metric_scales(env_id, obs, act, rew)
    # (b, the launch: the reference's key_list order; a, the method path, groups the pendulum's metrics by variable, as it did)
    assert list(per_b.keys()) == list(mean_b.keys()) == list(ops.EVAL_METRIC_KEYS[KIND[env_id]])
    assert sorted(per_a.keys()) == sorted(mean_a.keys()) == sorted(per_b.keys())
    for k in per_a:
        a, b = per_a[k].cpu().numpy(), per_b[k].cpu().numpy()
        if k == 'episode_len':
            assert (a == steps).all() and (b == steps).all() and mean_a[k] == mean_b[k] == steps
            continue
        scale = scales.get(k)
        if scale is None:
            scale = np.abs(a)
        tol = bar * steps * U * scale
        assert np.isfinite(a).all() and (np.abs(a - b) <= tol).all(), (k, a, b)
        assert abs(mean_a[k] - mean_b[k]) <= tol.mean() + len(a) * U * np.abs(a).mean(), (k, mean_a[k], mean_b[k])


@pytest.mark.parametrize('alg, kw, steps', [('MPG-v2', dict(num_eval_agent=5), 26), ('NADP', dict(num_eval_agent=3), 30)],
                         ids=['path-tracking', 'pendulum'])
def test_parallel_evaluation_in_one_launch_equals_the_method_path(engine, alg, kw, steps):
    """from the same seed and weights: every per-episode metric within the metrics test's bar, the means, and the env's observations,
    state and done flags afterwards bit for bit.  (steps: beyond the 20-step and 25-step windows; the bar grows with the steps, the
    difference of two orders of summation with their root)"""
    a = evaluator(alg, False, fixed_steps=steps, **kw)
    b = evaluator(alg, True, fixed_steps=steps, **kw)
    twin = evaluator(alg, False, fixed_steps=steps, **kw)
    traj = loop_trajectories(twin, 1)
    per_a, mean_a = a.run_n_episodes_parallel()
    per_b, mean_b = b.run_n_episodes_parallel()
    assert_metrics_agree(a.env_id, steps, per_a, mean_a, per_b, mean_b, traj)
    for x, y in ((a.env.obs, b.env.obs), (a.env._state, b.env._state), (a.env.reward, b.env.reward)):
        assert torch.equal(bits(x), bits(y))
    assert torch.equal(a.env.done, b.env.done) and torch.equal(a.env.done_intended, b.env.done_intended)
    assert a.env._ctr == b.env._ctr == 1
    # the metrics launch on the loop's own trajectories gives the one-launch evaluator's bits: its trajectories are the loop's
    per, _ = ops.eval_metrics(b.env.kind, *traj)
    for j, k in enumerate(ops.EVAL_METRIC_KEYS[b.env.kind]):
        assert torch.equal(per[j].cpu().view(torch.int64), per_b[k].contiguous().view(torch.int64)), k
    # a second evaluation draws new start states on both paths alike
    _, mean_a2 = a.run_n_episodes_parallel()
    _, mean_b2 = b.run_n_episodes_parallel()
    assert mean_a2['episode_return'] != mean_a['episode_return']
    assert mean_a2['episode_return'] == pytest.approx(mean_b2['episode_return'], rel=1e-12)
    assert torch.equal(bits(a.env._state), bits(b.env._state))


def test_five_serial_pendulum_episodes_in_one_launch(engine):
    """run_n_episodes(5) on a one-agent pendulum evaluator (the pendulum parsers' num_eval_agent = 1, num_eval_episode = 5): ONE launch
    over the five drawn states against the method path's five serial episodes"""
    steps, kw = 30, dict(num_eval_agent=1, num_eval_episode=5)
    a = evaluator('NADP', False, fixed_steps=steps, **kw)
    b = evaluator('NADP', True, fixed_steps=steps, **kw)
    twin = evaluator('NADP', False, fixed_steps=steps, **kw)
    per_a, mean_a = a.run_n_episodes(5)
    per_b, mean_b = b.run_n_episodes(5)
    traj = loop_trajectories(twin, 5)
    assert traj[0].shape == (steps, 5, 4) and per_a['episode_return'].shape == per_b['episode_return'].shape == (5,)
    assert_metrics_agree(a.env_id, steps, per_a, mean_a, per_b, mean_b, traj)
    # the trajectories, read back through ops.eval_rollout on the same concatenated start states
    pw = b.policy_with_value
    starts = [drawn_start(pw.cfg, 1, seed=b.env.seed, ctr=e) for e in range(5)]
    state, obs = torch.cat([s for s, _ in starts], 1).contiguous(), torch.cat([o for _, o in starts], 0)
    out = ops.eval_rollout(pw.cfg, pw.net('policy'), state, obs, steps)
    for nm, x, y in zip(NAMES[:3], out[:3], traj):
        assert torch.equal(bits(x), bits(y)), nm
    per, mean = ops.eval_metrics(1, *out[:3])
    for j, k in enumerate(ops.EVAL_METRIC_KEYS[1]):
        assert torch.equal(per[j].cpu().view(torch.int64), per_b[k].contiguous().view(torch.int64)), k
        assert float(mean[j]) == mean_b[k]
    # the draws advance: five different episodes
    ret = per_b['episode_return'].numpy()
    assert len(set(ret.tolist())) == 5, ret
    # the env holds the last episode's state, observation and done flag, as on the method path
    for x, y in ((a.env.obs, b.env.obs), (a.env._state, b.env._state)):
        assert torch.equal(bits(x), bits(y))
    assert torch.equal(a.env.done, b.env.done) and a.env._ctr == b.env._ctr == 5
    assert torch.equal(bits(b.env._state), bits(state[:, 4:5]))
    pw.check_status()


def test_run_evaluation_follows_the_reference_with_the_flag_and_is_unchanged_without(engine):
    """evaluator.py:222-225: one eval agent takes run_n_episodes(num_eval_episode) - with args.one_launch_eval.  Without it
    run_evaluation is run_n_episodes_parallel, as it was."""
    steps, kw = 30, dict(num_eval_agent=1, num_eval_episode=5)
    b, twin = evaluator('NADP', True, fixed_steps=steps, **kw), evaluator('NADP', True, fixed_steps=steps, **kw)
    mean = b.run_evaluation(7)
    per5, mean5 = twin.run_n_episodes(5)
    assert mean == mean5 and b.env._ctr == 5 and b.stats == dict(iteration=7, **mean)
    ret = per5['episode_return'].numpy()
    assert len(set(ret.tolist())) == 5 and mean['episode_return'] == pytest.approx(ret.mean(), rel=1e-14)
    # several agents take the parallel form
    c, ctwin = evaluator('MPG-v2', True, fixed_steps=steps, num_eval_agent=5), evaluator('MPG-v2', True, fixed_steps=steps, num_eval_agent=5)
    assert c.run_evaluation(0) == ctwin.run_n_episodes_parallel()[1] and c.env._ctr == 1
    # without the flag (absent, or False): one parallel episode whatever num_eval_episode says
    for flag in (None, False):
        d, dtwin = evaluator('NADP', flag, fixed_steps=steps, **kw), evaluator('NADP', flag, fixed_steps=steps, **kw)
        assert d.one_launch_eval is False and b.one_launch_eval is True      # (off unless the args ask for it)
        got, want = d.run_evaluation(3), dtwin.run_n_episodes_parallel()[1]
        assert got == want and d.env._ctr == 1 and d.stats == dict(iteration=3, **want)
        assert torch.equal(bits(d.env._state), bits(dtwin.env._state))
        assert got['episode_return'] != mean['episode_return']


def test_more_than_1024_steps_are_refused_by_the_one_launch_evaluator():
    with pytest.raises(ValueError, match='at most 1024 steps'):
        evaluator('MPG-v2', True, fixed_steps=1025)
    ev = evaluator('MPG-v2', True, fixed_steps=1024)
    ev.fixed_steps = 1025
    with pytest.raises(ValueError, match='at most 1024 steps'):
        ev.run_n_episodes_parallel()
    with pytest.raises(ValueError, match='at most 1024 steps'):
        ev.run_n_episodes(2)
    assert evaluator('MPG-v2', False, fixed_steps=1025).fixed_steps == 1025        # the loop takes any length
