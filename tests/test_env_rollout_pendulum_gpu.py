"""mpg_env_rollout_pendulum and mpg_nstep_targets_clipped on the GPU.

The one-launch real-env rollout against the chain of stand-alone launches it replaces (mpg_env_reset_from_obs, then per step
mpg_policy_action from the second step on and mpg_env_step), from identical inputs, bit for bit - rewards, last observations and the
status word - for both weight forms (packed image and strided) and both engines; at the env's edges (angles all round, |p| > 2 where
`done` would be true and nothing resets, |act0| > 3, a policy that saturates the range, a NaN start row); repeated launches; and
against the fixture of the unmodified reference (tests/golden/make_golden_mpg_pendulum.py; the env there is the documented closed-form
stand-in).  The clipped n-step target teacher-forced on the fixture's rewards and last observations against the
fixture's targets; against mpg_nstep_targets with bounds that clip nothing; a NaN bootstrap value.  Floats are compared as their
32-bit patterns where bit-identity is the claim."""
import ctypes

import numpy as np
import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops
from tests import mpg_pendulum_oracle as P
from tests import yardstick as Y

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KIND, OD = 1, 4              # MPG_ENV_INVERTED_PENDULUM, its observation width


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(params=['split', 'f32'])
def engine(request):
    """both builds of the library (mpg_amd/_lib.py ENGINES): the split-fp16 product and the exact-fp32 engine"""
    with L.engine(request.param):
        yield request.param


def start_rows(rng, rows):
    """start states from what the replay holds (|p| < 2, |theta| <= 0.2, modest velocities) and replay actions 3 tanh(.) plus the
    worker's 0.1 noise"""
    obs = rng.uniform(-1, 1, (rows, 4)) * np.array([1.9, 0.2, 1.0, 1.0])
    act = 3. * np.tanh(1.5 * rng.standard_normal((rows, 1))) + 0.1 * rng.standard_normal((rows, 1))
    return obs.astype(np.float32), act.astype(np.float32)


def chain(cfg, pol, obs0, act0, n):
    """the sequence mpg_env_rollout_pendulum replaces, through the existing entry points"""
    rows = obs0.shape[0]
    state = torch.zeros(8, rows, device=DEV)
    obs = torch.empty(rows, OD, device=DEV)
    act = torch.empty(rows, 1, device=DEV)
    rew = torch.empty(n, rows, device=DEV)
    done, done_i = torch.empty(rows, dtype=torch.uint8, device=DEV), torch.empty(rows, dtype=torch.uint8, device=DEV)
    L.call('mpg_env_reset_from_obs', L.c_int(KIND), L.c_int(rows), L.c_int(OD), L.ptr(state), L.ptr(obs0), L.stream())
    for t in range(n):
        if t > 0:
            L.call('mpg_policy_action', ctypes.byref(cfg), L.ptr(pol), L.c_int(rows), L.ptr(obs), L.c_float(0.), L.c_u64(0), L.c_u64(0),
                   L.ptr(act), L.stream())
        L.call('mpg_env_step', L.c_int(KIND), L.c_int(rows), L.c_int(OD), L.ptr(state), L.ptr(act0 if t == 0 else act), L.ptr(obs),
               L.ptr(rew[t]), L.ptr(done), L.ptr(done_i), L.stream())
    return rew, obs, done


def both(cache, pol, obs0, act0, n):
    """(chain, one launch, [status of the chain, status of the launch]) on the same inputs"""
    cfg = ops.make_cfg('InvertedPendulumConti-v0')
    pol = dev(pol)
    wc = None
    if cache:                                         # the packed-image instantiation: cfg.wcache[0] -> the policy's images
        wc = ops.WeightCache(pol, [(OD, 2)])
        cfg.wcache[0] = wc.pointer
    obs0, act0 = dev(obs0), dev(act0)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    cfg.status = st.data_ptr()
    ra, oa, done = chain(cfg, pol, obs0, act0, n)
    status = [int(st.item())]
    st.zero_()
    rb, ob = ops.env_rollout_pendulum(cfg, pol, obs0, act0, n)
    torch.cuda.synchronize()
    status.append(int(st.item()))
    del wc
    return (ra, oa), (rb, ob), status, done


def policy_weights(rng, out_gain=1.0, out_bias=0.0):
    from tests.golden_inputs import mlp_weights_flat
    w = mlp_weights_flat(rng, OD, 2)
    w[-(2 * 256 + 2):-2] *= np.float32(out_gain)        # W3
    w[-2:] += np.float32(out_bias)                      # b3
    return w


# ---- 1: bit-identity with the chain -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cache', [False, True], ids=['strided', 'packed'])
@pytest.mark.parametrize('n', [1, 2, 25])
@pytest.mark.parametrize('rows', [1, 15, 16, 17, 40])
def test_rollout_equals_the_per_step_sequence_bit_for_bit(engine, rows, n, cache):
    """rows: one row, a group one short of full, exactly full, one row into a second group, a partial third.  n = 1 runs no policy
    pass, n = 2 the first hand-over through LDS."""
    rng = np.random.Generator(np.random.PCG64(7000 + 10 * rows + n))
    o, a = start_rows(rng, rows)
    (ra, oa), (rb, ob), status, _ = both(cache, policy_weights(rng), o, a, n)
    assert torch.isfinite(ra).all() and torch.isfinite(oa).all()
    assert torch.equal(bits(ra), bits(rb)), 'rewards'
    assert torch.equal(bits(oa), bits(ob)), 'last observations'
    assert status[0] == status[1] == 0, status


def test_rollout_with_more_row_groups_than_one_round_of_workgroups(engine):
    """8330 rows = 521 groups of 16: more than two 512-thread workgroups on each of the 256 compute units hold at once"""
    rng = np.random.Generator(np.random.PCG64(7900))
    o, a = start_rows(rng, 8330)
    (ra, oa), (rb, ob), status, _ = both(True, policy_weights(rng), o, a, 3)
    assert torch.equal(bits(ra), bits(rb)) and torch.equal(bits(oa), bits(ob)) and status[0] == status[1] == 0


# ---- 2: the env's edges -----------------------------------------------------------------------------------------------------------
def edge_rows(rng):
    """40 rows: start angles all round (-pi, pi] (pi itself included), carts beyond |p| = 2 - `done` is true from the first step on and
    the rollout goes on with no reset - and replay actions beyond the control clamp +-3"""
    rows = 40
    o, a = start_rows(rng, rows)
    o[:, 1] = np.linspace(-np.pi, np.pi, rows + 1)[1:].astype(np.float32)
    o[::3, 0] = np.where(np.arange(0, rows, 3) % 2 == 0, 2.5, -3.0)
    a[1::4, 0] = np.where(np.arange(1, rows, 4) % 8 == 1, 4.5, -3.75)
    return o, a


@pytest.mark.parametrize('cache', [False, True], ids=['strided', 'packed'])
def test_rollout_at_large_angles_beyond_the_done_bounds_and_the_control_clamp(engine, cache):
    rng = np.random.Generator(np.random.PCG64(7100))
    o, a = edge_rows(rng)
    assert (np.abs(o[:, 1]) > 0.2).sum() >= 30 and np.float32(np.pi) in o[:, 1] and (np.abs(o[:, 0]) > 2).sum() >= 10
    assert (np.abs(a) > 3).sum() >= 8
    (ra, oa), (rb, ob), status, done = both(cache, policy_weights(rng), o, a, 25)
    assert torch.isfinite(ra).all() and torch.isfinite(oa).all()
    assert int(done.sum().item()) >= 30                 # the chain's own done flags at the last step: these rows were never reset
    assert torch.equal(bits(ra), bits(rb)) and torch.equal(bits(oa), bits(ob))
    assert status[0] == status[1] == 0, status


@pytest.mark.parametrize('cache', [False, True], ids=['strided', 'packed'])
def test_rollout_with_a_policy_that_saturates_the_action_range(engine, cache):
    """output layer x 400: a = 3 tanh(mean) sits at +-3 for most rows at every step"""
    rng = np.random.Generator(np.random.PCG64(7200))
    o, a = start_rows(rng, 40)
    pol = policy_weights(rng, out_gain=400.0)
    cfg = ops.make_cfg('InvertedPendulumConti-v0')
    acts = ops.policy_action(cfg, dev(pol), dev(o))
    assert int((acts.abs() == 3.0).sum().item()) >= 20, acts.abs().min()
    (ra, oa), (rb, ob), status, _ = both(cache, pol, o, a, 25)
    assert torch.isfinite(ra).all()
    assert torch.equal(bits(ra), bits(rb)) and torch.equal(bits(oa), bits(ob))
    assert status[0] == status[1], status


@pytest.mark.parametrize('cache', [False, True], ids=['strided', 'packed'])
def test_rollout_reports_a_nan_start_row_like_the_sequence(engine, cache):
    """one NaN entry in one row of obs0: that row is NaN from the first step on, its observation reaches the policy pass at the second
    step, and both paths OR MPG_STATUS_NAN into the status word; no other row is poisoned and all agree bit for bit.  With n = 1 no
    policy pass runs and neither path reports anything."""
    rows, row = 40, 21
    rng = np.random.Generator(np.random.PCG64(7300))
    o, a = start_rows(rng, rows)
    o[row, 2] = np.nan
    pol = policy_weights(rng)
    (ra, oa), (rb, ob), status, _ = both(cache, pol, o, a, 25)
    assert status[0] == status[1] and status[1] & ops.STATUS_NAN, status
    keep = torch.ones(rows, dtype=torch.bool, device=DEV)
    keep[row] = False
    assert torch.isnan(rb[:, row]).all() and torch.isnan(ra[:, row]).all() and torch.isnan(ob[row]).any()
    assert torch.isfinite(rb[:, keep]).all() and torch.isfinite(ob[keep]).all()
    assert torch.equal(bits(ra[:, keep]), bits(rb[:, keep])) and torch.equal(bits(oa[keep]), bits(ob[keep]))
    _, _, status1, _ = both(cache, pol, o, a, 1)
    assert status1 == [0, 0], status1


# ---- 3: repeated launches -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cache', [False, True], ids=['strided', 'packed'])
def test_three_repeated_launches_give_identical_bits(engine, cache):
    rng = np.random.Generator(np.random.PCG64(7400))
    rows, n = 40, 25
    cfg = ops.make_cfg('InvertedPendulumConti-v0')
    pol = dev(policy_weights(rng))
    wc = None
    if cache:
        wc = ops.WeightCache(pol, [(OD, 2)])
        cfg.wcache[0] = wc.pointer
    o, a = start_rows(rng, rows)
    obs0, act0 = dev(o), dev(a)
    outs = [ops.env_rollout_pendulum(cfg, pol, obs0, act0, n) for _ in range(3)]
    for r, ob in outs[1:]:
        assert torch.equal(bits(r), bits(outs[0][0])) and torch.equal(bits(ob), bits(outs[0][1]))
    assert torch.isfinite(outs[0][0]).all()
    del wc


# ---- 4: against the fixture of the unmodified reference --------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fixture_v1(golden):
    g = P.load(golden, 'MPG-v1')
    w = P.fixture_weights(int(g['weights_seed']), 'MPG-v1')
    return g, w, P.fixture_targets(w, g['target_scale'], g['q_scale'], g['q_shift'])


@pytest.mark.parametrize('cache', [False, True], ids=['strided', 'packed'])
def test_rollout_vs_reference_fixture(fixture_v1, engine, cache):
    """the reference's sample() on the stand-in env: all_rewards and the last observations, float32 and float64 runs, by the rule of
    tests/yardstick.py"""
    g, w, _ = fixture_v1
    cfg = ops.make_cfg('InvertedPendulumConti-v0')
    pol = dev(w['policy'])
    wc = None
    if cache:
        wc = ops.WeightCache(pol, [(OD, 2)])
        cfg.wcache[0] = wc.pointer
    r, last = ops.env_rollout_pendulum(cfg, pol, dev(g['batch_obs']), dev(g['batch_actions']), 25)
    r, last = r.cpu().numpy(), last.cpu().numpy()
    print('rollout vs fixture (%s): rewards %.2e (reference float32 %.2e), last_obs %.2e (reference float32 %.2e)'
          % (engine, Y.rel_l2(r, g['all_rewards_f64']), Y.rel_l2(g['all_rewards'], g['all_rewards_f64']),
             Y.rel_l2(last, g['last_obs_f64']), Y.rel_l2(g['last_obs'], g['last_obs_f64'])))
    Y.check_values(r, g['all_rewards'], g['all_rewards_f64'], what='all_rewards')
    Y.check_values(last, g['last_obs'], g['last_obs_f64'], what='last_obs')
    del wc


# ---- 5: mpg_nstep_targets_clipped ---------------------------------------------------------------------------------------------------
def test_clipped_targets_teacher_forced_on_the_fixture(fixture_v1, engine):
    """on the FIXTURE's rewards and last observations: the fixture's targets by the yard-stick; rows of all three clip regimes are
    present, and in the two clipped ones y - sum_t gamma^t r_t is gamma^n times the bound to float32 rounding"""
    g, w, t = fixture_v1
    cfg = ops.make_cfg('InvertedPendulumConti-v0')
    rew, last = dev(g['all_rewards']), dev(g['last_obs'])
    y = ops.nstep_targets(cfg, dev(t['policy']), dev(t['Q1']), rew, last, clip=ops.PENDULUM_NSTEP_Q_CLIP).cpu().numpy()
    print('clipped targets vs fixture (%s): %.2e (reference float32 %.2e)'
          % (engine, Y.rel_l2(y, g['targets_f64']), Y.rel_l2(g['targets'], g['targets_f64'])))
    Y.check_values(y, g['targets'], g['targets_f64'], what='targets')
    # the regimes, by the fixture's float64 bootstrap values; rows within 0.05 of a bound are left to the yard-stick above
    q = g['q_boot_f64'].astype(np.float64)
    lo, hi = P.Q_LO, P.Q_HI
    below, above, inside = q < lo - 0.05, q > hi + 0.05, (q > lo + 0.05) & (q < hi - 0.05)
    assert below.sum() >= 8 and above.sum() >= 8 and inside.sum() >= 4, (below.sum(), inside.sum(), above.sum())
    n = 25
    gam = np.float64(np.float32(0.98))
    terms = (gam ** np.arange(n))[:, None] * g['all_rewards'].astype(np.float64)
    rest = y.astype(np.float64) - terms.sum(0)
    # float32 rounding: n + 1 additions and n + 1 products of the kernel's sequential sum, each within 2^-24 of the running magnitude,
    # and powf's own error (a few ulp) on each factor
    tol = 8 * (n + 2) * 2.0 ** -24 * (np.abs(terms).sum(0) + 1.0)
    assert (np.abs(rest[below] - gam ** n * lo) <= tol[below]).all(), np.abs(rest[below] - gam ** n * lo).max()
    assert (np.abs(rest[above] - gam ** n * hi) <= tol[above]).all(), np.abs(rest[above] - gam ** n * hi).max()
    assert ((rest[inside] > gam ** n * lo - tol[inside]) & (rest[inside] < gam ** n * hi + tol[inside])).all()
    # without the clip the same inputs give another answer: the plain entry point is what the driver used to call here
    y_plain = ops.nstep_targets(cfg, dev(t['policy']), dev(t['Q1']), rew, last).cpu().numpy()
    assert Y.rel_l2(y_plain, g['targets_f64']) > 1e-3


def test_clipped_targets_with_bounds_that_clip_nothing_equal_the_plain_entry_point(fixture_v1, engine):
    g, w, t = fixture_v1
    cfg = ops.make_cfg('InvertedPendulumConti-v0')
    rew, last = dev(g['all_rewards']), dev(g['last_obs'])
    a = ops.nstep_targets(cfg, dev(t['policy']), dev(t['Q1']), rew, last)
    b = ops.nstep_targets(cfg, dev(t['policy']), dev(t['Q1']), rew, last, clip=(-3.4e38, 3.4e38))
    assert torch.isfinite(a).all() and torch.equal(bits(a), bits(b))


def test_a_nan_bootstrap_value_stays_nan(fixture_v1, engine):
    """TF's minimum / maximum hand a NaN on (fminf / fmaxf would return the bound): a NaN last observation gives a NaN target in
    that row only"""
    g, w, t = fixture_v1
    cfg = ops.make_cfg('InvertedPendulumConti-v0')
    last = g['last_obs'].copy()
    last[5, 1] = np.nan
    y = ops.nstep_targets(cfg, dev(t['policy']), dev(t['Q1']), dev(g['all_rewards']), dev(last), clip=ops.PENDULUM_NSTEP_Q_CLIP)
    keep = torch.ones(64, dtype=torch.bool, device=DEV)
    keep[5] = False
    assert torch.isnan(y[5]) and torch.isfinite(y[keep]).all()
    assert np.isfinite(g['all_rewards'][:, 5]).all()


# ---- 6: the ops wrappers' refusals --------------------------------------------------------------------------------------------------
def test_ops_wrappers_raise_mpg_error(fixture_v1, engine):
    """the wrappers themselves (they take device tensors and the current stream, so they are called here and not in the CPU file): the
    library's refusal comes back as MpgError with its text, and nothing is enqueued - the outputs of a later good call are the same"""
    g, w, t = fixture_v1
    cfg = ops.make_cfg('InvertedPendulumConti-v0')
    pol, obs0, act0 = dev(w['policy']), dev(g['batch_obs']), dev(g['batch_actions'])
    rew, last = dev(g['all_rewards']), dev(g['last_obs'])
    with pytest.raises(L.MpgError, match='mpg_env_rollout_pendulum: n <= 1024'):
        ops.env_rollout_pendulum(cfg, pol, obs0, act0, 1025)
    with pytest.raises(L.MpgError, match='mpg_env_rollout_pendulum: n >= 1'):
        ops.env_rollout_pendulum(cfg, pol, obs0, act0, 0)
    with pytest.raises(L.MpgError, match='mpg_env_rollout_pendulum: pendulum env only'):
        ops.env_rollout_pendulum(ops.make_cfg('PathTracking-v0'), pol, obs0, act0, 25)
    with pytest.raises(L.MpgError, match='mpg_nstep_targets_clipped: empty clip interval'):
        ops.nstep_targets(cfg, dev(t['policy']), dev(t['Q1']), rew, last, clip=(0.5, 0.0))
    with pytest.raises(L.MpgError, match='mpg_nstep_targets_clipped: the clip bounds must be finite'):
        ops.nstep_targets(cfg, dev(t['policy']), dev(t['Q1']), rew, last, clip=(float('-inf'), 0.0))
    with pytest.raises(L.MpgError, match='mpg_nstep_targets_clipped: the clip bounds must be finite'):
        ops.nstep_targets(cfg, dev(t['policy']), dev(t['Q1']), rew, last, clip=(-0.5, float('nan')))
    y = ops.nstep_targets(cfg, dev(t['policy']), dev(t['Q1']), rew, last, clip=ops.PENDULUM_NSTEP_Q_CLIP)
    assert torch.isfinite(y).all()
