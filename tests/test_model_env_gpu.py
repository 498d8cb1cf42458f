"""The model-backed InvertedDoublePendulum-v2 env on the device, both engines (tests/model_env_oracle.py restates it; tests/test_model_env.py
says on the CPU why these comparisons are worth running).

 1. mpg_model_env_reset against the oracle's reset rows under the bar tests/test_env_gpu.py holds the real envs' reset laws to (rtol
    2e-5, atol 2e-5): n in {1, 15, 16, 17, 70}, masks all / none / alternating; unmasked rows and ages bit-identical.
 2. mpg_model_env_step == mpg_model_step in bits on obs_next and rew - the fixture's 25 x 64 rows, 4096 rows next to the seam of the done
    law, a NaN row; done exact against the oracle's done law, truncation and ages.
 3. mpg_model_env_step_store_reset == mpg_model_env_step + mpg_replay_add + mpg_model_env_reset(mask = done), bit for bit.
 4. One launch == the chain of mpg_policy_action + mpg_model_env_step_store_reset, bit for bit, all ten names of tests/rollout_harness.py
    (the ages are its `state`): n in {1, 15, 16, 17, 33} x iters in {1, 2, 25}, sigma 0 and 0.1, packed and strided weights; the ring wrap
    and a 64-bit counter carry; non-zero incoming ages; a NaN row; 20 repeats.  Every iters = 25 case holds a fall and a truncation
    (max_steps 3) inside the launch, asserted on the device's own ring rows.
 5. The launch against the float64 oracle loop under tests/yardstick.check_values.
 6. OffPolicyWorker(args.env_on_model): _sample_loop == one_launch_sample over 3 consecutive samples.
 7. NADP and AMPC stacks (replay_batch_size 64, batch_size 64): 20 optimizer steps with the loop == with the launch, bit for bit, on the
    method path; checkpoint at step 7 and resume == uninterrupted.
 8. Caller-owned outputs of exactly the documented length between sentinels: nothing outside them is written.
Every figure is printed before it is asserted.

Measured on the MI355X (split engine | exact-fp32 engine; only the launch's policy pass touches the network engine):
  reset rows, worst share of the bar |got - ref| / (2e-5 + 2e-5 |ref|) against the float64 oracle     0.0039 | 0.0039 (n = 70)
  seam rows: tip_y within [-4.9e-5, 4.9e-5] of 1; rows at 1 + ulp / 1 / 1 - ulp                       3 / 6 / 0 (both)
  launch against the float64 loop, share of check_values' allowance, act / obs2 / rew                 0.13 / 0.10 / 0.09 | 0.19 / 0.14 / 0.09"""
import ctypes
from functools import partial

import numpy as np
import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops
from tests import model_env_oracle as V
from tests import rollout_harness as H
from tests import yardstick as Y
from tests.rollout_harness import assert_same, bits, engine, ring_ptrs  # noqa: F401 (engine: a fixture)
from tests.test_model_env import FIXTURE, falls_and_truncations, loop_case, run_loop
from tests.test_model_rollout import allowance_used

pytestmark = pytest.mark.gpu
DEV = 'cuda'
OD, AD = V.OD, V.AD
RTOL = ATOL = 2e-5          # tests/test_env_gpu.py: test_env_reset_law_philox_matches_oracle_and_distribution


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def make_cfg():
    return ops.make_cfg(V.ENV_ID)


# ---- 1: the reset law ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 15, 16, 17, 70])
def test_reset_against_the_oracle(engine, n):
    cfg, seed, ctr = make_cfg(), 1234 + 2 ** 33, 2 ** 32 - 1 + n
    ref64, ref32 = V.reset_rows(n, seed, ctr, torch.float64), V.reset_rows(n, seed, ctr)
    before = np.random.Generator(np.random.PCG64(n)).standard_normal((n, OD)).astype(np.float32)
    ages = (np.arange(n) + 3).astype(np.int32)
    for name, mask in (('all', None), ('all by mask', np.ones(n, np.uint8)), ('none', np.zeros(n, np.uint8)),
                       ('alternating', (np.arange(n) % 2).astype(np.uint8)), ('any non-zero byte', ((np.arange(n) % 3 == 0) * 0x80).astype(np.uint8))):
        obs, age = dev(before), dev(ages, torch.int32)
        ops.model_env_reset(cfg, obs, age, seed, ctr, None if mask is None else dev(mask, torch.uint8))
        got, got_age = obs.cpu().numpy(), age.cpu().numpy()
        m = np.ones(n, bool) if mask is None else mask.astype(bool)
        assert np.array_equal(got[~m].view(np.int32), before[~m].view(np.int32)) and np.array_equal(got_age[~m], ages[~m]), name
        assert not got_age[m].any() and not got[m][:, 8:].any(), name
        if m.any():
            share = np.abs(got[m] - ref64[m]) / (ATOL + RTOL * np.abs(ref64[m]))
            print('   n %d, mask %-18s worst share of the bar vs float64 %.4f, vs the float32 restatement %.2e absolute'
                  % (n, name, share.max(), np.abs(got[m] - ref32[m]).max()))
            np.testing.assert_allclose(got[m], ref64[m], rtol=RTOL, atol=ATOL)
            np.testing.assert_allclose(got[m], ref32[m], rtol=RTOL, atol=ATOL)


def test_env_object_resets_and_steps(engine):
    """InvertedDoublePendulumModelEnv: the first reset() draws every agent, later ones the done agents; step() advances the ages"""
    from mpg_amd.envs import make_model_env
    env = make_model_env(V.ENV_ID, num_agent=33, seed=5, max_episode_steps=2)
    o0 = env.reset()
    np.testing.assert_allclose(o0.cpu().numpy(), V.reset_rows(33, 5, 0, torch.float64), rtol=RTOL, atol=ATOL)
    assert env._ctr == 1 and not env._state.any()
    o1, r1, d1, _ = env.step(torch.zeros(33, 1, device=DEV))
    ref = V.step(o0.cpu().numpy(), np.zeros((33, 1), np.float32), np.zeros(33, np.int32), 2, torch.float64)
    np.testing.assert_allclose(o1.cpu().numpy(), ref[0], rtol=1e-5, atol=1e-6)
    assert not d1.any() and (env._state == 1).all() and o1 is not o0
    assert torch.equal(bits(env.reset()), bits(o1)) and env._ctr == 2                 # nobody done: nobody re-drawn
    _, _, d2, _ = env.step(torch.zeros(33, 1, device=DEV))
    assert d2.all() and (env._state == 2).all()                                        # truncated at age + 1 == 2
    o3 = env.reset()
    np.testing.assert_allclose(o3.cpu().numpy(), V.reset_rows(33, 5, 2, torch.float64), rtol=RTOL, atol=ATOL)
    assert not env._state.any()
    given = dev(V.leaning_rows(33, 0.3))
    assert env.reset(init_obs=given) is not None and torch.equal(env.obs, given) and not env._state.any()


# ---- 2: the step --------------------------------------------------------------------------------------------------------------------
def step_rows(golden):
    """(obs, act, age): the fixture's rows before each of its 25 steps with its actions, the seam rows at rest, a NaN row"""
    g = golden(FIXTURE)
    fix_obs = np.concatenate([g['obs0'][None], g['obs'][:-1]]).reshape(-1, OD)
    fix_act = g['actions'].reshape(-1, AD)
    seam = V.seam_rows()
    nan = V.leaning_rows(1, 0.1)
    nan[0, 6] = np.nan
    obs = np.concatenate([fix_obs, seam, nan]).astype(np.float32)
    act = np.concatenate([fix_act, np.zeros((seam.shape[0] + 1, AD), np.float32)])
    return g, obs, act, fix_obs.shape[0], seam.shape[0]


def test_step_equals_model_step_and_done_is_exact(golden, engine):
    g, obs, act, n_fix, n_seam = step_rows(golden)
    cfg, n = make_cfg(), obs.shape[0]
    ages = (np.arange(n) % 5).astype(np.int32)
    age = dev(ages, torch.int32)
    o, r = ops.model_step(cfg, dev(obs), dev(act))
    o2, r2, done = ops.model_env_step(cfg, dev(obs), dev(act), age, max_steps=4)
    assert torch.equal(bits(o), bits(o2)) and torch.equal(bits(r), bits(r2))
    assert torch.equal(age.cpu(), torch.as_tensor(ages + 1))
    on, done = o2.cpu().numpy(), done.cpu().numpy()
    assert set(np.unique(done)) == {0, 1}
    # the done law on the device's own new rows, exactly: float32 products and sum, the negated comparison, the truncation
    fell = V.fell(on)
    assert np.array_equal(done.astype(bool), fell | V.truncated(ages, 4))
    assert fell[-1] and np.isnan(on[-1, :8]).all() and np.isnan(r2.cpu().numpy()[-1])
    # without a limit done is the fall alone
    _, _, d0 = ops.model_env_step(cfg, dev(obs), dev(act), dev(ages, torch.int32), max_steps=0)
    assert np.array_equal(d0.cpu().numpy().astype(bool), fell)
    # the fixture's rows: the fall the float64 chain of the unmodified reference shows, wherever it is not within 1e-5 of the seam
    ty64 = np.stack([V.tip_y(x, torch.float64) for x in g['obs_f64']]).reshape(-1)
    clear = np.abs(ty64 - 1.) > 1e-5
    print('   fixture rows: %d of %d clear of the seam by 1e-5, %d of them fallen' % (clear.sum(), n_fix, (~(ty64 > 1.))[clear].sum()))
    assert clear.sum() >= n_fix - 4 and np.array_equal(fell[:n_fix][clear], ~(ty64 > 1.)[clear])
    # the seam rows: the device's tip heights reach the float32 values next to 1 on both sides
    ty = V.tip_y(on[n_fix:n_fix + n_seam])
    one = np.float32(1.)
    ulp = np.float32(2. ** -23)
    at = [int((ty == v).sum()) for v in (np.nextafter(one, np.float32(2.)), one, np.nextafter(one, np.float32(0.)))]
    print('   seam rows: tip_y in [%.3g, %.3g] around 1; rows at 1 + ulp / 1 / 1 - ulp: %s' % (ty.min() - 1., ty.max() - 1., at))
    assert ((ty > one) & (ty <= one + 4 * ulp)).any() and ((ty <= one) & (ty >= one - 4 * ulp)).any()
    assert 0 < fell[n_fix:n_fix + n_seam].sum() < n_seam


# ---- 3: the composition -------------------------------------------------------------------------------------------------------------
def mixed_rows(n, seed=1):
    """every third row leaning beyond the seam (falls at this step), the others leaning at 0.55 +- 0.02; entries 8 .. 10 not zero, as
    an env's start observation may hold them"""
    rng = np.random.Generator(np.random.PCG64(seed))
    obs = V.leaning_rows(n, 0.55, rng, 0.02)
    obs[::3] = V.leaning_rows(n, 0.62, rng, 0.01)[::3]
    obs[:, 5:8] = 0.1 * rng.standard_normal((n, 3)).astype(np.float32)
    obs[:, 8:] = rng.standard_normal((n, 3)).astype(np.float32)
    return obs


def fresh(n, cap, obs, ages, nan_row=None):
    """one side's buffers in tests/rollout_harness.py's names (state: the ages), rings full of a sentinel"""
    obs = np.array(obs, np.float32)
    if nan_row is not None:
        obs[nan_row, :8] = np.nan
    f = dict(dtype=torch.float32, device=DEV)
    u8 = dict(dtype=torch.uint8, device=DEV)
    return dict(state=dev(ages, torch.int32), obs_io=dev(obs), act_out=torch.full((n, AD), -7., **f), done_out=torch.full((n,), 0xAB, **u8),
                ring_obs=torch.full((cap, OD), -7., **f), ring_act=torch.full((cap, AD), -7., **f), ring_rew=torch.full((cap,), -7., **f),
                ring_obs2=torch.full((cap, OD), -7., **f), ring_done=torch.full((cap,), 0xAB, **u8))


@pytest.mark.parametrize('n,cap,nxt', [(1, 1, 0), (17, 40, 30), (70, 70, 69), (70, 300, 5)])
def test_step_store_reset_equals_its_three_calls(engine, n, cap, nxt):
    cfg = make_cfg()
    obs, ages = mixed_rows(n), (np.arange(n) % 4).astype(np.int32)
    act = dev(np.random.Generator(np.random.PCG64(2)).uniform(-1, 1, (n, AD)))
    a, b = fresh(n, cap, obs, ages), fresh(n, cap, obs, ages)
    seed, ctr, max_steps = 4 + 2 ** 40, 2 ** 32 - 1, 3
    # the three calls
    o2, rew, done = ops.model_env_step(cfg, a['obs_io'], act, a['state'], max_steps)
    L.call('mpg_replay_add', L.c_int(cap), L.c_int(nxt), L.c_int(n), L.c_int(OD), L.c_int(AD), L.ptr(a['obs_io']), L.ptr(act), L.ptr(rew),
           L.ptr(o2), L.ptr(done), *ring_ptrs(a), L.stream())
    ops.model_env_reset(cfg, o2, a['state'], seed, ctr, done)
    a['obs_io'], a['done_out'] = o2, done
    # the one
    ops.model_env_step_store_reset(cfg, b['obs_io'], act, b['state'], max_steps, [b[k] for k in H.RING], cap, nxt, seed, ctr, b['done_out'])
    torch.cuda.synchronize()
    names = tuple(k for k in H.NAMES if k not in ('act_out', 'status'))
    assert_same(a, b, (n, cap, nxt), names)
    d = b['done_out'].cpu().numpy()
    assert set(np.unique(d)) <= {0, 1} and d[::3].all() and (n < 3 or not d.all())
    assert not b['state'][b['done_out'] == 1].any() and (b['state'][b['done_out'] == 0].cpu().numpy() == ages[d == 0] + 1).all()
    w = H.touched(cap, nxt, n)
    assert (b['ring_rew'][~w] == -7.).all() and (b['ring_done'][~w] == 0xAB).all()
    slot0 = nxt % cap
    assert torch.equal(bits(b['ring_obs'][slot0]), bits(dev(obs[0]))), 'the row before the step, entries 8 .. 10 as they stood'
    assert not b['ring_obs2'][w][:, 8:].any() and not b['obs_io'][:, 8:].any()
    # done_out is nullable
    c = fresh(n, cap, obs, ages)
    ops.model_env_step_store_reset(cfg, c['obs_io'], act, c['state'], max_steps, [c[k] for k in H.RING], cap, nxt, seed, ctr, None)
    assert_same(b, c, 'no done_out', tuple(k for k in names if k != 'done_out'))


# ---- 4: one launch == the chain ---------------------------------------------------------------------------------------------------
NSEED, ESEED = 11, 4


def Policy(packed, seed=77):
    """the double pendulum's policy network (11 inputs, mean | log-std) under a linear output with action_range 1: a = tanh(mean).
    seed 77: the weights of tests/test_model_env.loop_case"""
    return H.PolicyNet(OD, 2, make_cfg(), packed, seed)


def run_chain(p, max_steps, sigma, t, n, iters, cap, nxt, nctr, ectr):
    p.status.zero_()
    for it in range(iters):
        L.call('mpg_policy_action', ctypes.byref(p.cfg), L.ptr(p.pol), L.c_int(n), L.ptr(t['obs_io']), L.c_float(sigma), L.c_u64(NSEED),
               L.c_u64(nctr + it), L.ptr(t['act_out']), L.stream())
        L.call('mpg_model_env_step_store_reset', ctypes.byref(p.cfg), L.c_int(n), L.ptr(t['obs_io']), L.ptr(t['act_out']), L.c_int(max_steps),
               L.ptr(t['state']), L.c_int(cap), L.c_int((nxt + it * n) % cap), *ring_ptrs(t), L.c_u64(ESEED), L.c_u64(ectr + it),
               L.ptr(t['done_out']), L.stream())
    t['status'] = p.status.clone()


def run_launch(p, max_steps, sigma, t, n, iters, cap, nxt, nctr, ectr):
    p.status.zero_()
    L.call('mpg_worker_rollout_model', ctypes.byref(p.cfg), L.ptr(p.pol), L.c_int(n), L.c_int(iters), L.ptr(t['obs_io']), L.ptr(t['state']),
           L.c_int(max_steps), L.c_float(sigma), L.c_u64(NSEED), L.c_u64(nctr), L.ptr(t['act_out']), L.c_int(cap), L.c_int(nxt), *ring_ptrs(t),
           L.c_u64(ESEED), L.c_u64(ectr), L.ptr(t['done_out']), L.stream())
    t['status'] = p.status.clone()


def both(p, n, iters, sigma, obs, ages, max_steps=3, nan_row=None, **where):
    """-> (chain, launch)"""
    runs = (partial(run_chain, p, max_steps, sigma), partial(run_launch, p, max_steps, sigma))
    return H.both(runs, lambda n_, cap: fresh(n_, cap, obs, ages, nan_row), n, iters, **where)


def device_record(t, n, iters, nxt=5):
    """the launch's ring rows in iteration order, as the oracle's sample_loop returns them"""
    cap = t['ring_rew'].shape[0]
    idx = (nxt + torch.arange(iters * n, device=DEV)) % cap
    return {k: t['ring_' + k][idx].view(iters, n, *t['ring_' + k].shape[1:]).cpu().numpy() for k in ('obs', 'act', 'rew', 'obs2', 'done')}


@pytest.mark.parametrize('sigma', [0., 0.1], ids=['no_noise', 'sigma_0.1'])
@pytest.mark.parametrize('packed', [False, True], ids=['strided', 'packed'])
def test_one_launch_equals_the_chain_bit_for_bit(engine, packed, sigma):
    """n: one agent (the reference-shaped default), a group short of one lane, a full group, one agent into a second group, one into a
    third.  iters = 1 is a single pair, 2 the first hand-over of the rows through LDS, 25 holds falls and truncations (max_steps 3;
    the start rows and ages of tests/test_model_env.loop_case, for which the oracle shows both)."""
    p = Policy(packed)
    for n in (1, 15, 16, 17, 33):
        c = loop_case(n, sigma)
        assert np.array_equal(p.pol.cpu().numpy(), c['wp'])
        for iters in (1, 2, 25):
            a, b = both(p, n, iters, sigma, c['obs'], c['age'], c['max_steps'], ctr=c['noise_ctr'], ectr=c['env_ctr'])
            assert_same(a, b, (n, iters, sigma))
            assert int(b['status'].item()) == 0
            w = H.touched(iters * n + 13, 5, iters * n)
            assert (b['ring_rew'][~w] == -7.).all() and (b['ring_rew'][w] != -7.).all()
            assert (b['ring_done'][~w] == 0xAB).all() and (b['ring_done'][w] <= 1).all()
            assert torch.isfinite(b['ring_obs2'][w]).all() and (b['state'] >= 0).all() and (b['state'] < 3).all()
            if iters == 25:
                falls, truncs, _ = falls_and_truncations(device_record(b, n, iters), 3)
                assert falls >= 1 and truncs >= 1, (n, falls, truncs)


@pytest.mark.parametrize('packed', [True, False], ids=['packed', 'strided'])
def test_ring_wrap_counter_carry_and_incoming_ages(engine, packed):
    """capacity == iters * n with next_idx = capacity - 3: every slot is written once and the wrap falls inside an iteration's block;
    noise_ctr = env_ctr = 2^32 - 2: the counters' low words overflow at the third iteration; incoming ages up to max_steps + 2 (an
    agent beyond the limit is truncated at its next step)."""
    p = Policy(packed, seed=78)
    max_steps = 6
    for n, iters in ((1, 25), (15, 5), (33, 25)):
        cap = iters * n
        obs, ages = mixed_rows(n, seed=3), (np.arange(n) % (max_steps + 3)).astype(np.int32)
        a, b = both(p, n, iters, 0.1, obs, ages, max_steps, cap=cap, nxt=cap - 3 if cap > 3 else 0, ctr=2 ** 32 - 2, ectr=2 ** 32 - 2)
        assert_same(a, b, (n, iters))
        assert (b['ring_rew'] != -7.).all() and (b['ring_done'] <= 1).all()
        rec = device_record(b, n, iters, nxt=cap - 3 if cap > 3 else 0)
        assert (rec['done'][0][ages + 1 >= max_steps] == 1).all()
    # the high words matter: the same start and the same low words under another high word draw other noise and - with episodes of one
    # step every agent is re-drawn at every iteration - other reset rows
    n, iters, cap = 16, 5, 5 * 16 + 13
    obs, ages = mixed_rows(n, seed=3), np.zeros(n, np.int32)
    lo, hi = fresh(n, cap, obs, ages), fresh(n, cap, obs, ages)
    run_launch(p, 1, 0.1, lo, n, iters, cap, 5, 2 ** 32 - 2, 2 ** 32 - 2)
    run_launch(p, 1, 0.1, hi, n, iters, cap, 5, 2 ** 33 - 2, 2 ** 33 - 2)
    torch.cuda.synchronize()
    assert not torch.equal(bits(lo['ring_act'][5:5 + n]), bits(hi['ring_act'][5:5 + n]))
    assert (lo['ring_done'][5:5 + iters * n] == 1).all() and (hi['ring_done'][5:5 + iters * n] == 1).all()
    first_reset = slice(5 + n, 5 + 2 * n)                     # iteration 1's rows: the reset rows keyed by iteration 0's counter
    assert not (bits(lo['ring_obs'][first_reset]) == bits(hi['ring_obs'][first_reset]))[:, :8].any()
    np.testing.assert_allclose(lo['ring_obs'][first_reset].cpu().numpy(), V.reset_rows(n, ESEED, 2 ** 32 - 2, torch.float64), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(hi['ring_obs'][first_reset].cpu().numpy(), V.reset_rows(n, ESEED, 2 ** 33 - 2, torch.float64), rtol=RTOL, atol=ATOL)
    third = slice(5 + 3 * n, 5 + 4 * n)                        # iteration 3's rows: keyed by iteration 2's counter, 2^32 - 2 + 2 = 2^32
    np.testing.assert_allclose(lo['ring_obs'][third].cpu().numpy(), V.reset_rows(n, ESEED, 2 ** 32, torch.float64), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize('packed', [False, True], ids=['strided', 'packed'])
def test_a_nan_row_is_reported_stored_and_redrawn_like_the_chain(engine, packed):
    """one agent's row NaN from the start: the policy pass sees it, its action and transition are NaN, both paths OR MPG_STATUS_NAN into
    the status word, and everything - the NaN entries' bit patterns included - is equal.  A NaN row is done (the negated comparison),
    so the agent is re-drawn and every other row is finite."""
    p = Policy(packed, seed=79)
    n, iters, row = 33, 5, 21
    c = loop_case(n)
    a, b = both(p, n, iters, 0.1, c['obs'], c['age'], 0, nan_row=row)
    assert_same(a, b, 'nan row')
    assert int(a['status'].item()) == int(b['status'].item()) and int(b['status'].item()) & ops.STATUS_NAN
    slot = 5 + row                                         # the row's transition of iteration 0
    assert torch.isnan(b['ring_obs'][slot][:8]).all() and torch.isnan(b['ring_act'][slot]).all() and torch.isnan(b['ring_rew'][slot])
    assert torch.isnan(b['ring_obs2'][slot][:8]).all() and int(b['ring_done'][slot]) == 1
    keep = ~H.touched(iters * n + 13, slot, 1)
    for k in ('ring_obs', 'ring_act', 'ring_rew', 'ring_obs2'):
        assert torch.isfinite(b[k][keep]).all(), k
    assert torch.isfinite(b['obs_io']).all() and torch.isfinite(b['act_out']).all()
    nxt = b['ring_obs'][5 + n + row].cpu().numpy()          # iteration 1's row of that agent: its reset row, keyed by iteration 0's counter
    np.testing.assert_allclose(nxt, V.reset_rows(n, ESEED, 3, torch.float64)[row], rtol=RTOL, atol=ATOL)


def test_twenty_launches_give_identical_bits(engine):
    p = Policy(True, seed=80)
    n, iters, cap = 33, 25, 33 * 25 + 13
    c = loop_case(n)
    H.assert_repeatable(lambda: fresh(n, cap, c['obs'], c['age']), lambda t: run_launch(p, 3, 0.1, t, n, iters, cap, 5, 7, 3), 20)


def test_ops_worker_rollout_takes_the_model_entry(engine):
    """ops.worker_rollout on an env_kind 2 cfg == the ctypes call above; the library's refusals reach Python as MpgError"""
    p = Policy(True)
    n, iters, cap = 17, 4, 17 * 4 + 13
    c = loop_case(n)
    a, b = fresh(n, cap, c['obs'], c['age']), fresh(n, cap, c['obs'], c['age'])
    run_launch(p, 3, 0.1, a, n, iters, cap, 5, 7, 3)
    b['act_out'] = ops.worker_rollout(p.cfg, p.pol, iters, b['state'], b['obs_io'], 0.1, NSEED, 7, [b[k] for k in H.RING], cap, 5, ESEED, 3,
                                      done_out=b['done_out'], max_steps=3)
    b['status'] = p.status.clone()
    torch.cuda.synchronize()
    assert_same(a, b, 'ops.worker_rollout')
    with pytest.raises(L.MpgError, match='mpg_worker_rollout_model: iters <= 1024'):
        ops.worker_rollout(p.cfg, p.pol, 1025, b['state'], b['obs_io'], 0., 0, 0, [b[k] for k in H.RING], cap, 5, 0, 0)
    with pytest.raises(L.MpgError, match='mpg_worker_rollout_model: iters \\* n = 85 transitions do not fit'):
        ops.worker_rollout(p.cfg, p.pol, 5, b['state'], b['obs_io'], 0., 0, 0, [b[k] for k in H.RING], cap - 1 - 12, 5, 0, 0)


# ---- 5: the launch against the float64 oracle loop ----------------------------------------------------------------------------------
@pytest.mark.parametrize('sigma', [0., 0.1], ids=['no_noise', 'sigma_0.1'])
def test_launch_against_the_float64_oracle_loop(engine, sigma):
    n = 33
    c = loop_case(n, sigma)
    ref64, ref32 = run_loop(c, torch.float64), run_loop(c, torch.float32)
    p = Policy(True)
    cap = c['iters'] * n + 13
    t = fresh(n, cap, c['obs'], c['age'])
    run_launch(p, c['max_steps'], sigma, t, n, c['iters'], cap, 5, c['noise_ctr'], c['env_ctr'])
    torch.cuda.synchronize()
    got = device_record(t, n, c['iters'])
    for k in ('obs', 'act', 'rew', 'obs2'):
        print('   %-5s vs float64 %.2e (float32 oracle %.2e)  vs float32 %.2e  uses %.3f of its allowance (%s, sigma %g)'
              % (k, Y.rel_l2(got[k], ref64[k]), Y.rel_l2(ref32[k], ref64[k]), Y.rel_l2(got[k], ref32[k]),
                 allowance_used(got[k], ref32[k], ref64[k]), engine, sigma))
    assert int(t['status'].item()) == 0
    assert np.array_equal(got['done'], ref64['done']) and np.array_equal(t['state'].cpu().numpy(), ref64['age_io'])
    for k in ('obs', 'obs2', 'rew'):
        Y.check_values(got[k], ref32[k], ref64[k], k)
    Y.check_values(t['obs_io'].cpu().numpy(), ref32['obs_io'], ref64['obs_io'], 'obs_io')


# ---- 6: OffPolicyWorker -------------------------------------------------------------------------------------------------------------
def model_args(alg='NADP', **more):
    from mpg_amd.config import default_args
    return default_args(alg, env_id=V.ENV_ID, env_on_model=True, **more)


@pytest.mark.parametrize('sigma', [None, 0.1], ids=['no_noise', 'sigma_0.1'])
@pytest.mark.parametrize('num_agent', [1, 8])
def test_worker_sample_one_launch_equals_the_loop(engine, num_agent, sigma):
    """three consecutive samples of 64 / num_agent iterations each, episodes of at most 20 steps: the second and third continue from
    the ages, rows and counters the one before left"""
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    out = []
    for one in (False, True):
        args = model_args(num_agent=num_agent, batch_size=64, explore_sigma=sigma, seed=5, init_seed=5, max_episode_steps=20,
                          **(dict(one_launch_sample=True) if one else {}))
        w = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
        assert w.env.kind == 2 and w.env.max_episode_steps == 20 and type(w.env).__name__ == 'InvertedDoublePendulumModelEnv'
        batches = [w.sample() for _ in range(3)]
        torch.cuda.synchronize()
        out.append((w, batches, (w._noise_ctr, w.env._ctr, w.num_sample, w.sample_times)))
    (wa, ba, ca), (wb, bb, cb) = out
    assert ca == cb == (3 * 64 // num_agent, 3 * 64 // num_agent + 1, 192, 3), (ca, cb)
    for x, y in zip(ba, bb):
        assert len(x) == len(y) == 5
        for u, v in zip(x, y):
            assert u.shape == v.shape and u.dtype == v.dtype and torch.equal(bits(u), bits(v))
    assert torch.equal(bits(wa.obs), bits(wb.obs)) and torch.equal(bits(wa.env.obs), bits(wb.env.obs))
    assert torch.equal(wa.env._state, wb.env._state) and torch.equal(wa.env.done, wb.env.done)
    done = torch.cat([b[4] for b in bb])
    assert 0 < int(done.sum()) < done.numel()
    assert wb.policy_with_value.check_status() == 0


def test_worker_refusals_on_the_model_env(engine):
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    w = OffPolicyWorker(PolicyWithQs, V.ENV_ID, model_args(num_agent=1, batch_size=2048, one_launch_sample=True), 0)
    with pytest.raises(ValueError, match='one_launch_sample on the model env takes at most 1024 iterations per launch'):
        w.sample()
    with pytest.raises(ValueError, match='_sample_one_launch_pendulum serves InvertedPendulumConti-v0 only .the env is InvertedDoublePendulumModelEnv.'):
        w._sample_one_launch_pendulum(4)
    with pytest.raises(ValueError, match='no device environment for .InvertedDoublePendulum-v2.'):
        from mpg_amd.config import default_args
        OffPolicyWorker(PolicyWithQs, V.ENV_ID, default_args('NADP', env_id=V.ENV_ID), 0)           # without env_on_model: as before


# ---- 7: the stacks ------------------------------------------------------------------------------------------------------------------
SMALL = dict(batch_size=64, replay_batch_size=64, replay_starts=128, max_buffer_size=1024, max_episode_steps=16, nan_check_interval=10 ** 9)


def _stack(alg, one, seed=3, **kw):
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.learners import AMPCLearner, NADPLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    more = dict(num_rollout_list_for_policy_update=[10]) if alg == 'AMPC' else {}
    args = model_args(alg, seed=seed, init_seed=seed, one_launch_sample=one, **dict(SMALL, **more, **kw))
    assert args.num_agent == 1
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    learner = (AMPCLearner if alg == 'AMPC' else NADPLearner)(PolicyWithQs, args)
    opt = SingleProcessOffPolicyOptimizer(worker, learner, ReplayBuffer(args, 0), None, args, sampling_interval=3)
    assert opt._fused is None                  # the model env is sampled on the method path
    return opt


def _state(opt):
    pw, rb, w, ln = opt.worker.policy_with_value, opt.replay_buffer, opt.worker, opt.learner
    torch.cuda.synchronize()
    tensors = [t.clone() for t in (pw.params, pw.m, pw.v, rb.obs, rb.act, rb.rew, rb.obs2, rb.done, w.obs, w.env._state, w.env.done)]
    counters = (dict(pw.opt_steps), rb._next_idx, len(rb), rb.replay_times, w._noise_ctr, w.env._ctr, ln.counter, opt.num_sampled_steps)
    return tensors, counters


def _equal(a, b):
    (ta, ca), (tb, cb) = a, b
    assert ca == cb, (ca, cb)
    for i, (x, y) in enumerate(zip(ta, tb)):
        assert x.shape == y.shape and torch.equal(bits(x), bits(y)), i


@pytest.mark.parametrize('alg', ['NADP', 'AMPC'])
def test_stack_with_the_launch_equals_the_loop_and_resumes_bit_identically(tmp_path, engine, alg):
    """20 optimizer steps (samples of 64 iterations at 0, 3, .. 18 behind the two that fill the buffer to replay_starts) with
    OffPolicyWorker's loop and with the one launch: parameters, Adam moments, ring, worker rows, ages and counters bit for bit; a
    checkpoint written at step 7 of the launch's run and loaded into a stack built with ANOTHER seed ends equal to the uninterrupted
    run."""
    from mpg_amd.checkpoint import load_checkpoint, save_checkpoint
    a, b = _stack(alg, False), _stack(alg, True)
    for _ in range(7):
        a.step(), b.step()
    path = save_checkpoint(str(tmp_path / 'ckpt.npz'), b)
    for _ in range(13):
        a.step(), b.step()
    sa, sb = _state(a), _state(b)
    _equal(sa, sb)
    assert all(bool(torch.isfinite(t).all()) for t in sb[0][:3]) and sb[1][0]['policy'] == 20 and sb[1][7] == 128 + 7 * 64
    n_rows = len(b.replay_buffer)
    done, fell = sb[0][7][:n_rows].cpu().numpy().astype(bool), V.fell(sb[0][6][:n_rows].cpu().numpy())
    print('   %s: %d transitions, %d done: %d falls, %d episodes cut at 16 steps' % (alg, n_rows, done.sum(), fell.sum(), (done & ~fell).sum()))
    assert not (fell & ~done).any() and 0 < done.sum() < n_rows
    assert b.worker.policy_with_value.check_status() == 0
    c = _stack(alg, True, seed=99)                            # different seed: every stream must come from the file
    meta = load_checkpoint(path, c)
    assert meta['optimizer']['iteration'] == 7 and c.iteration == 7 and c.worker.env._state.dtype == torch.int32
    for _ in range(13):
        c.step()
    _equal(sb, _state(c))


# ---- 8: caller-owned outputs between sentinels ------------------------------------------------------------------------------------
GUARD = 1 << 16


class Guarded(object):
    """tensors of EXACTLY the documented length, each a view between two guard regions of one uint8 buffer filled with 0xFF (every
    float32 word a NaN), in the manner of tests/workspace_guard.py: check() says the guards still hold the fill"""

    def __init__(self):
        self.blocks = []

    def take(self, shape, dtype, init=None):
        item = torch.empty((), dtype=dtype).element_size()
        nb = int(np.prod(shape)) * item
        buf = torch.full((GUARD + nb + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        view = buf[GUARD:GUARD + nb].view(dtype).view(*shape)
        assert view.data_ptr() == buf.data_ptr() + GUARD and view.numel() * item == nb
        if init is not None:
            view.copy_(init)
        self.blocks.append((buf, nb))
        return view

    def check(self, what):
        ok = torch.stack([torch.stack([(b[:GUARD] == 0xFF).all(), (b[GUARD + nb:] == 0xFF).all()]) for b, nb in self.blocks]).cpu().numpy()
        assert ok.all(), (what, ok)


@pytest.mark.parametrize('n,iters', [(1, 25), (17, 3), (33, 25)])
def test_outputs_of_exactly_the_documented_length_between_sentinels(engine, n, iters):
    """every entry point on outputs of exactly obs [n][11], age [n], act [n][1], done [n] and rings of exactly `capacity` rows, with
    capacity == iters * n and the wrap inside the run: the 64 KiB on either side of each stay 0xFF, and the results equal those of
    the plain buffers"""
    p = Policy(True)
    cfg, cap = p.cfg, iters * n
    nxt = cap - 1
    c = loop_case(n)
    f32, i32, u8 = torch.float32, torch.int32, torch.uint8
    g = Guarded()
    t = dict(state=g.take((n,), i32, dev(c['age'], i32)), obs_io=g.take((n, OD), f32, dev(c['obs'])), act_out=g.take((n, AD), f32),
             done_out=g.take((n,), u8), ring_obs=g.take((cap, OD), f32), ring_act=g.take((cap, AD), f32), ring_rew=g.take((cap,), f32),
             ring_obs2=g.take((cap, OD), f32), ring_done=g.take((cap,), u8))
    run_launch(p, 3, 0.1, t, n, iters, cap, nxt, 7, 3)
    plain = fresh(n, cap, c['obs'], c['age'])
    run_launch(p, 3, 0.1, plain, n, iters, cap, nxt, 7, 3)
    torch.cuda.synchronize()
    g.check('mpg_worker_rollout_model')
    assert_same(plain, t, 'guarded launch')
    # the three env entry points on the rows the launch left
    g2 = Guarded()
    obs, age = g2.take((n, OD), f32, t['obs_io']), g2.take((n,), i32, t['state'])
    o2, rew, done = g2.take((n, OD), f32), g2.take((n,), f32), g2.take((n,), u8)
    L.call('mpg_model_env_step', ctypes.byref(cfg), L.c_int(n), L.ptr(obs), L.ptr(t['act_out']), L.c_int(3), L.ptr(age), L.ptr(o2), L.ptr(rew),
           L.ptr(done), L.stream())
    ops.model_env_reset(cfg, o2, age, ESEED, 99, done)
    ring = [g2.take((n, OD), f32), g2.take((n, AD), f32), g2.take((n,), f32), g2.take((n, OD), f32), g2.take((n,), u8)]
    obs_b, age_b, done_b = g2.take((n, OD), f32, t['obs_io']), g2.take((n,), i32, t['state']), g2.take((n,), u8)
    ops.model_env_step_store_reset(cfg, obs_b, t['act_out'], age_b, 3, ring, n, n - 1, ESEED, 99, done_b)
    torch.cuda.synchronize()
    g2.check('mpg_model_env_step / _reset / _step_store_reset')
    assert torch.equal(bits(obs_b), bits(o2)) and torch.equal(age_b, age) and torch.equal(done_b, done)
    assert torch.equal(bits(ring[2].roll(1)), bits(rew)) and torch.isfinite(rew).all()
