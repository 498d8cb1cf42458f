"""The cart-pole env (mpg_amd/csrc/env_cart_pole.hip, step_agent) at its control clamp, its done bounds and far angles, on the start
rows of tests/cart_pole_edge_inputs.py (tests/test_cart_pole_edges.py holds the CPU conditions that make this worth running):

  a. mpg_env_step against the float32 oracle, step by step from the device's OWN state, under bars() - observations, state,
     rewards - done and done_intended in all 3900 pairs, none left out, and the branch counts of the device's trajectory;
  b. mpg_env_step_store_reset from each of those states == mpg_env_step bit for bit in the wrapped ring slots, the done agents re-drawn
     as oracle.cart_pole_reset_philox says (one counter above 2^32), the others kept;
  c. mpg_env_rollout_pendulum from the edge rows: one step against the oracle, 30 steps == the per-step chain bit for bit;
  d. mpg_worker_rollout_pendulum and mpg_worker_sample_rollout_pendulum from the edge states == their chains, bit for bit;
  e. NaN and infinite actions: a NaN action is a NaN transition (as the oracle's np.clip hands it on), an infinite one is +-3.

Every other device test of this env compares a launch with the chain of launches it replaces, which calls the same step_agent; (a),
(c) with n = 1 and (e) are what hold step_agent itself against the oracle.  Floats that must be equal are compared as their 32-bit
patterns."""
import functools

import numpy as np
import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops
from oracle import mpg_oracle as O
from tests import cart_pole_edge_inputs as E
from tests import test_env_rollout_pendulum_gpu as R
from tests import test_worker_rollout_pendulum_gpu as W
from tests import test_worker_sample_rollout_pendulum_gpu as S

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KIND = 1                                                  # MPG_ENV_INVERTED_PENDULUM


def dev(x):
    return torch.tensor(np.asarray(x)).to(DEV)            # (a copy: the shared inputs are read-only)


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


@pytest.fixture(params=list(L.ENGINES))
def engine(request):
    """both builds of the library (mpg_amd/_lib.py ENGINES): the split-fp16 product and the exact-fp32 engine"""
    with L.engine(request.param):
        yield request.param


def rows_of_state(state):
    """the device's state block [8][n] -> [n][4] as the oracle holds it"""
    return np.ascontiguousarray(state[:4].t().cpu().numpy())


# ---- a. mpg_env_step against the oracle --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_run():
    """30 steps of mpg_env_step on the edge rows; per step what the device took and gave, and the float32 oracle's one step from the
    same state with its log.  Computed once and shared by (a) and (b): nothing in it is written to later."""
    from mpg_amd.envs import InvertedPendulumContiEnv
    obs0, act = E.inputs()
    env = InvertedPendulumContiEnv(num_agent=E.N)
    env.reset(init_obs=dev(obs0))
    assert np.array_equal(rows_of_state(env._state).view(np.int32), obs0.view(np.int32))
    a = dev(act)[:, None].contiguous()
    rec = []
    for _ in range(E.STEPS):
        before = env._state.clone()
        o, r, d, _ = env.step(a)
        ref, log = E.one_step(rows_of_state(before), act)
        rec.append(dict(before=before, obs_in=before[:4].t().contiguous(), act=a, obs=o, rew=r, done=d, di=env.done_intended.clone(),
                        state=rows_of_state(env._state), ref=ref, log=log))
    torch.cuda.synchronize()
    return rec


def test_env_step_vs_oracle_at_the_edges():
    """Each step from the device's own previous state (a closed loop would measure how two float32 trajectories of a falling pole
    part, not the kernel).  No pair is left out: tests/test_cart_pole_edges.py shows that none of the oracle's is near a done bound,
    and the assertion on near() below says the same of the oracle's step from every device state.
    Counts: those of the actions alone (EXACT_COUNTS) equal the CPU's; the others - done 0 / 1, either term alone, |theta + theta0| >
    50, |thetadot| > 15 - depend on the last bits of a closed loop of their own and may differ from the CPU's by 5 (the float32 and
    the float64 oracle's closed loops give the SAME counts), and still meet the CPU minimums.
    Measured on an MI355X, worst error / bar: p 0.022, theta 0.033, pdot 0.073, thetadot 0.118, reward 0.015; per group calm 0.074,
    circle 0.060, wound 0.033, spin 0.073, runaway 0.063, clamp 0.118, threshold theta 0.082, threshold p 0.059, zero 0.019, corner
    0.044; 0 pairs near, 0 done flags wrong, every count equal to the CPU's."""
    rec = device_run()
    wo, ws, wr = np.zeros(4), np.zeros(4), 0.
    per_group, bad, done_wrong, left_out = {}, [], 0, 0
    for t, s in enumerate(rec):
        ref, log = s['ref'], s['log']
        left_out += int(E.near(ref['obs']).sum())
        got = s['obs'].cpu().numpy()
        ro, rr = E.ratios(got, s['rew'].cpu().numpy(), ref['obs'], ref['rew'], log['arg'])
        rs, _ = E.ratios(s['state'], ref['rew'], ref['obs'], ref['rew'], log['arg'])
        assert np.isfinite(ro).all() and np.isfinite(rs).all() and np.isfinite(rr).all(), t
        wo, ws, wr = np.maximum(wo, ro.max(0)), np.maximum(ws, rs.max(0)), max(wr, rr.max())
        for i in range(E.N):
            per_group[E.group_of(i)] = max(per_group.get(E.group_of(i), 0.), ro[i].max(), rr[i])
        bad += [(t, int(i), E.group_of(int(i)), E.ENTRY[int(j)], float(ro[i, j])) for i, j in np.argwhere(ro > 1.)[:3]]
        bad += [(t, int(i), E.group_of(int(i)), 'reward', float(rr[i])) for i in np.flatnonzero(rr > 1.)[:3]]
        d, di = s['done'].cpu().numpy().astype(bool), s['di'].cpu().numpy().astype(bool)
        done_wrong += int((d != ref['done']).sum()) + int((di != ref['done']).sum())
    got_obs = np.stack([s['obs'].cpu().numpy() for s in rec])
    got_done = np.stack([s['done'].cpu().numpy().astype(bool) for s in rec])
    c = E.branch_counts([s['log'] for s in rec], got_obs, got_done)
    tr = E.trajectory()
    cpu = E.branch_counts(tr['log'], np.stack([r['obs'] for r in tr['rec']]), np.stack([r['done'] for r in tr['rec']]))
    table = ('device vs float32 oracle, worst error / bar: observation ' + '  '.join('%s %.3f' % kv for kv in zip(E.ENTRY, wo))
             + '; state ' + '  '.join('%.3f' % x for x in ws) + '; reward %.3f; per group ' % wr
             + '  '.join('%s %.3f' % kv for kv in per_group.items())
             + '; pairs left out %d of %d; done / done_intended wrong %d; counts (device / CPU) ' % (left_out, E.PAIRS, done_wrong)
             + '  '.join('%s %d / %d' % (k, c[k], cpu[k]) for k in c))
    print('\n' + table)
    assert not bad, (bad[:10], table)
    assert ws.max() <= 1. and wr <= 1., table
    assert left_out == 0, table
    assert done_wrong == 0, table
    for k in c:
        assert c[k] == cpu[k] if k in E.EXACT_COUNTS else abs(c[k] - cpu[k]) <= 5, (k, table)
        assert c[k] >= E.CPU_MINIMUMS[k], (k, table)


# ---- b. step + ring store + reset == the step ----------------------------------------------------------------------------------
def test_step_store_reset_equals_the_step_at_the_edges():
    """mpg_env_step_store_reset from every pre-step state of (a): its ring row - obs, act, rew, obs2, done, in slots that wrap (100 +
    130 > 160) - equals the state it started from, the action and mpg_env_step's reward, observation and done; a done agent's new
    state and obs_out are row i of cart_pole_reset_philox(130, seed, counter), bit for bit (step 7 with a counter above 2^32); the
    others keep the state the step left."""
    rec = device_run()
    n, cap, nxt, seed = E.N, 160, 100, 5
    slot = (nxt + torch.arange(n, device=DEV)) % cap
    assert int(slot.min()) == 0 and int(slot.max()) == cap - 1
    redrawn = 0
    for t, s in enumerate(rec):
        ctr = 2 ** 33 + 7 if t == 7 else t
        state = s['before'].clone()
        ring = [torch.full((cap, 4), -7., device=DEV), torch.full((cap, 1), -7., device=DEV), torch.full((cap,), -7., device=DEV),
                torch.full((cap, 4), -7., device=DEV), torch.full((cap,), 0xAB, dtype=torch.uint8, device=DEV)]
        obs_out, done_out = torch.empty(n, 4, device=DEV), torch.empty(n, dtype=torch.uint8, device=DEV)
        L.call('mpg_env_step_store_reset', L.c_int(KIND), L.c_int(n), L.c_int(4), L.ptr(state), L.ptr(s['act']), L.c_int(cap), L.c_int(nxt),
               *[L.ptr(x) for x in ring], L.c_u64(seed), L.c_u64(ctr), L.ptr(obs_out), L.ptr(done_out), L.stream())
        for name, got, want in (('obs', ring[0], s['obs_in']), ('act', ring[1], s['act']), ('rew', ring[2], s['rew']),
                                ('obs2', ring[3], s['obs']), ('done', ring[4], s['done'])):
            assert torch.equal(bits(got[slot]), bits(want)), (t, name, torch.nonzero(bits(got[slot]) != bits(want))[:5].tolist())
        untouched = torch.ones(cap, dtype=torch.bool, device=DEV)
        untouched[slot] = False
        assert (ring[2][untouched] == -7.).all() and (ring[4][untouched] == 0xAB).all()
        assert torch.equal(done_out, s['done'])
        done = s['done'].cpu().numpy().astype(bool)
        want = np.where(done[:, None], O.cart_pole_reset_philox(n, seed, ctr), s['obs'].cpu().numpy())
        assert np.array_equal(obs_out.cpu().numpy().view(np.int32), want.view(np.int32)), t
        assert np.array_equal(rows_of_state(state).view(np.int32), want.view(np.int32)), t
        redrawn += int(done.sum())
        if t == 7:                                      # the counter's high word is read: the low word alone draws other states
            assert done.any() and not np.array_equal(O.cart_pole_reset_philox(n, seed, 7)[done], want[done])
    assert 0 < redrawn < E.PAIRS


# ---- c. mpg_env_rollout_pendulum ------------------------------------------------------------------------------------------------
def test_env_rollout_first_step_vs_oracle_at_the_edges(engine):
    """n = 1: no policy pass, rewards[0] and last_obs are step_agent's from (obs0, act0) - under the oracle's bars"""
    obs0, act = E.inputs()
    cfg = ops.make_cfg('InvertedPendulumConti-v0')
    pol = dev(R.policy_weights(np.random.Generator(np.random.PCG64(7500))))
    rew, last = ops.env_rollout_pendulum(cfg, pol, dev(obs0), dev(act)[:, None].contiguous(), 1)
    ref, log = E.one_step(obs0, act)
    ro, rr = E.ratios(last.cpu().numpy(), rew[0].cpu().numpy(), ref['obs'], ref['rew'], log['arg'])
    print('\nmpg_env_rollout_pendulum, n = 1 (%s): worst error / bar observation %s, reward %.3f' % (engine, ro.max(0).round(3), rr.max()))
    assert np.isfinite(ro).all() and np.isfinite(rr).all()
    assert ro.max() <= 1. and rr.max() <= 1., (np.argwhere(ro > 1.)[:5], ro.max(), rr.max())


@pytest.mark.parametrize('gain', [1.0, 400.0], ids=['plain', 'saturated'])
@pytest.mark.parametrize('cache', [False, True], ids=['strided', 'packed'])
def test_env_rollout_equals_the_chain_at_the_edges(engine, cache, gain):
    """n = 30 from the edge rows with their own actions (infinite ones included) as act0: rewards, last observations and the status
    word against mpg_env_reset_from_obs + per step mpg_policy_action (from the second step on) + mpg_env_step, bit for bit; with
    the plain weights and with the output layer x 400 (actions pinned at +-3)"""
    obs0, act = E.inputs()
    pol = R.policy_weights(np.random.Generator(np.random.PCG64(7600)), out_gain=gain)
    if gain > 1.:
        a = ops.policy_action(ops.make_cfg('InvertedPendulumConti-v0'), dev(pol), dev(obs0))
        assert int((a.abs() == 3.0).sum().item()) >= E.N // 2, a.abs().min()
    (ra, oa), (rb, ob), status, _ = R.both(cache, pol, obs0.copy(), act[:, None].copy(), E.STEPS)
    assert torch.isfinite(ra).all() and torch.isfinite(oa).all()
    assert float(oa[:, 1].abs().max()) > 50.           # the wound rows are still wound: nothing was reset
    assert torch.equal(bits(ra), bits(rb)), 'rewards'
    assert torch.equal(bits(oa), bits(ob)), 'last observations'
    assert status[0] == status[1] and not status[1] & ops.STATUS_NAN, status


# ---- d. the worker launches ----------------------------------------------------------------------------------------------------
def both_branches_in_iteration_0(t, n, nxt=5):
    done = t['ring_done'][nxt:nxt + n]
    assert int((done == 0).sum()) >= 10 and int((done == 1).sum()) >= 10, (int((done == 0).sum()), int((done == 1).sum()))


@pytest.mark.parametrize('sigma', [0., 0.1], ids=['no_noise', 'sigma_0.1'])
@pytest.mark.parametrize('packed', [False, True], ids=['strided', 'packed'])
def test_worker_rollout_equals_the_chain_at_the_edges(engine, packed, sigma):
    """mpg_worker_rollout_pendulum with 2 iterations from the edge states == 2 x (mpg_policy_action + mpg_env_step_store_reset): state,
    obs_io, act_out, done_out, the five ring arrays and the status word.  Iteration 0 steps the edge states themselves (the ring's
    observations are the edge rows), iteration 1 the survivors and the re-drawn."""
    obs0, _ = E.inputs()
    p = W.Policy(packed, seed=6)
    a, b = W.both(p, E.N, 2, sigma, init_obs=obs0.copy())
    W.assert_same(a, b, ('worker_rollout_pendulum', packed, sigma))
    assert torch.equal(bits(a['ring_obs'][5:5 + E.N]), bits(dev(obs0)))
    assert not int(a['status'].item()) & ops.STATUS_NAN
    both_branches_in_iteration_0(a, E.N)


@pytest.mark.parametrize('packed', [False, True], ids=['strided', 'packed'])
def test_worker_sample_rollout_equals_the_chain_at_the_edges(engine, packed):
    """the same for mpg_worker_sample_rollout_pendulum against mpg_normal_fill + mpg_policy_sample_squashed + mpg_env_step_store_reset"""
    obs0, _ = E.inputs()
    p = S.Policy(packed, seed=6)
    a, b = S.both(p, E.N, 2, init_obs=obs0.copy())
    S.assert_same(a, b, ('worker_sample_rollout_pendulum', packed))
    assert torch.equal(bits(a['ring_obs'][5:5 + E.N]), bits(dev(obs0)))
    assert not int(a['status'].item()) & ops.STATUS_NAN
    both_branches_in_iteration_0(a, E.N)


# ---- e. non-finite actions -----------------------------------------------------------------------------------------------------
def nan_action_rows():
    """16 calm rows; actions NaN in the even rows, +inf and -inf in turn in the odd ones; and the same rows with +-3 for the infinities"""
    obs0, _ = E.inputs()
    obs = obs0[E.rows_of('calm')].copy()
    act = np.full(E.G, np.nan, np.float32)
    act[1::4], act[3::4] = np.inf, -np.inf
    at3 = np.clip(act, -3., 3.)
    return obs, act, at3


def env_step(obs, act):
    n = len(act)
    state, obs_d, act_d = torch.zeros(8, n, device=DEV), dev(obs), dev(act)
    o, r = torch.empty(n, 4, device=DEV), torch.empty(n, device=DEV)
    d, di = torch.empty(n, dtype=torch.uint8, device=DEV), torch.empty(n, dtype=torch.uint8, device=DEV)
    L.call('mpg_env_reset_from_obs', L.c_int(KIND), L.c_int(n), L.c_int(4), L.ptr(state), L.ptr(obs_d), L.stream())
    L.call('mpg_env_step', L.c_int(KIND), L.c_int(n), L.c_int(4), L.ptr(state), L.ptr(act_d), L.ptr(o), L.ptr(r), L.ptr(d), L.ptr(di), L.stream())
    torch.cuda.synchronize()
    return state, o, r, d, di


def test_a_nan_action_is_a_nan_transition_and_an_infinite_one_is_the_clamp():
    """The oracle's np.clip hands a NaN action on (the reference's PathTracking env does the same through tf.clip_by_value): state,
    observation and reward are NaN and done is 1, every comparison being false.  fminf(fmaxf(NaN, -3), 3) is -3: without the select
    in step_agent a NaN action was a full push to the left with a finite transition and `done` as if nothing had happened
    (measured before the fix: all 8 NaN rows finite with done 0; in the worker launches the ring row held act = NaN beside a finite
    obs2, a reward of -1.02 and done 0).  mpg_env_step and mpg_env_step_store_reset have no status
    word, so the NaN transition is all a caller of InvertedPendulumContiEnv.step gets to see of a NaN policy."""
    obs, act, at3 = nan_action_rows()
    nan, inf = np.isnan(act), np.isinf(act)
    assert nan.sum() == 8 and (act[inf] > 0).sum() == 4 and (act[inf] < 0).sum() == 4
    with np.errstate(invalid='ignore'):
        ref, _ = E.one_step(obs, act)
    assert np.isnan(ref['obs'][nan]).all() and np.isnan(ref['rew'][nan]).all() and ref['done'][nan].all() and np.isfinite(ref['obs'][inf]).all()
    state, o, r, d, di = env_step(obs, act)
    _, o3, r3, d3, _ = env_step(obs, at3)
    nan_t, inf_t = torch.as_tensor(nan).to(DEV), torch.as_tensor(inf).to(DEV)
    print('\nNaN-action rows: finite observations %d of 8, finite rewards %d, done %s' % (
        int(torch.isfinite(o[nan_t]).all(1).sum()), int(torch.isfinite(r[nan_t]).sum()), d[nan_t].tolist()))
    assert torch.isnan(o[nan_t]).all() and torch.isnan(state[:4].t()[nan_t]).all() and torch.isnan(r[nan_t]).all()
    assert (d[nan_t] == 1).all() and (di[nan_t] == 1).all()
    # the infinite rows: the rows at +-3, bit for bit, and the oracle's inside its bars
    assert torch.equal(bits(o[inf_t]), bits(o3[inf_t])) and torch.equal(bits(r[inf_t]), bits(r3[inf_t])) and torch.equal(d[inf_t], d3[inf_t])
    ro, rr = E.ratios(o[inf_t].cpu().numpy(), r[inf_t].cpu().numpy(), ref['obs'][inf], ref['rew'][inf], None)
    assert ro.max() <= 1. and rr.max() <= 1. and np.array_equal(d[inf_t].cpu().numpy().astype(bool), ref['done'][inf])
    # the fused step: act NaN, obs2 and reward NaN, done 1, and the agent re-drawn
    n, cap, nxt, seed, ctr = E.G, 24, 20, 9, 2
    st2, obs_d, act_d = torch.zeros(8, n, device=DEV), dev(obs), dev(act)
    L.call('mpg_env_reset_from_obs', L.c_int(KIND), L.c_int(n), L.c_int(4), L.ptr(st2), L.ptr(obs_d), L.stream())
    ring = [torch.full((cap, 4), -7., device=DEV), torch.full((cap, 1), -7., device=DEV), torch.full((cap,), -7., device=DEV),
            torch.full((cap, 4), -7., device=DEV), torch.full((cap,), 0xAB, dtype=torch.uint8, device=DEV)]
    obs_out, done_out = torch.empty(n, 4, device=DEV), torch.empty(n, dtype=torch.uint8, device=DEV)
    L.call('mpg_env_step_store_reset', L.c_int(KIND), L.c_int(n), L.c_int(4), L.ptr(st2), L.ptr(act_d), L.c_int(cap), L.c_int(nxt),
           *[L.ptr(x) for x in ring], L.c_u64(seed), L.c_u64(ctr), L.ptr(obs_out), L.ptr(done_out), L.stream())
    slot = (nxt + torch.arange(n, device=DEV)) % cap
    assert torch.equal(bits(ring[0][slot]), bits(obs_d)) and torch.equal(bits(ring[1][slot][:, 0]), bits(act_d))
    assert torch.isnan(ring[1][slot][nan_t]).all() and torch.isnan(ring[3][slot][nan_t]).all() and torch.isnan(ring[2][slot][nan_t]).all()
    assert (ring[4][slot][nan_t] == 1).all() and (done_out[nan_t] == 1).all()
    assert torch.equal(bits(ring[3][slot][inf_t]), bits(o[inf_t])) and torch.equal(bits(ring[2][slot][inf_t]), bits(r[inf_t]))
    fresh = O.cart_pole_reset_philox(n, seed, ctr)
    assert np.array_equal(obs_out.cpu().numpy()[nan].view(np.int32), fresh[nan].view(np.int32))
    assert np.array_equal(rows_of_state(st2)[nan].view(np.int32), fresh[nan].view(np.int32))


def nan_policy_row(t, row):
    """a NaN into that row's obs_io only: the agent's state stays finite, its policy output is NaN"""
    t['obs_io'][row] = float('nan')
    return t


@pytest.mark.parametrize('which', ['rollout', 'rollout_noise', 'sample_rollout'])
def test_worker_launches_with_a_nan_policy_output_equal_their_chains(engine, which):
    """one edge-state row whose policy output is NaN (its obs_io is NaN, its state is not): the launch and its chain stay bit-identical,
    both report MPG_STATUS_NAN, and the row's transition of iteration 0 is the NaN one - a finite observation, a NaN action, NaN
    obs2 and reward, done 1 - behind which the agent is re-drawn and finite again"""
    obs0, _ = E.inputs()
    n, iters, nxt, row = E.N, 2, 5, 5
    cap = iters * n + 13
    if which == 'sample_rollout':
        M, p = S, S.Policy(True, seed=6)
        run = lambda f, t: f(p, t, n, iters, cap, nxt, 7, 3)
    else:
        M, p = W, W.Policy(True, seed=6)
        run = lambda f, t: f(p, t, n, iters, 0.1 if which == 'rollout_noise' else 0., cap, nxt, 7, 3)
    a, b = nan_policy_row(M.start(n, cap, obs0.copy()), row), nan_policy_row(M.start(n, cap, obs0.copy()), row)
    run(M.run_chain, a)
    run(M.run_launch, b)
    torch.cuda.synchronize()
    M.assert_same(a, b, which)
    assert int(b['status'].item()) & ops.STATUS_NAN
    s = nxt + row
    print('\n%s (%s): the NaN-policy row: act %s, obs2 %s, rew %s, done %d' % (which, engine, b['ring_act'][s].tolist(), b['ring_obs2'][s].tolist(),
                                                                            float(b['ring_rew'][s]), int(b['ring_done'][s])))
    assert torch.equal(bits(b['ring_obs'][s]), bits(dev(obs0[row])))       # the ring's observation is the agent's state: finite
    assert torch.isnan(b['ring_act'][s]).all() and torch.isnan(b['ring_obs2'][s]).all() and torch.isnan(b['ring_rew'][s])
    assert int(b['ring_done'][s]) == 1
    keep = torch.ones(cap, dtype=torch.bool, device=DEV)
    keep[s] = False
    for k in ('ring_act', 'ring_rew', 'ring_obs2'):
        assert torch.isfinite(b[k][keep]).all(), k
    assert torch.isfinite(b['state'][:4]).all() and torch.isfinite(b['obs_io']).all() and torch.isfinite(b['act_out']).all()
