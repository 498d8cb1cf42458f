"""The real path-tracking env (mpg_amd/csrc/env_path_tracking.hip) at its own branches, on the start rows of tests/env_edge_inputs.py
(tests/test_env_edges.py holds the CPU conditions that make this worth running):

  a. mpg_env_step against the float32 oracle, step by step from the device's OWN state, under bars() - observations, state, rewards,
     done and done_intended - with the branch counts of the device's trajectory, exact clamp values and the range of x;
  b. mpg_env_step_store_reset (four lanes per agent, step_agent<4>) from each of those states == mpg_env_step (one lane), bit for bit;
  c. mpg_env_rollout (four lanes, 25 steps, policies that push the groups into their branches) == the per-step chain, bit for bit;
  d. mpg_worker_step and mpg_worker_rollout from the edge states == their chains, bit for bit.

Floats that must be equal are compared as their 32-bit patterns."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops
from tests import env_edge_inputs as E
from tests import test_worker_rollout_gpu as W

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PAIRS = E.N * E.STEPS


def dev(x):
    return torch.tensor(np.asarray(x)).to(DEV)           # (a copy: the shared inputs are read-only)


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


@pytest.fixture(params=['split', 'f32'])
def engine(request):
    """both builds of the library (mpg_amd/_lib.py ENGINES): the split-fp16 product and the exact-fp32 engine"""
    with L.engine(request.param):
        yield request.param


def split_state(state):
    """the device's state block [8][n] -> (veh_state, veh_full_state) as the oracle holds them"""
    s = state.cpu().numpy()
    return np.ascontiguousarray(s[[0, 1, 2, 6, 7, 5]].T), np.ascontiguousarray(s[:6].T)


def obs_of_state(state, od):
    """the observation of a state block as the device forms it: mpg_env_reset under a mask of zeros draws nothing and writes it"""
    n = state.shape[1]
    obs = torch.empty(n, od, device=DEV)
    mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
    L.call('mpg_env_reset', L.c_int(0), L.c_int(n), L.c_int(od), L.ptr(state), L.ptr(mask), L.c_u64(0), L.c_u64(0), L.ptr(obs), L.stream())
    return obs


# ---- a. mpg_env_step against the oracle --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_run(K):
    """30 steps of mpg_env_step on the edge rows; per step what the device took and gave, and the float32 oracle's one step from the
    same state with its log.  Computed once per K and shared by (a) and (b): nothing in it is written to later."""
    from mpg_amd.envs import PathTrackingEnv
    obs0, act = E.inputs(K)
    env = PathTrackingEnv(num_future_data=K, num_agent=E.N)
    env.reset(init_obs=dev(obs0))
    start = split_state(env._state)
    rec = []
    for t in range(E.STEPS):
        a = E.actions_at(act, t)
        before = env._state.clone()
        obs_in = obs_of_state(before, 6 + K)
        assert torch.equal(bits(before), bits(env._state))
        o, r, d, _ = env.step(dev(a))
        ref, log = E.one_step(K, split_state(before), a)
        vs, fs = split_state(env._state)
        rec.append(dict(before=before, act=dev(a), obs_in=obs_in, obs=o, rew=r, done=d, di=env.done_intended.clone(), state=vs, full=fs,
                        ref=ref, log=log, x_before=before[5].cpu().numpy()))
    torch.cuda.synchronize()
    return dict(start=start, rec=rec)


@pytest.mark.parametrize('K', [0, 3, 10])
def test_env_step_vs_oracle_at_the_edges(K):
    """Each step from the device's own previous state (a closed loop would measure how two float32 trajectories part, not the
    kernel).  Pairs that near() marks on the oracle's side are left out of the x, heading, delta_phi and done_intended comparisons
    only, and may be 1 % of all pairs at the most."""
    obs0, _ = E.inputs(K)
    run = device_run(K)
    # reset(init_obs): path_ref at far and negative x (the sincosf branch of sincos_bounded included)
    ora = E.LoggingEnvOracle(E.N, K)
    ora.reset(init_obs=obs0.copy())
    vs0, fs0 = run['start']
    _, ftol = E.bars(obs0, ora.veh_full_state)
    assert np.array_equal(vs0, ora.veh_state) and np.array_equal(fs0[:, [0, 1, 2, 5]], ora.veh_full_state[:, [0, 1, 2, 5]])
    e0 = np.abs(fs0.astype(np.float64) - ora.veh_full_state) / ftol
    print('\nK=%d reset(init_obs): y %.3f of its bar, phi %.3f' % (K, e0[:, 3].max(), e0[:, 4].max()))
    assert e0.max() <= 1., np.argwhere(e0 > 1.)[:5]

    wo, wf, wr = np.zeros(6 + K), np.zeros(6), 0.
    bad, left_out, di_wrong = [], 0, 0
    inside = E.in_range_rows()
    for t, s in enumerate(run['rec']):
        ref, log = s['ref'], s['log']
        nr = E.near([log], [ref['cmp']])[0]
        left_out += int(nr.sum())
        ro, rf, rr = E.ratios(s['obs'].cpu().numpy(), s['full'], s['rew'].cpu().numpy(), ref['obs'].astype(np.float64),
                              ref['full'].astype(np.float64), ref['rew'], E.x_magnitude(log, s['x_before']), skip=nr)
        assert np.isfinite(ro).all() and np.isfinite(rf).all() and np.isfinite(rr).all(), t
        wo, wf, wr = np.maximum(wo, ro.max(0)), np.maximum(wf, rf.max(0)), max(wr, rr.max())
        bad += [(t,) + tuple(i) for i in np.argwhere(ro > 1.)[:3]] + [(t, 'state') + tuple(i) for i in np.argwhere(rf > 1.)[:3]]
        assert bool(s['done'].all()), t                                     # the literal flag: always 1
        di = s['di'].cpu().numpy().astype(bool)
        di_wrong += int((di != ref['di'])[~nr].sum())
        # the clamp's own values, exactly, where the oracle's last sub-step clamps
        raw = log['vx'][-1]
        assert (s['full'][raw < 1. - 1e-6, 0] == 1.).all() and (s['full'][raw > 35. + 1e-5, 0] == 35.).all(), t
        assert (s['full'][:, 0] >= 1.).all() and (s['full'][:, 0] <= 35.).all(), t
        # x inside (0, 1200] for every agent that started there; the far and negative rows come back by one period per sub-step
        x = s['full'][inside, 5]
        assert (x > 0.).all() and (x <= 1200.).all(), t
        assert (np.abs(s['full'][:, 4]) <= np.pi + 1e-6).all(), t
    names = E.ENTRY + tuple('ahead %d' % k for k in range(K))
    print('K=%d device vs float32 oracle, worst error / bar per entry' % K)
    print('   observation: ' + '  '.join('%s %.3f' % kv for kv in zip(names, wo)))
    print('   state:       ' + '  '.join('%s %.3f' % kv for kv in zip(E.FULL_ENTRY, wf)))
    print('   reward %.3f   pairs left out as near: %d of %d   done_intended wrong outside them: %d' % (wr, left_out, PAIRS, di_wrong))
    c = E.branch_counts([s['log'] for s in run['rec']])
    print('   branch counts of the device trajectory: ' + '  '.join('%s %d' % (k, c[k]) for k in list(E.CPU_MINIMUMS) + ['leave_hi']))
    assert not bad, bad[:10]
    assert wr <= 1., wr
    assert di_wrong == 0
    assert left_out <= 0.01 * PAIRS, left_out
    for k, least in E.CPU_MINIMUMS.items():                                  # half the CPU minimums: the closed loops drift apart
        assert c[k] >= least / 2, (k, c[k])
    assert c['leave_hi'] >= 1, c


# ---- b. four lanes == one lane -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [0, 3])
def test_four_lane_step_equals_one_lane_step_at_the_edges(K):
    """mpg_env_step_store_reset below 65 536 agents is k_step_store_reset (step_agent<4>: the heading wraps in phase A, x in phase
    C); from every pre-step state of (a) its ring row - obs, act, obs2, rew, done - equals the input observation, the action and
    mpg_env_step's obs, reward and done.  The ring position wraps (150 + 146 > 200)."""
    run = device_run(K)
    c = E.branch_counts([s['log'] for s in run['rec']])
    for k in list(E.CPU_MINIMUMS) + ['leave_hi', 'last_x_down', 'last_x_up', 'last_phi_down', 'last_phi_up', 'last_dphi_down', 'last_dphi_up']:
        assert c[k] >= 1, (k, c)                       # every branch is among the states stepped here
    n, od, cap, nxt = E.N, 6 + K, 200, 150
    slot = (nxt + torch.arange(n, device=DEV)) % cap
    for t, s in enumerate(run['rec']):
        if t > 0:                                      # the observation of a state IS the previous step's output
            assert torch.equal(bits(s['obs_in']), bits(run['rec'][t - 1]['obs'])), t
        state = s['before'].clone()
        ring = [torch.full((cap, od), -7., device=DEV), torch.full((cap, 2), -7., device=DEV), torch.full((cap,), -7., device=DEV),
                torch.full((cap, od), -7., device=DEV), torch.full((cap,), 0xAB, dtype=torch.uint8, device=DEV)]
        obs_out, done_out = torch.empty(n, od, device=DEV), torch.empty(n, dtype=torch.uint8, device=DEV)
        L.call('mpg_env_step_store_reset', L.c_int(0), L.c_int(n), L.c_int(od), L.ptr(state), L.ptr(s['act']), L.c_int(cap), L.c_int(nxt),
               *[L.ptr(x) for x in ring], L.c_u64(5), L.c_u64(t), L.ptr(obs_out), L.ptr(done_out), L.stream())
        for name, got, want in (('obs', ring[0], s['obs_in']), ('act', ring[1], s['act']), ('obs2', ring[3], s['obs']),
                                ('rew', ring[2], s['rew']), ('done', ring[4], s['done'])):
            assert torch.equal(bits(got[slot]), bits(want)), (t, name, torch.nonzero(bits(got[slot]) != bits(want))[:5].tolist())
        assert torch.equal(done_out, s['done']) and torch.isfinite(obs_out).all()


# ---- c. mpg_env_rollout ------------------------------------------------------------------------------------------------------
# (steer, a_x) the policy's mean action is pushed to, and the end of [1, 35] that at least 20 (agent, step) pairs must be clamped at.
# 'throttle_right' has none: a steer of -0.8 (0.34 rad) at 34 m/s makes v_y r about -6 m/s^2 against an a_x of 2.4, the vehicle slows
# down and 4 .. 5 pairs sit at 35 (measured on the chain); 'throttle' is the policy that holds the 'accelerate' group at 35, 'throttle_right'
# the one that spins every group to the right.
PUSHES = {'brake_left': (0.8, -0.8, 1.), 'throttle_right': (-0.8, 0.8, None), 'throttle': (-0.1, 0.8, 35.)}


class PushPolicy(object):
    """a policy whose last-layer bias is shifted so that its mean action is about (steer, a_x): tanh output, the shift is
    atanh(action); with or without the packed weight image (built AFTER the shift).  The last layer's kernel is scaled by 0.1 so
    that the bias decides for EVERY group: with the plain kernel the edge rows' large inputs (v_x - 20 = 14, x / 1200 = 33) leave
    the 'accelerate' group a mean a_x of 0.19 (obs_dim 6) and -0.05 (obs_dim 9) under a push to +0.8 (float32 oracle)."""

    def __init__(self, od, packed, steer, a_x):
        from tests.golden_inputs import mlp_weights_flat
        w = mlp_weights_flat(np.random.Generator(np.random.PCG64(300 + od)), od, 4)
        w[-4 - 256 * 4:-4] *= np.float32(0.1)
        w[-4] += np.arctanh(steer)
        w[-3] += np.arctanh(a_x)
        self.cfg = ops.make_cfg(obs_dim=od)
        self.pol = dev(w)
        self.wc = None
        if packed:
            self.wc = ops.WeightCache(self.pol, [(od, 4)])
            self.cfg.wcache[0] = self.wc.pointer
        self.status = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.cfg.status = self.status.data_ptr()


def recorded_chain(p, obs0, act0, n):
    """mpg_env_reset_from_obs, then per step mpg_policy_action (from the second step on) and mpg_env_step - the sequence
    mpg_env_rollout replaces - with the state and the action every step was taken from"""
    rows, od = obs0.shape
    state = torch.zeros(8, rows, device=DEV)
    obs, act, rew = torch.empty(rows, od, device=DEV), torch.empty(rows, 2, device=DEV), torch.empty(n, rows, device=DEV)
    done, done_i = torch.empty(rows, dtype=torch.uint8, device=DEV), torch.empty(rows, dtype=torch.uint8, device=DEV)
    L.call('mpg_env_reset_from_obs', L.c_int(0), L.c_int(rows), L.c_int(od), L.ptr(state), L.ptr(obs0), L.stream())
    taken = []
    for t in range(n):
        if t > 0:
            L.call('mpg_policy_action', ctypes.byref(p.cfg), L.ptr(p.pol), L.c_int(rows), L.ptr(obs), L.c_float(0.), L.c_u64(0), L.c_u64(0),
                   L.ptr(act), L.stream())
        a = act0 if t == 0 else act
        taken.append((state.clone(), a.clone()))
        L.call('mpg_env_step', L.c_int(0), L.c_int(rows), L.c_int(od), L.ptr(state), L.ptr(a), L.ptr(obs), L.ptr(rew[t]), L.ptr(done),
               L.ptr(done_i), L.stream())
        taken[-1] += (state[0].clone(),)
    return rew, obs, taken


@pytest.mark.parametrize('push', list(PUSHES))
@pytest.mark.parametrize('packed', [False, True], ids=['strided', 'packed'])
@pytest.mark.parametrize('od', [6, 9])
def test_env_rollout_equals_the_chain_at_the_edges(engine, od, packed, push):
    """k_env_rollout: step_agent<4> 25 times with the agents held in registers, no reset.  Rewards, last observations and the status
    word against the chain, bit for bit; and the chain's own states say that the branches were taken."""
    K, n = od - 6, 25
    o, a = E.inputs(K)
    obs0, act0 = dev(o), dev(a)
    steer, a_x, end = PUSHES[push]
    p = PushPolicy(od, packed, steer, a_x)
    rew_a, obs_a, taken = recorded_chain(p, obs0, act0, n)
    status_a = int(p.status.item())
    p.status.zero_()
    rew_b, obs_b = ops.env_rollout(p.cfg, p.pol, obs0, act0, n)
    torch.cuda.synchronize()
    assert torch.isfinite(rew_a).all() and torch.isfinite(obs_a).all()
    assert torch.equal(bits(rew_a), bits(rew_b)), 'rewards'
    assert torch.equal(bits(obs_a), bits(obs_b)), 'last observations'
    assert status_a == int(p.status.item())
    # what the chain went through: the oracle's log of one step from each recorded state
    logs, mean_act, clamped = [], np.zeros(2), 0
    at = 35. if end is None else end
    for t, (state, act, vx_after) in enumerate(taken):
        logs.append(E.one_step(K, split_state(state), act.cpu().numpy())[1])
        clamped += int((vx_after == at).sum().item())
        if t > 0:
            mean_act += act.mean(0).cpu().numpy() / (n - 1)
    c = E.branch_counts(logs)
    print('\nod %d %s %s (%s): mean action (%.2f, %.2f); pairs clamped at %g: %d; last-sub-step wraps x %d / %d, heading %d / %d' % (
        od, 'packed' if packed else 'strided', push, engine, mean_act[0], mean_act[1], at, clamped, c['last_x_down'], c['last_x_up'],
        c['last_phi_down'], c['last_phi_up']))
    assert abs(mean_act[0] - steer) <= 0.2 and abs(mean_act[1] - a_x) <= 0.2, mean_act
    if end is not None:
        assert clamped >= 20, clamped
    assert c['last_x_down'] + c['last_x_up'] >= 1, c
    if abs(steer) > 0.5:                              # the policies that spin
        assert c['last_phi_down'] + c['last_phi_up'] >= 1, c
    del p


# ---- d. the worker launches --------------------------------------------------------------------------------------------------
def edge_start(p, cap):
    """one side's buffers (tests/test_worker_rollout_gpu.start) with the agents and obs_io loaded from the edge rows"""
    o, _ = E.inputs(p.od - 6)
    obs = dev(o)
    state = torch.zeros(8, E.N, device=DEV)
    L.call('mpg_env_reset_from_obs', L.c_int(0), L.c_int(E.N), L.c_int(p.od), L.ptr(state), L.ptr(obs), L.stream())
    f = dict(dtype=torch.float32, device=DEV)
    return dict(state=state, obs_io=obs.clone(), act_out=torch.full((E.N, 2), -7., **f),
                done_out=torch.full((E.N,), 0xAB, dtype=torch.uint8, device=DEV),
                ring_obs=torch.full((cap, p.od), -7., **f), ring_act=torch.full((cap, 2), -7., **f), ring_rew=torch.full((cap,), -7., **f),
                ring_obs2=torch.full((cap, p.od), -7., **f), ring_done=torch.full((cap,), 0xAB, dtype=torch.uint8, device=DEV))


def stepped_the_edge_rows(t, p, nxt, cap):
    """the ring rows of iteration 0 hold the edge rows' own x (far and negative ones included) and finite results"""
    o, _ = E.inputs(p.od - 6)
    slot = (nxt + torch.arange(E.N, device=DEV)) % cap
    assert torch.equal(bits(t['ring_obs'][slot][:, 5]), bits(dev(o[:, 5])))
    assert torch.isfinite(t['ring_obs2'][slot]).all() and torch.isfinite(t['ring_rew'][slot]).all() and (t['ring_done'][slot] == 1).all()


@pytest.mark.parametrize('od,packed', [(6, False), (6, True), (9, False)])
def test_worker_step_equals_its_two_launches_at_the_edges(engine, od, packed):
    """mpg_worker_step (policy pass + env_lane<4>) == mpg_policy_action + mpg_env_step_store_reset from the edge states"""
    p = W.Policy(od, packed, seed=4)
    n, cap, nxt, sigma = E.N, 2 * E.N + 5, E.N + 30, 0.1               # nxt + n wraps
    a, b = edge_start(p, cap), edge_start(p, cap)
    p.status.zero_()
    L.call('mpg_policy_action', ctypes.byref(p.cfg), L.ptr(p.pol), L.c_int(n), L.ptr(a['obs_io']), L.c_float(sigma), L.c_u64(11), L.c_u64(7),
           L.ptr(a['act_out']), L.stream())
    L.call('mpg_env_step_store_reset', L.c_int(0), L.c_int(n), L.c_int(od), L.ptr(a['state']), L.ptr(a['act_out']), L.c_int(cap), L.c_int(nxt),
           *W.ring_ptrs(a), L.c_u64(4), L.c_u64(3), L.ptr(a['obs_io']), L.ptr(a['done_out']), L.stream())
    a['status'] = p.status.clone()
    W.run_chain(p, b, n, 1, sigma, cap, nxt, 7, 3)                     # (one mpg_worker_step)
    torch.cuda.synchronize()
    W.assert_same(a, b, ('worker_step', od, packed))
    stepped_the_edge_rows(b, p, nxt, cap)


@pytest.mark.parametrize('packed', [False, True], ids=['strided', 'packed'])
def test_worker_rollout_equals_the_chain_at_the_edges(engine, packed):
    """mpg_worker_rollout with 2 iterations == 2 x mpg_worker_step: iteration 0 steps the edge states, everything after it is a
    fresh reset-law draw (done is always 1)"""
    p = W.Policy(6, packed, seed=5)
    n, iters, cap, nxt, sigma = E.N, 2, 2 * E.N, E.N + 30, 0.1         # every slot written once, the wrap inside iteration 0
    a, b = edge_start(p, cap), edge_start(p, cap)
    W.run_chain(p, a, n, iters, sigma, cap, nxt, 7, 3)
    W.run_launch(p, b, n, iters, sigma, cap, nxt, 7, 3)
    torch.cuda.synchronize()
    W.assert_same(a, b, ('worker_rollout', packed))
    stepped_the_edge_rows(b, p, nxt, cap)
