"""mpg_mpc_rollout, mpc_rollout and run_mpc(one_launch / warm_start) on the GPU, on both engines: the one launch against the chain it
replaces - mpc_solve, the torch ops of run_mpc and PathTrackingEnv.step, step by step - bit for bit on everything both leave behind.
Floats are compared as their 32-bit patterns.  Start observations: tests/env_edge_inputs.inputs(0), the rows that drive the env through
its clamps and wraps, and for the warm start's worth the reset law as the oracle env draws it."""
import functools

import numpy as np
import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import mpc as M
from mpg_amd.envs import PathTrackingEnv
from oracle.mpg_oracle import PathTrackingEnvOracle
from tests import env_edge_inputs as E

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KEYS = ('obs_traj', 'plan_traj', 'rew_traj', 'cost_traj', 'pgnorm_traj', 'info_traj', 'state', 'obs_io', 'u_io', 'done', 'done_intended')
SENTINEL, SENTINEL_U8 = -7, 249


@pytest.fixture(params=['split', 'f32'])
def engine(request):
    """both builds of the library (mpg_amd/_lib.py ENGINES); the code has no matrix instruction and is the same in both"""
    with L.engine(request.param):
        yield request.param


def bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def assert_same(got, want, keys=KEYS):
    for k in keys:
        assert same_bits(got[k], want[k]), k


@functools.lru_cache(maxsize=None)
def edge_obs(n):
    """n rows of the edge inputs, read-only: the start speeds of 0.5 and 40 first, then the nine groups in turn (a row of each: the clamp at
    1, the clamp at 35, the x wraps, the heading wraps, far and negative x, the calm ones), cycled"""
    obs, _ = E.inputs(0)
    order = [E.ROW_SLOW, E.ROW_FAST] + [g * E.G + j for j in range(E.G) for g in range(len(E.GROUPS))]
    assert sorted(order) == list(range(E.N))
    out = np.ascontiguousarray(obs[np.array(order)[np.arange(n) % E.N]], dtype=np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def start_point(n, h, kind):
    """zeros (main.py:184), or a start with a fifth of its entries outside the box"""
    u = np.zeros((n, h, 2), np.float32) if kind == 'zeros' else np.random.default_rng(17).uniform(-1.25, 1.25, (n, h, 2)).astype(np.float32)
    u.setflags(write=False)
    return u


def dev(x):
    return torch.as_tensor(np.array(x), dtype=torch.float32).to(DEV)


def fresh_env(obs0):
    env = PathTrackingEnv(num_future_data=0, num_agent=obs0.shape[0], device=DEV)
    env.reset(init_obs=obs0.clone())
    return env


def chain(obs0, u0, steps, iters, tol, warm):
    """the five steps of include/mpg_hip.h, a launch or a torch op each"""
    n, h = u0.shape[0], u0.shape[1]
    env = fresh_env(obs0)
    shift = torch.zeros(6, device=DEV)
    shift[0] = 20.
    u_io = u0.clone()
    out = {k: [] for k in KEYS[:6]}
    for _ in range(steps):
        out['obs_traj'].append(env.obs)
        x0 = env.obs + shift
        u, cost, pg, info = M.mpc_solve(x0, u_io, iters=iters, tol=tol)
        if warm:
            u_io = torch.cat([u[:, 1:], u[:, -1:]], 1)
        _, rew, _, _ = env.step(u[:, 0, :].contiguous())
        for k, v in (('plan_traj', u), ('rew_traj', rew), ('cost_traj', cost), ('pgnorm_traj', pg), ('info_traj', info)):
            out[k].append(v)
    out = {k: torch.stack(v) for k, v in out.items()}
    out.update(state=env._state, obs_io=env.obs, u_io=u_io, done=env.done, done_intended=env.done_intended)
    return out


def launch(obs0, u0, steps, iters, tol, warm, null=(), pad=0, state=None):
    """one call of the entry point on its own buffers; every array is flat with room for `pad` more agents behind it, filled with the
    sentinel; `null`: the nullable arguments to leave out; `state`: the env state block to go on from (default: rebuilt from obs0)"""
    n, h = u0.shape[0], u0.shape[1]

    def buf(per_agent, rows=1, dtype=torch.float32, init=None):
        t = torch.full((rows * n * per_agent + pad * per_agent,), SENTINEL_U8 if dtype == torch.uint8 else SENTINEL, dtype=dtype, device=DEV)
        if init is not None:
            t[:init.numel()] = init.reshape(-1)
        return t
    st = buf(8, init=fresh_env(obs0)._state if state is None else state)
    b = dict(state=st, obs_io=buf(6, init=obs0), u_io=buf(2 * h, init=u0), obs_traj=buf(6, steps), plan_traj=buf(2 * h, steps),
             rew_traj=buf(1, steps), cost_traj=buf(1, steps), pgnorm_traj=buf(1, steps), info_traj=buf(1, steps, torch.int32),
             done=buf(1, dtype=torch.uint8, init=None), done_intended=buf(1, dtype=torch.uint8))
    arg = {k: (None if k in null else v) for k, v in b.items()}
    L.call('mpg_mpc_rollout', L.c_int(n), L.c_int(steps), L.c_int(h), L.c_int(iters), L.c_float(tol), L.c_int(int(warm)), L.ptr(arg['state']),
           L.ptr(arg['obs_io']), L.ptr(arg['u_io']), L.ptr(arg['obs_traj']), L.ptr(arg['plan_traj']), L.ptr(arg['rew_traj']),
           L.ptr(arg['cost_traj']), L.ptr(arg['pgnorm_traj']), L.ptr(arg['info_traj']), L.ptr(arg['done']), L.ptr(arg['done_intended']),
           L.stream())
    shapes = dict(state=(8, n), obs_io=(n, 6), u_io=(n, h, 2), obs_traj=(steps, n, 6), plan_traj=(steps, n, h, 2), rew_traj=(steps, n),
                  cost_traj=(steps, n), pgnorm_traj=(steps, n), info_traj=(steps, n), done=(n,), done_intended=(n,))
    out = {k: v[:int(np.prod(shapes[k]))].view(shapes[k]) for k, v in b.items()}
    tails = {k: v[int(np.prod(shapes[k])):] for k, v in b.items()}
    return out, tails


# ---- the chain, bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('warm', (0, 1))
@pytest.mark.parametrize('tol', (0., 1e-2))
@pytest.mark.parametrize('h', (1, 5))
@pytest.mark.parametrize('n', (1, 63, 65, 130))
def test_one_launch_is_the_chain(engine, n, h, tol, warm):
    obs0, u0 = dev(edge_obs(n)), dev(start_point(n, h, 'zeros'))
    want = chain(obs0, u0, 3, 20, tol, warm)
    got, _ = launch(obs0, u0, 3, 20, tol, warm)
    assert_same(got, want)
    assert same_bits(got['obs_traj'][0], obs0)
    if not warm:
        assert same_bits(got['u_io'], u0)


def test_a_nan_agent_fails_every_search_and_leaves_its_neighbours_alone(engine):
    n, h, bad = 65, 5, 3
    obs0, u0 = dev(edge_obs(n)), dev(start_point(n, h, 'zeros'))
    clean, _ = launch(obs0, u0, 3, 20, 1e-2, 1)
    obs_nan = obs0.clone()
    obs_nan[bad, 1] = float('nan')                  # v_y
    got, _ = launch(obs_nan, u0, 3, 20, 1e-2, 1)
    assert (got['info_traj'][:, bad] == -1).all()
    assert (got['plan_traj'][:, bad] == 0).all()    # the last accepted point: the start, and its shift
    keep = [i for i in range(n) if i != bad]
    for k in KEYS:
        a, b = (got[k], clean[k]) if k != 'state' else (got[k].t(), clean[k].t())
        if k in KEYS[:6]:
            a, b = a.transpose(0, 1), b.transpose(0, 1)
        assert same_bits(a[keep], b[keep]), k
    # and the chain does the same with it (a NaN's payload is not part of the claim: NaN wherever the chain has one, the bits elsewhere)
    want = chain(obs_nan, u0, 3, 20, 1e-2, 1)
    for k in KEYS:
        a, b = got[k], want[k]
        if a.dtype == torch.float32:
            assert torch.equal(a.isnan(), b.isnan()), k
            a, b = a.nan_to_num(nan=0.), b.nan_to_num(nan=0.)
        assert same_bits(a, b), k


@pytest.mark.parametrize('n, steps, h, iters', [(2, 2, 25, 30), (1, 2, 31, 5)])
@pytest.mark.parametrize('warm', (0, 1))
def test_long_horizons(engine, n, steps, h, iters, warm):
    """horizon 25: main.py's; horizon 31: 85 KiB of LDS, which this kernel asks for by name"""
    obs0, u0 = dev(edge_obs(n + 2)[2:]), dev(start_point(n, h, 'zeros'))
    got, _ = launch(obs0, u0, steps, iters, 0., warm)
    assert_same(got, chain(obs0, u0, steps, iters, 0., warm))


@pytest.mark.parametrize('warm', (0, 1))
def test_a_start_point_outside_the_box(engine, warm):
    n, h = 65, 5
    obs0, u0 = dev(edge_obs(n)), dev(start_point(n, h, 'outside'))
    assert (u0.abs() > 1).any()
    got, _ = launch(obs0, u0, 3, 20, 1e-2, warm)
    assert_same(got, chain(obs0, u0, 3, 20, 1e-2, warm))
    assert (got['plan_traj'].abs() <= 1).all()
    # no iterations: the plan of every step is the clamped start point, moved up by one pair per step with a warm start
    got0, _ = launch(obs0, u0, 3, 0, 0., warm)
    assert_same(got0, chain(obs0, u0, 3, 0, 0., warm))
    assert same_bits(got0['plan_traj'][0], u0.clamp(-1, 1))
    if warm:
        assert same_bits(got0['plan_traj'][2][:, 0], u0.clamp(-1, 1)[:, 2]) and same_bits(got0['u_io'][:, 0], u0.clamp(-1, 1)[:, 3])
        assert same_bits(got0['u_io'][:, -1], u0.clamp(-1, 1)[:, -1])
    else:
        assert same_bits(got0['plan_traj'][2], u0.clamp(-1, 1)) and same_bits(got0['u_io'], u0)


@pytest.mark.parametrize('warm', (0, 1))
def test_two_and_three_steps_are_five(engine, warm):
    n, h = 65, 5
    obs0, u0 = dev(edge_obs(n)), dev(start_point(n, h, 'outside'))
    whole, _ = launch(obs0, u0, 5, 20, 1e-2, warm)
    first, _ = launch(obs0, u0, 2, 20, 1e-2, warm)
    second, _ = launch(first['obs_io'], first['u_io'], 3, 20, 1e-2, warm, state=first['state'])
    for k in KEYS[:6]:
        assert same_bits(torch.cat([first[k], second[k]]), whole[k]), k
    assert_same(second, whole, KEYS[6:])


@pytest.mark.parametrize('warm', (0, 1))
def test_an_agent_does_not_depend_on_its_neighbours(engine, warm):
    n, h = 130, 5
    obs0, u0 = dev(edge_obs(n)), dev(start_point(n, h, 'outside'))
    whole, _ = launch(obs0, u0, 3, 20, 1e-2, warm)
    for i in (0, 64, 129):
        alone, _ = launch(obs0[i:i + 1].contiguous(), u0[i:i + 1].contiguous(), 3, 20, 1e-2, warm)
        for k in KEYS[:6]:
            assert same_bits(alone[k][:, 0], whole[k][:, i]), (k, i)
        assert same_bits(alone['state'][:, 0], whole['state'][:, i])
        for k in KEYS[7:]:
            assert same_bits(alone[k][0], whole[k][i]), (k, i)


def test_null_outputs_change_nothing_else(engine):
    n, h = 65, 5
    obs0, u0 = dev(edge_obs(n)), dev(start_point(n, h, 'zeros'))
    full, _ = launch(obs0, u0, 3, 20, 1e-2, 1)
    optional = ('cost_traj', 'pgnorm_traj', 'info_traj', 'done', 'done_intended')
    for null in [(k,) for k in optional] + [optional]:
        got, _ = launch(obs0, u0, 3, 20, 1e-2, 1, null=null)
        assert_same(got, full, [k for k in KEYS if k not in null])
        for k in null:                                      # (the buffer that was not handed over)
            assert (got[k] == (SENTINEL_U8 if got[k].dtype == torch.uint8 else SENTINEL)).all()


@pytest.mark.parametrize('n', (1, 63, 65))
def test_nothing_is_written_behind_the_last_agent(engine, n):
    h = 5
    obs0, u0 = dev(edge_obs(n)), dev(start_point(n, h, 'zeros'))
    got, tails = launch(obs0, u0, 3, 20, 1e-2, 1, pad=1)
    plain, _ = launch(obs0, u0, 3, 20, 1e-2, 1)
    assert_same(got, plain)
    for k, t in tails.items():
        assert t.numel() > 0 and (t == (SENTINEL_U8 if t.dtype == torch.uint8 else SENTINEL)).all(), k


# ---- the warm start earns its keep -----------------------------------------------------------------------------------------------
def test_the_warm_start_saves_iterations_and_keeps_the_closed_loop(engine):
    """8 agents of the reset law, 6 steps, horizon 25, iters 200, tol 1e-2.  The float32 oracle loop (tests/mpc_oracle.spg_solve and the
    oracle env) accepts 0.56 times the cold start's iterations with the shifted plan on exactly these inputs, and its mean reward sums
    differ by 0.003; the bars are 0.8 and 0.02."""
    obs0 = dev(PathTrackingEnvOracle(8).reset(rng=np.random.RandomState(0)))
    u0 = dev(start_point(8, 25, 'zeros'))
    cold, _ = launch(obs0, u0, 6, 200, 1e-2, 0)
    warm, _ = launch(obs0, u0, 6, 200, 1e-2, 1)
    assert (cold['info_traj'] >= 0).all() and (warm['info_traj'] >= 0).all()      # no failed search: info counts accepted iterations
    it_cold, it_warm = int(cold['info_traj'].sum()), int(warm['info_traj'].sum())
    rew_cold, rew_warm = float(cold['rew_traj'].double().sum(0).mean()), float(warm['rew_traj'].double().sum(0).mean())
    print('accepted iterations: cold %d, warm %d (ratio %.3f); mean reward sums: cold %.4f, warm %.4f' %
          (it_cold, it_warm, it_warm / it_cold, rew_cold, rew_warm))
    assert it_warm <= 0.8 * it_cold
    assert abs(rew_warm - rew_cold) < 0.02
    assert same_bits(warm['plan_traj'][0], cold['plan_traj'][0]) and same_bits(warm['info_traj'][0], cold['info_traj'][0])     # the first solve is cold


# ---- the wrappers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('warm', (False, True))
def test_mpc_rollout_wraps_the_entry_point(engine, warm):
    n, h = 65, 5
    obs0, u0 = dev(edge_obs(n)), dev(start_point(n, h, 'outside'))
    want, _ = launch(obs0, u0, 3, 20, 1e-2, warm)
    env = fresh_env(obs0)
    before = u0.clone()
    out = M.mpc_rollout(env, u0, 3, h, iters=20, tol=1e-2, warm_start=warm)
    assert same_bits(u0, before) and same_bits(env.obs, want['obs_io']) and env.obs is not obs0
    for got, k in zip(out, ('obs_traj', 'plan_traj', 'rew_traj', 'cost_traj', 'pgnorm_traj', 'info_traj', 'u_io')):
        assert same_bits(got, want[k]), k
    assert same_bits(env._state, want['state']) and same_bits(env.done, want['done']) and same_bits(env.done_intended, want['done_intended'])
    assert same_bits(env.reward, want['rew_traj'][-1])


@pytest.mark.parametrize('warm', (False, True))
def test_run_mpc_one_launch_is_run_mpc(engine, warm):
    """iters = 500: chunks of 2048 // 500 = 4 steps, so 4 + 1"""
    from mpg_amd.policy import PolicyWithQs
    policy = PolicyWithQs(6, 2, init_seed=3, device=DEV)
    loop = M.run_mpc(policy, num_agent=2, steps=5, horizon=5, seed=11, iters=500, warm_start=warm)
    one = M.run_mpc(policy, num_agent=2, steps=5, horizon=5, seed=11, iters=500, one_launch=True, warm_start=warm)
    assert sorted(loop) == sorted(one) == sorted(('mpc_obs', 'rl_obs', 'mpc_action', 'rl_action', 'rl_action_mpc', 'mpc_rew', 'rl_rew'))
    for k in loop:
        assert same_bits(one[k], loop[k]), k
    assert (one['mpc_rew'][0] == 0).all() and (one['rl_rew'][0] == 0).all() and (one['mpc_rew'][1:] != 0).all()


def test_wrappers_raise_mpg_error(engine):
    from mpg_amd.policy import PolicyWithQs
    obs0 = dev(edge_obs(3))
    env = fresh_env(obs0)
    u = torch.zeros(3, 5, 2, device=DEV)
    with pytest.raises(L.MpgError, match='mpg_mpc_rollout: steps \\* iters = 2200'):
        M.mpc_rollout(env, u, 11, 5, iters=200)
    with pytest.raises(L.MpgError, match='mpg_mpc_rollout: steps >= 1'):
        M.mpc_rollout(env, u, 0, 5)
    with pytest.raises(L.MpgError, match='mpg_mpc_rollout: tol negative or NaN'):
        M.mpc_rollout(env, u, 2, 5, tol=-1.)
    assert same_bits(env.obs, obs0)                          # a refusal leaves the env where it was
    policy = PolicyWithQs(6, 2, init_seed=3, device=DEV)
    with pytest.raises(L.MpgError, match='mpg_mpc_rollout: iters <= 1000'):
        M.run_mpc(policy, num_agent=2, steps=3, horizon=5, iters=1001, one_launch=True)
    with pytest.raises(L.MpgError, match='mpg_mpc_rollout: horizon <= 31'):
        M.run_mpc(policy, num_agent=2, steps=3, horizon=32, iters=10, one_launch=True)
