"""mpg_mpc_cost_grad, mpg_mpc_solve and run_mpc on the GPU, on both engines.

Cost, gradient and states against the float64 oracle (tests/mpc_oracle.py, pinned to the reference by tests/test_mpc_golden.py) from the
same float32-rounded inputs, at the bar tests/test_rollout_gpu.py holds the model rollouts to: 5e-5 relative L2 per array.  The solver
against the reference's own SLSQP solutions and against the float32 emulation of the same method (the project's factor-4 rule), and its
invariants bit for bit.  Floats are compared as their 32-bit patterns where bit-identity is the claim.

Measured on an MI355X (both engines alike; printed by the tests before they assert):
    cost / gradient / states, worst relative L2 over all cases       2.4e-7 / 2.9e-7 / 2.6e-7 (bar 5e-5)
    float64 cost at the device's solution minus the optimum           at most 3.6e-7 at horizon 25 (the float32 emulation: 6.0e-7)"""
import math
import os

import numpy as np
import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import mpc as M
from tests import mpc_oracle as MO

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'mpc_ref.npz')
BAR = 5e-5
ROWS = (1, 63, 64, 65, 130)          # one lane, the wave's edge, two workgroups with a tail
HORIZONS = (1, 2, 25, 31)
SLSQP_HORIZONS = (25, 5, 10)


@pytest.fixture(params=['split', 'f32'])
def engine(request):
    """both builds of the library (mpg_amd/_lib.py ENGINES); the code has no matrix instruction and is the same in both"""
    with L.engine(request.param):
        yield request.param


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def rel_l2(got, want):
    got, want = got.double().cpu().reshape(-1), want.double().reshape(-1)
    return float((got - want).norm() / want.norm())


def pool(gold, h, rows):
    """`rows` problems at horizon h, float32-rounded: the 5 edge rows first (their controls cut or repeated to h steps), then the fixture's
    64 random rows, cycled; each further cycle with delta_y moved, so that no two rows are the same problem"""
    eu = gold['edge_u']
    eu = eu[:, :h] if h <= eu.shape[1] else np.concatenate([eu, eu[:, :h - eu.shape[1]]], 1)
    x0 = np.concatenate([gold['edge_x0'], gold['x0']])
    u = np.concatenate([eu, gold['u_h%d' % h]])
    idx = np.arange(rows) % len(x0)
    x0, u = x0[idx].copy(), u[idx].copy()
    x0[:, 3] += 0.25 * (np.arange(rows) // 69)
    return x0.astype(np.float32), u.astype(np.float32)


# ---- cost, gradient, states ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h', HORIZONS)
@pytest.mark.parametrize('rows', ROWS)
def test_cost_grad_and_states_against_the_float64_oracle(engine, gold, rows, h):
    x0, u = pool(gold, h, rows)
    cost, grad, traj = M.mpc_cost_grad(dev(x0), dev(u), want_grad=True, want_traj=True)
    x64, u64 = torch.from_numpy(x0).double(), torch.from_numpy(u).double()
    want_cost, want_traj = MO.horizon_cost(x64, u64, return_traj=True)
    _, want_grad = MO.cost_and_grad(x64, u64)
    e_cost, e_grad = rel_l2(cost, want_cost), rel_l2(grad, want_grad)
    print('rows %d horizon %d: cost %.3g grad %.3g' % (rows, h, e_cost, e_grad))
    assert e_cost <= BAR and e_grad <= BAR
    # exact zeros of the oracle are exact zeros on the device
    zero = want_grad == 0
    assert (grad.cpu()[zero] == 0).all()
    if h == 25 and rows >= 5:
        assert zero[4, -1, 1] and zero.sum() >= 2          # (the row with zeros behind its +-1 controls)
    # the states, column by column; the wrapped angle modulo 2 pi
    got = traj.double().cpu()
    assert got.shape == (rows, h + 1, 6)
    for c in range(6):
        d = got[:, :, c] - want_traj[:, :, c]
        if c == 4:
            d = torch.remainder(d + math.pi, 2 * math.pi) - math.pi
        e = float(d.norm() / want_traj[:, :, c].norm())
        print('   state column %d: %.3g' % (c, e))
        assert e <= BAR
    for bound in (1., 35.):
        on = want_traj[:, :, 0] == bound
        assert (got[:, :, 0][on] == bound).all()
    if rows >= 2 and h >= 2:
        assert (want_traj[0, 1:, 0] == 1.).all() and (want_traj[1, 1:, 0] == 35.).all()     # the clamp rows hold their clamp


@pytest.mark.parametrize('h', (1, 25, 31))
def test_cost_is_the_same_bits_without_gradient_or_states_and_between_two_launches(engine, gold, h):
    x0, u = pool(gold, h, 130)
    x0, u = dev(x0), dev(u)
    full = M.mpc_cost_grad(x0, u, want_grad=True, want_traj=True)
    again = M.mpc_cost_grad(x0, u, want_grad=True, want_traj=True)
    for a, b in zip(full, again):
        assert same_bits(a, b)
    assert same_bits(M.mpc_cost_grad(x0, u, want_grad=False, want_traj=False)[0], full[0])
    g_only = M.mpc_cost_grad(x0, u, want_grad=True, want_traj=False)
    t_only = M.mpc_cost_grad(x0, u, want_grad=False, want_traj=True)
    assert same_bits(g_only[0], full[0]) and same_bits(g_only[1], full[1]) and g_only[2] is None
    assert same_bits(t_only[0], full[0]) and same_bits(t_only[2], full[2]) and t_only[1] is None


def test_arrays_behind_the_last_row_are_not_written(engine, gold):
    """65 rows launch two workgroups; the second one's 63 idle lanes store nothing"""
    x0, u = pool(gold, 25, 65)
    cost = torch.full((128,), -7., device=DEV)
    grad = torch.full((128, 25, 2), -7., device=DEV)
    traj = torch.full((128, 26, 6), -7., device=DEV)
    L.call('mpg_mpc_cost_grad', L.c_int(65), L.c_int(25), L.ptr(dev(x0)), L.ptr(dev(u)), L.ptr(cost), L.ptr(grad), L.ptr(traj), L.stream())
    assert (cost[65:] == -7).all() and (grad[65:] == -7).all() and (traj[65:] == -7).all()
    assert (cost[:65] != -7).all()


# ---- the solver ------------------------------------------------------------------------------------------------------------------
def slsqp_states(gold, h):
    return gold['slsqp_x0'] if h == 25 else gold['slsqp_x0'][gold['slsqp_short_rows']]


@pytest.fixture(scope='module')
def emulation(gold):
    """the float32 emulation's solutions at 200 iterations, once for the module: {h: u [n, h, 2] float64}"""
    return {h: MO.spg_solve(torch.from_numpy(slsqp_states(gold, h)).float(), horizon=h, iters=200, dtype=torch.float32)[0].double()
            for h in SLSQP_HORIZONS}


@pytest.mark.parametrize('h', SLSQP_HORIZONS)
def test_solver_against_slsqp_and_the_float32_emulation(engine, gold, emulation, h):
    x64 = torch.from_numpy(slsqp_states(gold, h))
    x0 = dev(slsqp_states(gold, h))
    mpc = M.ModelPredictiveControl(x0, h)
    u, cost, pg, info = mpc.solve(iters=200)
    assert (u.abs() <= 1).all()
    # the reference's float64 cost (the oracle's, pinned equal) at the device's solution against the reference's own SLSQP
    at_dev = MO.horizon_cost(x64, u.double().cpu())
    slsqp = torch.from_numpy(gold['cost_slsqp_h%d' % h])
    print('horizon %d: SLSQP - device %s' % (h, (slsqp - at_dev).numpy()))
    assert (at_dev <= slsqp).all()
    # the gap to the float64 optimum against the float32 emulation's: factor 4 and a floor of 1e-5 max(1, cost)
    best = torch.from_numpy(gold['cost_oracle_h%d' % h])
    gap_dev, gap_emu = at_dev - best, MO.horizon_cost(x64, emulation[h]) - best
    print('horizon %d: device gap max %.3g, emulation gap max %.3g; info %s' % (h, gap_dev.max(), gap_emu.max(), info.tolist()))
    assert (gap_dev <= 4 * gap_emu.clamp(min=0) + 1e-5 * best.clamp(min=1)).all()
    # cost_out is mpg_mpc_cost_grad's at the returned point
    assert same_bits(cost, mpc.cost_function(u))
    # and again: the same bits
    for a, b in zip((u, cost, pg, info), mpc.solve(iters=200)):
        assert same_bits(a, b)


def test_no_iterations_return_the_clamped_start_point_and_its_cost(engine, gold):
    x0 = dev(gold['slsqp_x0'])
    rng = np.random.default_rng(5)
    start = dev(rng.uniform(-2, 2, (16, 25, 2)))
    mpc = M.ModelPredictiveControl(x0, 25)
    u, cost, pg, info = mpc.solve(u_init=start, iters=0)
    assert same_bits(u, start.clamp(-1, 1)) and (info == 0).all()
    c, g = mpc.cost_and_gradient(u)
    assert same_bits(cost, c)
    assert same_bits(pg, ((u - g).clamp(-1, 1) - u).abs().flatten(1).amax(1))
    assert (start.abs() > 1).any() and same_bits(start, dev(np.random.default_rng(5).uniform(-2, 2, (16, 25, 2))))     # the start is left alone


def test_rows_do_not_depend_on_their_neighbours(engine, gold):
    """130 rows in one launch against rows 0..63, 64..127 and 128..129 in three: any coupling between lanes through the wave-uniform
    exits of the line search would show"""
    x0, _ = pool(gold, 25, 130)
    x0 = dev(x0)
    zeros = torch.zeros(130, 25, 2, device=DEV)
    whole = M.mpc_solve(x0, zeros, iters=200)
    assert len(set(whole[3].tolist())) > 4                                  # the rows stop at different iterations
    for lo, hi in ((0, 64), (64, 128), (128, 130)):
        part = M.mpc_solve(x0[lo:hi].contiguous(), zeros[lo:hi].contiguous(), iters=200)
        for a, b in zip(whole, part):
            assert same_bits(a[lo:hi], b)


def test_a_nan_row_fails_its_search_and_leaves_its_neighbours_alone(engine, gold):
    x0, _ = pool(gold, 25, 64)
    x0 = dev(x0)
    zeros = torch.zeros(64, 25, 2, device=DEV)
    clean = M.mpc_solve(x0, zeros, iters=200)
    bad = x0.clone()
    bad[7, 3] = float('nan')
    bad[40, 0] = float('nan')
    got = M.mpc_solve(bad, zeros, iters=200)
    assert got[3][7] == -1 and got[3][40] == -1
    assert (got[0][[7, 40]] == 0).all()                                       # the last accepted point: the start
    keep = [i for i in range(64) if i not in (7, 40)]
    for a, b in zip(clean, got):
        assert same_bits(a[keep], b[keep])


@pytest.mark.parametrize('h', SLSQP_HORIZONS)
def test_a_tolerance_stops_every_fixture_row_early(engine, gold, h):
    x0 = dev(slsqp_states(gold, h))
    u, cost, pg, info = M.ModelPredictiveControl(x0, h).solve(iters=200, tol=1e-3)
    print('horizon %d: info %s pgnorm max %.3g' % (h, info.tolist(), pg.max()))
    assert (pg <= 1e-3).all() and (info > 0).all() and (info < 200).all()


def test_one_row_forms(engine, gold):
    """[6] in: a Python float from cost_function, as the reference returns, and [horizon, 2] controls"""
    x0 = dev(gold['slsqp_x0'])
    one = M.ModelPredictiveControl(x0[3], 10)
    u, cost, pg, info = one.solve(iters=50)
    assert u.shape == (10, 2) and cost.dim() == 0 and info.dim() == 0
    f = one.cost_function(u.reshape(-1))
    assert isinstance(f, float) and np.float32(f) == cost.item()
    ub, cb, _, _ = M.ModelPredictiveControl(x0, 10).solve(iters=50)
    assert same_bits(ub[3], u) and same_bits(cb[3], cost)
    c, g = one.cost_and_gradient(u)
    assert g.shape == u.shape and same_bits(c, cost)


def test_wrappers_raise_mpg_error(engine, gold):
    x0 = dev(gold['slsqp_x0'])
    with pytest.raises(L.MpgError, match='mpg_mpc_solve: iters <= 1000'):
        M.ModelPredictiveControl(x0, 25).solve(iters=1001)
    with pytest.raises(L.MpgError, match='mpg_mpc_solve: tol negative or NaN'):
        M.ModelPredictiveControl(x0, 25).solve(tol=-1.)
    with pytest.raises(L.MpgError, match='mpg_mpc_cost_grad: horizon <= 31'):
        M.ModelPredictiveControl(x0, 32).cost_function(torch.zeros(16, 32, 2, device=DEV))


# ---- the closed loop -------------------------------------------------------------------------------------------------------------
def test_run_mpc_is_the_chain_of_solve_env_step_and_policy_action(engine):
    from mpg_amd.envs import PathTrackingEnv
    from mpg_amd.policy import PolicyWithQs
    policy = PolicyWithQs(6, 2, init_seed=3, device=DEV)
    rec = M.run_mpc(policy, num_agent=2, steps=3, horizon=5, seed=11, iters=200)
    assert {k: tuple(v.shape) for k, v in rec.items()} == dict(mpc_obs=(3, 2, 6), rl_obs=(3, 2, 6), mpc_action=(3, 2, 5, 2), rl_action=(3, 2, 2),
                                                               rl_action_mpc=(3, 2, 2), mpc_rew=(3, 2), rl_rew=(3, 2))
    assert same_bits(rec['rl_obs'][0], rec['mpc_obs'][0])
    # by hand
    e_mpc, e_rl = PathTrackingEnv(num_agent=2, device=DEV, seed=11), PathTrackingEnv(num_agent=2, device=DEV, seed=11)
    obs = e_mpc.reset()
    obs_rl = e_rl.reset(init_obs=obs.clone())
    rew, rew_rl = torch.zeros(2, device=DEV), torch.zeros(2, device=DEV)
    for t in range(3):
        x0 = obs.clone()
        x0[:, 0] += 20.
        plan = M.mpc_solve(x0, torch.zeros(2, 5, 2, device=DEV), iters=200)[0]
        a_mpc, a_rl = policy.compute_action(obs)[0], policy.compute_action(obs_rl)[0]
        for k, v in (('mpc_obs', obs), ('rl_obs', obs_rl), ('mpc_action', plan), ('rl_action', a_rl), ('rl_action_mpc', a_mpc), ('mpc_rew', rew),
                     ('rl_rew', rew_rl)):
            assert same_bits(rec[k][t], v), (k, t)
        obs, rew, _, _ = e_mpc.step(plan[:, 0, :].contiguous())
        obs_rl, rew_rl, _, _ = e_rl.step(a_rl)
    assert (rec['mpc_rew'][1:] != 0).all() and (rec['mpc_rew'][0] == 0).all()
    assert not same_bits(rec['rl_obs'][2], rec['mpc_obs'][2])               # the two loops part ways
