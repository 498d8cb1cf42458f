"""tests/mpc_oracle.py against the UNMODIFIED reference's mpc/main.py, through tests/golden/mpc_ref.npz (make_golden_mpc.py), without a
GPU: the restated cost, its autograd gradient against central differences of the reference's cost, the clamp's gate on the edge rows,
and the oracle solver against the reference's own SLSQP solutions."""
import os

import numpy as np
import pytest
import torch

from tests import mpc_oracle as MO

GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'mpc_ref.npz')
HORIZONS = (1, 2, 25, 31)
SLSQP_HORIZONS = (25, 5, 10)
MARGIN = 1e-4


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def slsqp_states(gold, h):
    """the start states of the SLSQP part at horizon h"""
    return gold['slsqp_x0'] if h == 25 else gold['slsqp_x0'][gold['slsqp_short_rows']]


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize('h', HORIZONS)
def test_restated_cost_equals_the_references(gold, h):
    want = gold['cost_h%d' % h]
    got = MO.horizon_cost(t(gold['x0']), t(gold['u_h%d' % h])).numpy()
    assert want.shape == (64,) and np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), np.abs(got - want).max()


def test_restated_cost_on_the_edge_rows(gold):
    want = gold['edge_cost']
    got, traj = MO.horizon_cost(t(gold['edge_x0']), t(gold['edge_u']), return_traj=True)
    assert np.all(np.abs(got.numpy() - want) <= 1e-12 * np.abs(want))
    names = list(gold['edge_names'])
    traj = traj.numpy()
    # the rows take the branches they were built for
    assert (traj[names.index('vx_1.2_full_braking'), 1:, 0] == 1.).sum() >= 5
    assert (traj[names.index('vx_34.9_full_throttle'), 1:, 0] == 35.).sum() >= 5
    up, down = traj[names.index('dphi_near_plus_pi_positive_r'), :, 4], traj[names.index('dphi_near_minus_pi_negative_r'), :, 4]
    assert up[0] > 3.13 and up[1] < -3.1 and down[0] < -3.13 and down[1] > 3.1            # wrapped at the first step
    assert set(np.unique(gold['edge_u'][names.index('controls_on_the_bounds')])) == {-1., 0., 1.}


def test_autograd_gradient_against_central_differences_of_the_references_cost(gold):
    """central differences with a step of 1e-6 in float64 are good to about 1e-8; 1e-5 relative L2 per row catches a wrong term"""
    rows = gold['fd_rows']
    _, g = MO.cost_and_grad(t(gold['x0'][rows]), t(gold['u_h25'][rows]))
    g, fd = g.numpy().reshape(len(rows), 50), gold['fd_grad']
    err = np.linalg.norm(g - fd, axis=1) / np.linalg.norm(fd, axis=1)
    print('relative L2 per row', err)
    assert np.all(err <= 1e-5), err


@pytest.mark.parametrize('h', HORIZONS)
def test_hand_adjoint_equals_autograd(gold, h):
    """what the oracle solver iterates on: the same cost bit for bit, the gradient to 1e-12 relative L2 per row, on the random rows and
    (horizon 25) the edge rows; exact zeros where autograd has them"""
    x0, u = gold['x0'], gold['u_h%d' % h]
    if h == 25:
        x0, u = np.concatenate([x0, gold['edge_x0']]), np.concatenate([u, gold['edge_u']])
    f, g = MO.cost_and_grad(t(x0), t(u))
    fa, ga = MO.cost_and_grad_adjoint(t(x0), t(u))
    assert torch.equal(f, fa)
    err = (g - ga).flatten(1).norm(dim=1) / g.flatten(1).norm(dim=1)
    assert (err <= 1e-12).all(), err.max()
    assert ((ga == 0) == (g == 0)).all()


def test_a_clamped_speed_passes_no_gradient_on_the_edge_rows(gold):
    """with the controls' own penalty left out, an acceleration whose step ends on the v_x clamp can reach the cost through nothing
    else: its gradient is EXACTLY zero (np.clip's derivative outside its bounds); so is the last step's pair, which feeds no later
    state.  The unclamped entries beside them are not zero."""
    x0, u = t(gold['edge_x0']), t(gold['edge_u'])
    _, traj = MO.horizon_cost(x0, u, return_traj=True)
    _, g = MO.cost_and_grad(x0, u, control_penalty=False)
    s = traj[:, :-1]
    raw = s[:, :, 0] + MO.TAU * (u[:, :, 1] * MO.ACC_SCALE + s[:, :, 1] * s[:, :, 2])
    clamped = (raw < 1) | (raw > 35)
    assert clamped[0].sum() >= 5 and clamped[1].sum() >= 5 and not clamped[2:].any()
    assert (g[:, :, 1][clamped] == 0).all()
    assert (g[:, -1, :] == 0).all()
    free = ~clamped
    free[:, -1] = False
    assert (g[:, :, 1][free] != 0).all() and (g[:, :-1, 0] != 0).all()
    # the full gradient there is the penalty's alone
    _, gf = MO.cost_and_grad(x0, u)
    np.testing.assert_allclose(gf[:, :, 1][clamped].numpy(), (2 * 0.05 * MO.ACC_SCALE ** 2 * u[:, :, 1])[clamped].numpy(), rtol=1e-15)


@pytest.fixture(scope='module')
def solved(gold):
    return {h: MO.spg_solve(t(slsqp_states(gold, h)), horizon=h, iters=200) for h in SLSQP_HORIZONS}


@pytest.mark.parametrize('h', SLSQP_HORIZONS)
def test_oracle_solver_ends_below_the_references_slsqp(gold, solved, h):
    """every SLSQP solve of the reference succeeded, and the float64 oracle solver at 200 iterations ends at least 1e-4 below its cost
    on every row (what the generator asserted when it wrote the fixture)"""
    assert gold['success_h%d' % h].all() and len(gold['cost_slsqp_h%d' % h]) == (16 if h == 25 else 4)
    u, f, pg, info = solved[h]
    # the stored SLSQP cost is the restated cost at the stored solution
    at = MO.horizon_cost(t(slsqp_states(gold, h)), t(gold['u_slsqp_h%d' % h])).numpy()
    assert np.all(np.abs(at - gold['cost_slsqp_h%d' % h]) <= 1e-12 * np.abs(at))
    gap = gold['cost_slsqp_h%d' % h] - f.numpy()
    print('SLSQP - oracle', gap)
    assert np.all(gap >= MARGIN), gap
    # ... and reproduces the end cost the generator stored (the GPU tests take it as the optimum instead of solving again)
    stored = gold['cost_oracle_h%d' % h]
    assert np.all(np.abs(f.numpy() - stored) <= 1e-9 * np.maximum(1., np.abs(stored))), np.abs(f.numpy() - stored).max()
    assert (u.abs() <= 1).all()
    assert np.all(np.abs(MO.horizon_cost(t(slsqp_states(gold, h)), u).numpy() - f.numpy()) == 0)


def test_oracle_solver_is_bit_identical_between_two_runs(gold, solved):
    again = MO.spg_solve(t(slsqp_states(gold, 5)), horizon=5, iters=200)
    for a, b in zip(solved[5], again):
        assert torch.equal(a, b)


def test_oracle_solver_conventions(gold):
    """iters 0 returns the clamped start point; tol stops a row with info = its accepted steps; a NaN row fails its first search"""
    x0 = t(gold['slsqp_x0'][:3].copy())
    start = torch.full((3, 5, 2), 1.5, dtype=torch.float64)
    u, f, pg, info = MO.spg_solve(x0, u_init=start, horizon=5, iters=0)
    assert (u == 1).all() and info.tolist() == [0, 0, 0] and torch.equal(f, MO.horizon_cost(x0, u))
    u, f, pg, info = MO.spg_solve(x0, horizon=5, iters=200, tol=1e-3)
    assert (pg <= 1e-3).all() and (info > 0).all() and (info < 200).all()
    x0[1, 3] = float('nan')
    un, fn, pgn, infon = MO.spg_solve(x0, horizon=5, iters=200, tol=1e-3)
    assert infon[1] == -1 and torch.equal(un[[0, 2]], u[[0, 2]]) and torch.equal(fn[[0, 2]], f[[0, 2]])
