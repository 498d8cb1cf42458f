"""What makes tests/test_model_rollout_gpu.py worth running, by the oracle alone (CPU; tests/model_rollout_oracle.py):

  * the restated step reproduces the chains of the three fixtures of the unmodified reference (model_rollout_ref.npz,
    pendulum_model_ref.npz, double_pendulum_model_ref.npz) when fed their actions, in float64 and in float32;
  * the single-step edge rows reach what they are chosen to reach - v_x clamped at both ends of [1, 35], the heading error wrapped
    across +pi and across -pi, a pendulum angle beyond +pi and beyond -pi - with no raw value within 1e-3 of a threshold, so a float32
    step falls on the same side as the float64 one;
  * the float32 oracle sits at least 4 x inside every bar of the device test: teacher-forced and free-running on the fixtures under
    tests/yardstick.check_values (this file DECIDES per model whether the free-running comparison is gated there: FREE_RUNNING_GATED),
    and as the float32 reference of the edge steps and of the closed loops, 4 x inside check_values' 1e-4;
  * a PathTracking step without the clamp, or without the wrap, misses those bars - in the single edge step and along the closed loop.

Every figure is printed before anything is asserted."""
import numpy as np
import pytest
import torch

from tests import model_edge_inputs as E
from tests import model_rollout_oracle as M
from tests import yardstick as Y

INSIDE = 4.                 # the float32 oracle's margin to every bar
BAR = 1e-4                  # check_values' bar on the distance to the float32 reference


def allowance_used(got, ref32, ref64):
    """the larger of check_values' two ratios, error / allowance: <= 1 passes"""
    e_ref, e_got = Y.rel_l2(ref32, ref64), Y.rel_l2(got, ref64)
    return max(e_got / (4. * e_ref + Y.FLOOR), Y.rel_l2(got, ref32) / BAR)


# the models whose FREE-RUNNING float32 oracle chain stays 4 x inside check_values on its fixture: the device test gates the same chain
# there and only prints it elsewhere.  Decided here by test_float32_oracle_on_the_fixtures, which fails if this set is not the outcome.
FREE_RUNNING_GATED = (M.PT, M.PD, M.DPEND)


@pytest.mark.parametrize('env_id', [M.PT, M.PD, M.DPEND])
def test_restated_step_reproduces_the_fixture_chain(golden, env_id):
    """float64 against the reference's float64 chain: 1e-9 relative L2, the bar of the restatements (tests/test_double_pendulum.py) -
    the double pendulum's per-step atan2 of its own sines and cosines returns the angle to one rounding (2e-16), which 25 steps of a
    falling pendulum do not amplify by 1e7; float32 against the float32 chain under check_values"""
    g, ocfg = golden(M.FIXTURES[env_id]), M.ocfg_of(env_id)
    o64, r64 = M.free_running(g, ocfg, torch.float64)
    e = max(Y.rel_l2(o64, g['obs_f64']), Y.rel_l2(r64, g['reward_f64']))
    print('%s float64 chain vs the reference\'s: %.2e' % (env_id, e))
    assert e <= 1e-9, e
    o32, r32 = M.free_running(g, ocfg, torch.float32)
    Y.check_values(o32, g['obs'], g['obs_f64'], 'obs')
    Y.check_values(r32, g['reward'], g['reward_f64'], 'reward')
    if env_id == M.DPEND:      # the model observations' last three entries are zeros whatever the start observation held
        assert np.abs(g['obs0'][:, 8:]).min() > 0 and not o32[:, :, 8:].any()


@pytest.mark.parametrize('env_id', [M.PT, M.PD, M.DPEND])
def test_float32_oracle_on_the_fixtures(golden, env_id):
    g, ocfg = golden(M.FIXTURES[env_id]), M.ocfg_of(env_id)
    used = {}
    for name, run in (('teacher-forced', M.teacher_forced), ('free-running', M.free_running)):
        o, r = run(g, ocfg, torch.float32)
        used[name] = max(allowance_used(o, g['obs'], g['obs_f64']), allowance_used(r, g['reward'], g['reward_f64']))
        print('%s %-14s float32 oracle uses %.3f of its allowance (1 / %g = %.3f)' % (env_id, name, used[name], INSIDE, 1. / INSIDE))
    assert used['teacher-forced'] <= 1. / INSIDE, used
    assert (used['free-running'] <= 1. / INSIDE) == (env_id in FREE_RUNNING_GATED), used


def raw_values(ocfg, obs, act, eps):
    log = []
    m = E.EdgePathTrackingModel(ocfg.obs_dim - 6, log=log)
    m.reset(torch.as_tensor(obs).double())
    m.rollout_out(torch.as_tensor(act).double(), torch.as_tensor(eps).double())
    return log[0]


@pytest.mark.parametrize('env_id,K,rows', M.EDGE_STEP_CASES)
def test_edge_rows_reach_their_branches(env_id, K, rows):
    ocfg, obs, act, eps = M.edge_step_case(env_id, K, rows)
    assert obs.shape == (rows, ocfg.obs_dim)
    o64, r64 = M.edge_step_reference(env_id, K, rows)
    o32, r32 = M.edge_step_reference(env_id, K, rows, f64=False)
    own = max(Y.rel_l2(o32, o64), Y.rel_l2(r32, r64))
    if env_id == M.PT:
        vx, dphi = raw_values(ocfg, obs, act, eps)
        c = dict(hi=int((vx > 35.).sum()), lo=int((vx < 1.).sum()), down=int((dphi > np.pi).sum()), up=int((dphi <= -np.pi).sum()),
                 near_vx=float(np.minimum(np.abs(vx - 1.), np.abs(vx - 35.)).min()), near_dphi=float(np.abs(np.abs(dphi) - np.pi).min()))
        print('pt K %d rows %d: %s   float32 oracle vs float64 %.1e' % (K, rows, c, own))
        assert c['hi'] >= 2 and c['lo'] >= 2 and c['down'] >= 1 and c['up'] >= 1, c
        assert c['near_vx'] >= 1e-3 and c['near_dphi'] >= 1e-3, c
        assert (o64[:, 0] == 15.).sum() == c['hi'] and (o64[:, 0] == -19.).sum() == c['lo']
        assert np.abs(obs[:, 4]).max() > 3.3 and np.abs(o64[:, 4]).max() <= np.pi       # unwrapped on the way in, wrapped on the way out
        if K:
            assert (obs[:, 6:] != obs[:, 3:4]).all() and (o64[:, 6:] == o64[:, 3:4]).all()
    else:
        beyond = (int((o64[:, 1] > np.pi).sum()), int((o64[:, 1] < -np.pi).sum()))
        print('pendulum rows %d: angles beyond +pi / -pi %s   float32 oracle vs float64 %.1e' % (rows, beyond, own))
        assert min(beyond) >= 1 and np.abs(obs[:, 1]).max() < np.pi, beyond
    assert own <= BAR / INSIDE, own


@pytest.mark.parametrize('env_id,K', M.LOOP_CASES)
def test_float32_closed_loop_is_inside_the_bar(env_id, K):
    a, b = M.loop_reference(env_id, K), M.loop_reference(env_id, K, f64=False)
    e = {nm: Y.rel_l2(y, x) for nm, x, y in zip(('obs_traj', 'act_traj', 'rew_traj', 'last_obs'), a, b)}
    print('%s K %d: float32 closed loop vs float64 %s' % (env_id, K, '  '.join('%s %.1e' % kv for kv in e.items())))
    assert max(e['obs_traj'], e['rew_traj']) <= BAR / INSIDE, e
    assert a[0].shape == (M.LOOP_STEPS, M.LOOP_ROWS, M.loop_case(env_id, K)[0].obs_dim)
    assert np.array_equal(a[0][0], M.loop_case(env_id, K)[2].astype(np.float64))
    assert np.isfinite(a[0]).all() and np.isfinite(a[2]).all()


@pytest.mark.parametrize('variant', sorted(M.VARIANTS))
@pytest.mark.parametrize('K,rows', [(0, 48), (3, 17)])
def test_a_step_without_a_branch_misses_the_bars(variant, K, rows):
    """the allowance of check_values on the edge step, 4 x the float32 oracle's error + 1e-6, and its 1e-4: both missed; along the
    closed loop of the K-entry case as well"""
    ocfg, obs, act, eps = M.edge_step_case(M.PT, K, rows)
    o64, _ = M.edge_step_reference(M.PT, K, rows)
    o32, _ = M.edge_step_reference(M.PT, K, rows, f64=False)
    wrong, _ = M.step(ocfg, obs, act, eps, torch.float64, variant)
    used = allowance_used(wrong, o32, o64)
    lcfg, wp, obs0, leps = M.loop_case(M.PT, K)
    loop = M.closed_loop(lcfg, wp, obs0, M.LOOP_STEPS, leps, torch.float64, variant=variant)
    ref64, ref32 = M.loop_reference(M.PT, K), M.loop_reference(M.PT, K, f64=False)
    used_loop = min(allowance_used(loop[0], ref32[0], ref64[0]), allowance_used(loop[2], ref32[2], ref64[2]))
    print('%s, K %d: the edge step uses %.0f x its allowance, the closed loop at least %.0f x' % (variant, K, used, used_loop))
    assert used >= 20. and used_loop >= 20., (used, used_loop)
