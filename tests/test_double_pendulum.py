"""InvertedDoublePendulum-v2 without a GPU: the restated model, its closed-form adjoint and NADP on it (tests/dp_oracle.py) against
the fixtures of the unmodified reference (tests/golden/make_golden_dp.py) and against autograd; the cfg of the env id and the
refusals of the C ABI (every entry point validates before it touches the device)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import dp_oracle as DP
from tests import yardstick as Y
from mpg_amd import _lib as L
from mpg_amd import ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NETS = [('Q1', 12, 1), ('policy', 11, 2)]
STATS = ('q_loss', 'policy_loss', 'value_mean', 'q_gradient_norm', 'policy_gradient_norm')


# ---- model -----------------------------------------------------------------------------------------------------------------
def _run_model(g, dt):
    m = DP.DoublePendulumModelOracle()
    m.reset(torch.as_tensor(g['obs0']).to(dt))
    s0 = m.states.numpy().copy()
    obs, rew = [], []
    for t in range(g['actions'].shape[0]):
        o, r = m.rollout_out(torch.as_tensor(g['actions'][t]).to(dt))
        obs.append(o.numpy()), rew.append(r.numpy())
    return s0, np.stack(obs), np.stack(rew), m.states.numpy()


def test_restated_model_reproduces_the_reference(golden):
    g = golden('double_pendulum_model_ref.npz')
    assert np.abs(g['state_f64'][:, 1:3]).max() > np.pi          # the fixture leaves the principal range: the angles are not wrapped
    s0, obs, rew, sT = _run_model(g, torch.float64)
    worst = 0.0
    for got, key in ((s0, 'state0'), (obs, 'obs'), (rew, 'reward'), (sT, 'state')):
        e = Y.rel_l2(got, g[key + '_f64'])
        print('float64 restatement vs reference float64, %-7s rel L2 %.3e' % (key, e))
        worst = max(worst, e)
    assert worst <= 1e-9, worst                                  # same arithmetic, same dtype (tests/test_model_vjp.py's bar)
    s0, obs, rew, sT = _run_model(g, torch.float32)
    for got, key in ((s0, 'state0'), (obs, 'obs'), (rew, 'reward'), (sT, 'state')):
        Y.check_values(got, g[key], g[key + '_f64'], what=key)
    # the model observations carry zeros in the constraint-force entries, whatever the start observation held
    assert np.abs(g['obs0'][:, 8:]).min() > 0 and not obs[:, :, 8:].any() and not g['obs'][:, :, 8:].any()


def _random_states(rng, N):
    s = rng.standard_normal((N, 6)) * np.array([0.5, 1.0, 1.0, 1.0, 3.0, 3.0])
    s[: N // 3, 1:3] = rng.uniform(-12., 12., (N // 3, 2))       # |theta| > pi: nothing wraps the angles
    s[N // 3: N // 2, 3:] *= 8.                                   # the velocities of a falling pendulum (30 rad/s and more)
    return s


def test_closed_form_step_matches_the_restated_step():
    """the kernel's cofactor solve of the 3 x 3 system against torch.linalg.inv + matmul, float64"""
    rng = np.random.Generator(np.random.PCG64(3))
    s, a = _random_states(rng, 300), rng.uniform(-1, 1, (300, 1))
    m = DP.DoublePendulumModelOracle()
    m.obses, m.states = None, torch.tensor(s)
    _, rew = m.rollout_out(torch.tensor(a))
    s2, r2 = DP.dp_model_step(s, a)
    np.testing.assert_allclose(s2, m.states.numpy(), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(r2, rew.numpy(), rtol=1e-9, atol=1e-9)


def test_double_pendulum_model_step_vjp_matches_autograd():
    rng = np.random.Generator(np.random.PCG64(4))
    N = 300
    s, a = _random_states(rng, N), rng.uniform(-1, 1, (N, 1))
    assert (np.abs(s[:, 1:3]) > np.pi).any() and np.abs(s[:, 3:]).max() > 10
    lam, rho = rng.standard_normal((N, 6)), rng.standard_normal(N)
    st, at = torch.tensor(s, requires_grad=True), torch.tensor(a, requires_grad=True)
    m = DP.DoublePendulumModelOracle()
    m.obses, m.states = None, st
    _, rew = m.rollout_out(at)
    loss = (m.states * torch.tensor(lam)).sum() + (rew * torch.tensor(rho)).sum()
    g_s, g_a = torch.autograd.grad(loss, [st, at])
    gs, ga = DP.dp_model_step_vjp(s, a, lam, rho)
    np.testing.assert_allclose(gs, g_s.numpy(), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(ga, g_a.numpy(), rtol=1e-9, atol=1e-9)


def test_feature_map_vjp_matches_autograd():
    rng = np.random.Generator(np.random.PCG64(5))
    N = 200
    s, v = _random_states(rng, N), rng.standard_normal((N, 16))
    scale = rng.uniform(0.5, 2., 11)
    st = torch.tensor(s, requires_grad=True)
    x = DP.get_obs(st) * torch.tensor(scale)
    g_s, = torch.autograd.grad((x * torch.tensor(v[:, :11])).sum(), [st])
    np.testing.assert_allclose(DP.feature_vjp(s, v[:, :11], scale), g_s.numpy(), rtol=1e-9, atol=1e-9)
    # atan2(sin, cos) gives the state back on the principal range (reset of a batch observation)
    back = DP.get_state(DP.get_obs(st).detach()).numpy()
    np.testing.assert_allclose(np.sin(back[:, 1:3]), np.sin(s[:, 1:3]), atol=1e-12)


# ---- NADP ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,n', [(32, 25), (256, 25), (32, 10), (256, 10)])
def test_restated_nadp_reproduces_the_reference(H, n):
    inp, g = DP.load_case(GOLDEN, H, n)
    cfg = DP.make_cfg(n, H=H)
    grads, st = DP.nadp_compute_gradient(cfg, DP.nets_of(cfg, inp, torch.float32), [inp['batch_obs'], inp['batch_actions']])
    got = np.concatenate([x.ravel() for x in grads])
    where = 'nadp_dp H%d n%d' % (H, n)
    if H == 256:
        worst = Y.check_gradients(got, g['grads'], g['grads_f64'], NETS, where=where, small64=g['small64'])
        print(where, 'worst error / allowance %.3f' % worst)
    else:
        DP.check_arrays(got, g['grads'], g['grads_f64'], NETS, 32, where)
    Y.check_values(st['targets'], g['targets'], g['targets_f64'], what='targets')
    for k in STATS:
        Y.check_values(st[k], g[k], g[k + '_f64'], what=k)


# ---- cfg and refusals ------------------------------------------------------------------------------------------------------
NULL, FAKE = ctypes.c_void_p(0), ctypes.c_void_p(0x1000)      # FAKE: never dereferenced - the call must be refused before any launch
I, U64, F, SZ = ctypes.c_int, ctypes.c_uint64, ctypes.c_float, ctypes.c_size_t
MPG_EINVAL = -1000
SEL2, W2 = (I * 2)(0, 25), (F * 2)(0.0, 1.0)


def _cfg(obs_dim=11, act_dim=1, env_kind=2):
    c = ops.make_cfg(DP.ENV_ID)
    c.obs_dim, c.act_dim, c.env_kind = obs_dim, act_dim, env_kind
    return c


def test_make_cfg_of_the_env_id():
    c = ops.make_cfg(DP.ENV_ID)
    assert (c.obs_dim, c.act_dim, c.env_kind) == (11, 1, 2)
    assert c.policy_out_act == ops.ACT_LINEAR and c.action_range == 1.0 and c.rew_scale == 1.0 and c.rew_shift == 0.0
    assert list(c.obs_scale)[:11] == [1.0] * 11
    from mpg_amd.envs import ENV_KIND
    assert ENV_KIND[DP.ENV_ID] == 2
    # every other id is served as before
    p, q, u = ops.make_cfg('PathTracking-v0'), ops.make_cfg('InvertedPendulumConti-v0'), ops.make_cfg('SomethingElse-v0')
    assert (p.obs_dim, p.act_dim, p.env_kind) == (6, 2, 0) and (q.obs_dim, q.act_dim, q.env_kind) == (4, 1, 1)
    assert (u.obs_dim, u.act_dim, u.env_kind) == (4, 1, 1)
    from mpg_amd import config
    a = config.default_args('NADP', env_id=DP.ENV_ID)
    assert (a.obs_dim, a.act_dim, a.action_range, a.policy_out_activation) == (11, 1, 1.0, 'linear') and a.obs_scale == [1.] * 11
    assert a.num_rollout_list_for_policy_update == [25] and a.num_rollout_list_for_q_estimation == [25]


def test_make_env_still_raises_and_says_why():
    from mpg_amd.envs import make_env
    with pytest.raises(ValueError, match='MuJoCo'):
        make_env(DP.ENV_ID, device='cpu')


def _queries(lib, c):
    return (lib.mpg_rollout_pg_workspace_bytes(ctypes.byref(c), I(4096), I(1), I(25), I(2), I(1)),
            lib.mpg_rollout_q_target_workspace_bytes(ctypes.byref(c), I(4096)),
            lib.mpg_rollout_q_estimation_workspace_bytes(ctypes.byref(c), I(4096), I(2), I(3)))


def test_workspace_queries_serve_the_model_and_refuse_every_mismatched_triple():
    lib = L.lib()
    assert lib.mpg_abi_version() == 10
    assert all(v > 0 for v in _queries(lib, _cfg()))
    for triple in ((11, 1, 1), (4, 1, 2), (11, 2, 2), (6, 2, 2), (11, 1, 0)):
        assert _queries(lib, _cfg(*triple)) == (0, 0, 0), triple


@pytest.mark.parametrize('triple', [(11, 1, 1), (4, 1, 2), (11, 2, 2)])
def test_rollout_entry_points_refuse_a_mismatched_triple(triple):
    lib, c = L.lib(), _cfg(*triple)
    ws, nb = FAKE, SZ(1 << 30)
    calls = [
        ('mpg_rollout_pg', (FAKE, FAKE, I(64), I(1), I(25), SEL2, I(2), W2, FAKE, NULL, U64(1), U64(0), F(1. / 64), I(1), FAKE, FAKE, FAKE,
                            ws, nb, NULL)),
        ('mpg_rollout_q_target', (FAKE, FAKE, I(64), I(25), FAKE, FAKE, NULL, U64(1), U64(0), FAKE, ws, nb, NULL)),
        ('mpg_rollout_q_estimation', (FAKE, FAKE, I(64), I(1), SEL2, I(2), FAKE, FAKE, NULL, U64(1), U64(0), FAKE, ws, nb, NULL)),
    ]
    for name, args in calls:
        assert getattr(lib, name)(ctypes.byref(c), *args) == MPG_EINVAL, (name, triple)
        assert name.replace('mpg_', '') in lib.mpg_last_error().decode()


def test_the_matching_triple_passes_validation():
    """... and is refused only for its workspace: one byte short of the query, before anything is enqueued"""
    lib, c = L.lib(), _cfg()
    need = lib.mpg_rollout_q_target_workspace_bytes(ctypes.byref(c), I(64))
    rc = lib.mpg_rollout_q_target(ctypes.byref(c), FAKE, FAKE, I(64), I(25), FAKE, FAKE, NULL, U64(1), U64(0), FAKE, FAKE, SZ(need - 1), NULL)
    assert rc == -1001 and 'workspace too small' in lib.mpg_last_error().decode()


REAL_ENV = [
    ('mpg_env_reset_from_obs', lambda: (I(2), I(16), I(11), FAKE, FAKE, NULL)),
    ('mpg_env_reset', lambda: (I(2), I(16), I(11), FAKE, NULL, U64(1), U64(0), FAKE, NULL)),
    ('mpg_env_step', lambda: (I(2), I(16), I(11), FAKE, FAKE, FAKE, FAKE, FAKE, NULL, NULL)),
    ('mpg_env_step_store_reset', lambda: (I(2), I(16), I(11), FAKE, FAKE, I(64), I(0), FAKE, FAKE, FAKE, FAKE, FAKE, U64(1), U64(0), FAKE,
                                          NULL, NULL)),
]


@pytest.mark.parametrize('name,args', REAL_ENV, ids=[c[0] for c in REAL_ENV])
def test_real_env_entry_points_refuse_the_model_only_kind(name, args):
    lib = L.lib()
    assert getattr(lib, name)(*args()) == MPG_EINVAL
    msg = lib.mpg_last_error().decode()
    assert name in msg and 'MuJoCo' in msg and 'not provided' in msg, msg


def test_worker_step_refuses_the_model_only_kind():
    lib, c = L.lib(), _cfg()
    rc = lib.mpg_worker_step(ctypes.byref(c), FAKE, I(16), FAKE, FAKE, F(0.1), U64(1), U64(0), FAKE, I(64), I(0), FAKE, FAKE, FAKE, FAKE, FAKE,
                             U64(1), U64(0), NULL, NULL, I(0), NULL, NULL, NULL, NULL, NULL)
    assert rc == MPG_EINVAL and 'MuJoCo' in lib.mpg_last_error().decode()
