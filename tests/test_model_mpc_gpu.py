"""mpg_model_mpc_cost_grad, mpg_model_mpc_solve, ModelMPC, run_model_mpc and ModelEvaluator.gap_to_mpc on the GPU, on both engines
(tests/model_mpc_oracle.py restates them; tests/test_model_mpc.py builds the input sets and says on the CPU why they are worth running).

 1. Cost, gradient, obs_traj and rew_traj against the float64 oracle under tests/yardstick.check_values (4 x the float32 oracle's error
    + 1e-6, and 1e-4 from the float32 oracle): PathTracking K = 0 and K = 3, pendulum, double pendulum x rows (1, 63, 64, 65, 130) x
    horizons (1, 2, 25, 31); eps NULL, and given once per model.  The observation record as one array, PathTracking's wrapped angle
    modulo 2 pi, and every column of it at the rule's 1e-4 bar.
 2. The anchor to shipped code: with u = the act_traj of mpg_model_rollout (same obs0, eps, steps = horizon) the cost is - sum rew_traj
    and obs_traj is the rollout's, at rtol 5e-5, atol 1e-6 (the anchor bar of tests/test_model_rollout_gpu.py).
 3. Bit-level invariants, compared as 32-bit patterns.
 4. The solver against the fixture's kept rows, 200 iterations from zeros: the float64 oracle cost at the device's point minus `best` is at
    most 4 x the float32 emulation's gap (clamped at 0) + 1e-5 max(best, 1) - tests/test_mpc_gpu.py's rule.
 5. The Python layer: ModelMPC's one-row forms, run_model_mpc against the chain it wraps, gap_to_mpc.
Every figure is printed before it is asserted.

Measured on an MI355X (both engines alike: the code has no matrix instruction), worst relative L2 against the
float64 oracle over all rows x horizons, cost / gradient / obs_traj / rew_traj:
    PathTracking 4.6e-7 / 5.7e-7 / 1.5e-7 / 5.3e-7, K = 3 2.8e-7 / 1.6e-6 / 1.2e-7 / 3.3e-7, pendulum 3.7e-7 / 8.4e-7 / 5.4e-7 / 4.7e-7,
    double pendulum 8.6e-7 / 5.3e-6 / 2.0e-6 / 1.6e-6
    anchor: cost vs - sum rew_traj at most 3.2e-7 relative (bar 5e-5), obs_traj at most 0.51 of 1e-6 + 5e-5 |x|
    solver: float64 cost at the device's point minus the optimum at most 8.5e-8 (PathTracking, emulation 1.7e-7), 1.7e-13 (pendulum,
    1.5e-11), 6.1e-5 (double pendulum at horizon 10, emulation 5.1e-5)"""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import mpc as M
from mpg_amd import ops
from tests import model_mpc_oracle as MO
from tests import model_rollout_oracle as R
from tests import yardstick as Y
from tests.golden_inputs import mlp_weights_flat
from tests.test_model_mpc import EPS_SETS, FIXTURE_SETS, HORIZONS, MODEL_IDS, MODELS, ROWS, columns, input_set
from tests.test_model_rollout_gpu import device_cfg
from tests.test_sac_gpu import engine  # noqa: F401  (the fixture: both builds of the library)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'model_mpc_ref.npz')


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def cfg_of(mi):
    return device_cfg(*MODELS[mi])


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


# ---- 1: cost, gradient and records against the float64 oracle ---------------------------------------------------------------------
def _against_the_oracle(engine, mi, rows, h, with_eps):
    env_id = MODELS[mi][0]
    _, obs0, u, eps, r64, r32 = input_set(mi, h, with_eps)
    e = None if eps is None else dev(eps[:, :rows])
    cost, grad, obs_traj, rew_traj = M.model_mpc_cost_grad(cfg_of(mi), dev(obs0[:rows]), dev(u[:rows]), e, want_grad=True, want_traj=True)
    got = dict(cost=cost.cpu().numpy(), grad=grad.cpu().numpy(), rew=rew_traj.cpu().numpy())
    obs = obs_traj.cpu().numpy()
    assert obs.shape == (rows, h + 1, obs0.shape[1]) and got['grad'].shape == u[:rows].shape and got['rew'].shape == (rows, h)
    for name in ('cost', 'grad', 'rew'):
        a, b32, b64 = got[name], r32[name][:rows], r64[name][:rows]
        print('   %s %s rows %d horizon %d %s: vs float64 %.2e (float32 oracle %.2e)  vs float32 oracle %.2e'
              % (MODEL_IDS[mi], engine, rows, h, name, Y.rel_l2(a, b64), Y.rel_l2(b32, b64), Y.rel_l2(a, b32)))
    # the observation record: as ONE array under the rule (PathTracking's wrapped angle modulo 2 pi), and column by column against the
    # rule's 1e-4 bar, so that the wide columns (x up to 600 m) do not carry the narrow ones
    ref64 = r64['obs'][:rows]
    mine, theirs = (np.stack([col for _, col in columns(env_id, a, ref64)], 2) for a in (obs, r32['obs'][:rows]))
    per_column = [Y.rel_l2(mine[:, :, c], ref64[:, :, c]) for c in range(ref64.shape[2]) if np.linalg.norm(ref64[:, :, c]) > 0]
    print('   %s rows %d horizon %d obs_traj: vs float64 %.2e (float32 oracle %.2e)  vs float32 oracle %.2e; worst column vs float64 %.2e'
          % (MODEL_IDS[mi], rows, h, Y.rel_l2(mine, ref64), Y.rel_l2(theirs, ref64), Y.rel_l2(mine, theirs), max(per_column)))
    for name in ('cost', 'grad', 'rew'):
        Y.check_values(got[name], r32[name][:rows], r64[name][:rows], name)
    Y.check_values(mine, theirs, ref64, 'obs_traj')
    assert max(per_column) <= 1e-4, per_column
    # row 0 is the start row as given; the rest is in mpg_model_step's row format
    assert np.array_equal(obs[:, 0].view(np.int32), obs0[:rows].view(np.int32))
    if env_id == R.PT:
        assert (obs[:, 1:, 6:] == obs[:, 1:, 3:4]).all() and np.abs(obs[:, 1:, 4]).max() <= np.float32(np.pi)
        for bound in (1., 35.):         # the clamp is exact
            on = ref64[:, 1:, 0] == bound - 20.
            assert (obs[:, 1:, 0][on] == np.float32(bound - 20.)).all()
    if env_id == R.DPEND:
        assert (obs[:, 1:, 8:] == 0).all() and (obs0[:rows, 8:] != 0).any()


@pytest.mark.parametrize('h', HORIZONS)
@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('mi', range(len(MODELS)), ids=MODEL_IDS)
def test_cost_gradient_and_records_against_the_float64_oracle(engine, mi, rows, h):
    _against_the_oracle(engine, mi, rows, h, False)


@pytest.mark.parametrize('mi,h', EPS_SETS, ids=MODEL_IDS)
def test_with_model_noise_against_the_float64_oracle(engine, mi, h):
    _against_the_oracle(engine, mi, 65, h, True)
    # eps = NULL is eps = zeros
    _, obs0, u, _, _, _ = input_set(mi, h, True)
    a = M.model_mpc_cost_grad(cfg_of(mi), dev(obs0), dev(u), None, want_traj=True)
    b = M.model_mpc_cost_grad(cfg_of(mi), dev(obs0), dev(u), torch.zeros(h, obs0.shape[0], device=DEV), want_traj=True)
    assert all(same_bits(x, y) for x, y in zip(a, b))


# ---- 2: the anchor to mpg_model_rollout ---------------------------------------------------------------------------------------------
def anchor_cfg(mi):
    """a policy whose actions are in the tanh range: PathTracking's tanh output, the double pendulum's tanh(mean) * 1, and on the pendulum
    tanh(mean) * 1 in place of its default range of 3"""
    return ops.make_cfg(R.PD, action_range=1.0) if MODELS[mi][0] == R.PD else cfg_of(mi)


@pytest.mark.parametrize('mi', range(len(MODELS)), ids=MODEL_IDS)
def test_cost_and_record_of_a_policys_rollout(engine, mi):
    env_id, _ = MODELS[mi]
    h, rows = 10, 48
    _, obs0, _, eps, _, _ = input_set(mi, 25, True)
    cfg = anchor_cfg(mi)
    obs0, eps = dev(obs0[:rows]), dev(eps[:h, :rows])
    pol = dev(mlp_weights_flat(np.random.Generator(np.random.PCG64(77 + mi)), cfg.obs_dim, 2 * cfg.act_dim))
    obs_t, act_t, rew_t, last = ops.model_rollout(cfg, pol, obs0, h, eps)
    assert float(act_t.abs().max()) <= 1.
    cost, _, obs_traj, rew_traj = M.model_mpc_cost_grad(cfg, obs0, act_t.permute(1, 0, 2).contiguous(), eps, want_grad=False, want_traj=True)
    want = -rew_t.double().sum(0).cpu().numpy()
    print('   %s (%s): cost vs - sum rew_traj, worst relative difference %.2e' % (MODEL_IDS[mi], engine, np.abs(cost.cpu().numpy() / want - 1).max()))
    want_obs = torch.cat([obs_t, last[None]]).permute(1, 0, 2).cpu().numpy().astype(np.float64)
    got_obs = obs_traj.cpu().numpy().astype(np.float64)
    if env_id == R.PT:
        got_obs[:, :, 4] = got_obs[:, :, 4] - 2 * np.pi * np.round((got_obs[:, :, 4] - want_obs[:, :, 4]) / (2 * np.pi))
    print('   %s: obs_traj vs the rollout, worst |difference| / (1e-6 + 5e-5 |x|) %.3f'
          % (MODEL_IDS[mi], (np.abs(got_obs - want_obs) / (1e-6 + 5e-5 * np.abs(want_obs))).max()))
    np.testing.assert_allclose(cost.cpu().numpy(), want, rtol=5e-5, atol=1e-6)
    np.testing.assert_allclose(got_obs, want_obs, rtol=5e-5, atol=1e-6)
    np.testing.assert_allclose(rew_traj.cpu().numpy(), rew_t.t().cpu().numpy(), rtol=5e-5, atol=1e-6)


# ---- 3: bit-level invariants --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h', (1, 25, 31))
@pytest.mark.parametrize('mi', range(len(MODELS)), ids=MODEL_IDS)
def test_cost_is_the_same_bits_without_the_optional_outputs_and_between_two_launches(engine, mi, h):
    _, obs0, u, _, _, _ = input_set(mi, h)
    cfg, obs0, u = cfg_of(mi), dev(obs0), dev(u)
    full = M.model_mpc_cost_grad(cfg, obs0, u, want_grad=True, want_traj=True)
    again = M.model_mpc_cost_grad(cfg, obs0, u, want_grad=True, want_traj=True)
    for a, b in zip(full, again):
        assert same_bits(a, b)
    assert same_bits(M.model_mpc_cost_grad(cfg, obs0, u, want_grad=False, want_traj=False)[0], full[0])
    g_only = M.model_mpc_cost_grad(cfg, obs0, u, want_grad=True, want_traj=False)
    t_only = M.model_mpc_cost_grad(cfg, obs0, u, want_grad=False, want_traj=True)
    assert same_bits(g_only[0], full[0]) and same_bits(g_only[1], full[1]) and g_only[2] is None and g_only[3] is None
    assert same_bits(t_only[0], full[0]) and same_bits(t_only[2], full[2]) and same_bits(t_only[3], full[3]) and t_only[1] is None
    # each record alone
    cost = torch.empty(130, device=DEV)
    rew = torch.empty(130, h, device=DEV)
    L.call('mpg_model_mpc_cost_grad', ctypes.byref(cfg), L.c_int(130), L.c_int(h), L.ptr(obs0), L.ptr(u), L.ptr(None), L.ptr(cost), L.ptr(None),
           L.ptr(None), L.ptr(rew), L.stream())
    assert same_bits(cost, full[0]) and same_bits(rew, full[3])


@pytest.mark.parametrize('mi', range(len(MODELS)), ids=MODEL_IDS)
def test_nothing_is_written_behind_the_last_row_or_outside_the_outputs(engine, mi):
    """65 rows launch two workgroups, the second one's 63 idle lanes store nothing; every output is exactly sized and sits between
    sentinels in one allocation"""
    h = 25
    _, obs0, u, _, _, _ = input_set(mi, h)
    cfg = cfg_of(mi)
    od, ad, S = cfg.obs_dim, cfg.act_dim, -7.
    sizes = dict(cost=65, grad=65 * h * ad, obs=65 * (h + 1) * od, rew=65 * h)
    slab = torch.full((sum(sizes.values()) + 64 * (len(sizes) + 1),), S, device=DEV)
    view, o = {}, 64
    for k, n in sizes.items():
        view[k] = slab[o:o + n]
        o += n + 64
    L.call('mpg_model_mpc_cost_grad', ctypes.byref(cfg), L.c_int(65), L.c_int(h), L.ptr(dev(obs0[:65])), L.ptr(dev(u[:65])), L.ptr(None),
           L.ptr(view['cost']), L.ptr(view['grad']), L.ptr(view['obs']), L.ptr(view['rew']), L.stream())
    inside = torch.zeros_like(slab, dtype=torch.bool)
    o = 64
    for k, n in sizes.items():
        inside[o:o + n] = True
        o += n + 64
    assert (slab[~inside] == S).all()
    assert (view['cost'] != S).all() and (view['rew'] != S).all() and (view['obs'] != S).all()
    # the solver's outputs likewise, 65 rows in arrays of 128
    u_io = torch.full((128, h, ad), S, device=DEV)
    u_io[:65] = 0.
    cost, pg = torch.full((128,), S, device=DEV), torch.full((128,), S, device=DEV)
    info = torch.full((128,), -7, dtype=torch.int32, device=DEV)
    L.call('mpg_model_mpc_solve', ctypes.byref(cfg), L.c_int(65), L.c_int(h), L.c_int(20), L.c_float(0.), L.ptr(dev(obs0[:65])), L.ptr(None),
           L.ptr(u_io), L.ptr(cost), L.ptr(pg), L.ptr(info), L.stream())
    assert (u_io[65:] == S).all() and (cost[65:] == S).all() and (pg[65:] == S).all() and (info[65:] == -7).all()
    assert (info[:65] != -7).all() and (cost[:65] != S).all()


@pytest.mark.parametrize('mi', range(len(MODELS)), ids=MODEL_IDS)
def test_no_iterations_return_the_clamped_start_its_cost_and_the_norms_formula(engine, mi):
    h = 25
    _, obs0, _, _, _, _ = input_set(mi, h)
    cfg, obs0 = cfg_of(mi), dev(obs0[:16])
    draw = lambda: dev(np.random.default_rng(5).uniform(-2, 2, (16, h, cfg.act_dim)))
    start = draw()
    mpc = M.ModelMPC(cfg, obs0, h)
    u, cost, pg, info = mpc.solve(u_init=start, iters=0)
    assert same_bits(u, start.clamp(-1, 1)) and (info == 0).all()
    c, g = mpc.cost_and_gradient(u)
    assert same_bits(cost, c)
    assert same_bits(pg, ((u - g).clamp(-1, 1) - u).abs().flatten(1).amax(1))
    assert (start.abs() > 1).any() and same_bits(start, draw())          # the start is left alone


@pytest.mark.parametrize('mi', range(len(MODELS)), ids=MODEL_IDS)
def test_solve_invariants(engine, mi):
    """cost_out is cost_grad's at the returned u; rows solved alone equal the same rows solved together; a NaN row gives info -1 and
    leaves its neighbours alone; cost_out <= the cost of the clamped start from a random start in [-2, 2]"""
    env_id = MODELS[mi][0]
    h, iters = 25, 60
    _, obs0, _, _, _, _ = input_set(mi, h)
    cfg, obs0 = cfg_of(mi), dev(obs0)
    start = dev(np.random.default_rng(6 + mi).uniform(-2, 2, (130, h, cfg.act_dim)))
    whole = M.model_mpc_solve(cfg, obs0, start, iters=iters)
    u, cost, pg, info = whole
    assert float(u.abs().max()) <= 1.
    assert same_bits(cost, M.model_mpc_cost_grad(cfg, obs0, u, want_grad=False)[0])
    f0 = M.model_mpc_cost_grad(cfg, obs0, start.clamp(-1, 1), want_grad=False)[0]
    print('   %s (%s): info %s ... ; cost_out - cost(clamped start) max %.3g' % (MODEL_IDS[mi], engine, info[:12].tolist(), float((cost - f0).max())))
    assert (cost <= f0).all()
    assert (info != 0).any()
    for lo, hi in ((0, 64), (64, 130), (63, 65)):
        part = M.model_mpc_solve(cfg, obs0[lo:hi].contiguous(), start[lo:hi].contiguous(), iters=iters)
        for a, b in zip(whole, part):
            assert same_bits(a[lo:hi], b), (lo, hi)
    for a, b in zip(whole, M.model_mpc_solve(cfg, obs0, start, iters=iters)):
        assert same_bits(a, b)
    bad = obs0[:64].clone()
    bad[7, 1] = float('nan')
    bad[40, 0] = float('nan')
    z = torch.zeros(64, h, cfg.act_dim, device=DEV)
    clean, got = M.model_mpc_solve(cfg, obs0[:64].contiguous(), z, iters=iters), M.model_mpc_solve(cfg, bad, z, iters=iters)
    assert got[3][7] == -1 and got[3][40] == -1
    assert (got[0][[7, 40]] == 0).all()                                       # the last accepted point: the start
    keep = [i for i in range(64) if i not in (7, 40)]
    for a, b in zip(clean, got):
        assert same_bits(a[keep], b[keep])


# ---- 4: the solver against the fixture ---------------------------------------------------------------------------------------------
def fixture_cfg(env_id):
    return ops.make_cfg(env_id)


@pytest.mark.parametrize('tag,env_id,h', FIXTURE_SETS, ids=['%s-h%d' % (t, h) for t, _, h in FIXTURE_SETS])
def test_solver_against_the_float64_optimum_and_the_float32_emulation(engine, gold, tag, env_id, h):
    k = '%s_h%d' % (tag, h)
    ocfg, kept = R.ocfg_of(env_id), gold['kept_' + k]
    obs0, best, gap_emu = gold['obs0_' + k][kept], gold['best_' + k][kept], gold['spg32_gap_' + k][kept]
    mpc = M.ModelMPC(fixture_cfg(env_id), dev(obs0), h)
    u, cost, pg, info = mpc.solve(iters=200)
    assert (u.abs() <= 1).all()
    at_dev = MO.horizon_cost(ocfg, obs0, u.double().cpu()).numpy()
    gap_dev = at_dev - best
    print('   %s (%s): device gap %s' % (k, engine, gap_dev))
    print('   %s: float32 emulation gap %s; info %s' % (k, gap_emu, info.tolist()))
    assert (gap_dev <= 4 * np.maximum(gap_emu, 0.) + 1e-5 * np.maximum(best, 1.)).all()
    assert same_bits(cost, mpc.cost_function(u))
    for a, b in zip((u, cost, pg, info), mpc.solve(iters=200)):
        assert same_bits(a, b)


@pytest.mark.parametrize('tag,env_id,h', FIXTURE_SETS, ids=['%s-h%d' % (t, h) for t, _, h in FIXTURE_SETS])
def test_a_tolerance_stops_every_fixture_row_early(engine, gold, tag, env_id, h):
    k = '%s_h%d' % (tag, h)
    obs0 = gold['obs0_' + k][gold['kept_' + k]]
    u, cost, pg, info = M.ModelMPC(fixture_cfg(env_id), dev(obs0), h).solve(iters=200, tol=1e-3)
    print('   %s (%s): info %s pgnorm max %.3g' % (k, engine, info.tolist(), float(pg.max())))
    assert (pg <= 1e-3).all() and (info > 0).all() and (info < 200).all()


# ---- 5: the Python layer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mi', range(len(MODELS)), ids=MODEL_IDS)
def test_one_row_forms(engine, mi):
    _, obs0, _, _, _, _ = input_set(mi, 25)
    cfg, obs0 = cfg_of(mi), dev(obs0[16:24])
    ad = cfg.act_dim
    one = M.ModelMPC(cfg, obs0[3], 10)
    u, cost, pg, info = one.solve(iters=30)
    assert u.shape == (10, ad) and cost.dim() == 0 and info.dim() == 0
    f = one.cost_function(u.reshape(-1))
    assert isinstance(f, float) and np.float32(f) == cost.item()
    ub, cb, _, _ = M.ModelMPC(cfg, obs0, 10).solve(iters=30)
    assert same_bits(ub[3], u) and same_bits(cb[3], cost)
    c, g = one.cost_and_gradient(u)
    assert g.shape == u.shape and same_bits(c, cost)
    one.reset_init_obs(obs0[4])
    assert same_bits(one.solve(iters=30)[0], ub[4])


def test_model_mpc_by_env_id_and_refusals_as_mpg_error(engine):
    from tests.test_model_mpc_abi import CAPS
    _, obs0, _, _, _, _ = input_set(3, 25)
    obs0 = dev(obs0[:4])
    a = M.ModelMPC(R.DPEND, obs0, 5).solve(iters=10)
    b = M.model_mpc_solve(ops.make_cfg(R.DPEND), obs0, horizon=5, iters=10)
    assert all(same_bits(x, y) for x, y in zip(a, b))
    with pytest.raises(L.MpgError, match='mpg_model_mpc_solve: iters <= %d for env kind 2' % CAPS[2]):
        M.ModelMPC(R.DPEND, obs0, 5).solve(iters=CAPS[2] + 1)
    with pytest.raises(L.MpgError, match='mpg_model_mpc_solve: tol negative or NaN'):
        M.ModelMPC(R.DPEND, obs0, 5).solve(tol=-1.)
    with pytest.raises(L.MpgError, match='mpg_model_mpc_cost_grad: horizon <= 31'):
        M.ModelMPC(R.DPEND, obs0, 32).cost_function(torch.zeros(4, 32, 1, device=DEV))


@pytest.mark.parametrize('warm', [False, True], ids=['cold', 'warm'])
@pytest.mark.parametrize('mi', range(len(MODELS)), ids=MODEL_IDS)
def test_run_model_mpc_is_the_chain_of_solve_and_model_step(engine, mi, warm):
    _, obs0, _, _, _, _ = input_set(mi, 25)
    cfg, obs0 = cfg_of(mi), dev(obs0[16:18])
    rec = M.run_model_mpc(cfg, obs0, steps=3, horizon=5, iters=40, warm_start=warm)
    od, ad = cfg.obs_dim, cfg.act_dim
    assert {k: tuple(v.shape) for k, v in rec.items()} == dict(obs_traj=(3, 2, od), act_traj=(3, 2, ad), rew_traj=(3, 2), cost=(3, 2),
                                                               pgnorm=(3, 2), info=(3, 2), last_obs=(2, od))
    assert rec['info'].dtype == torch.int32
    obs, u_init = obs0, torch.zeros(2, 5, ad, device=DEV)
    for t in range(3):
        plan, cost, pg, info = M.model_mpc_solve(cfg, obs, u_init, iters=40)
        if warm:
            u_init = torch.cat([plan[:, 1:], plan[:, -1:]], 1)
        act = plan[:, 0, :].contiguous()
        nxt, rew = ops.model_step(cfg, obs, act)
        for k, v in (('obs_traj', obs), ('act_traj', act), ('rew_traj', rew), ('cost', cost), ('pgnorm', pg), ('info', info)):
            assert same_bits(rec[k][t], v), (k, t)
        obs = nxt
    assert same_bits(rec['last_obs'], obs)
    if MODELS[mi][0] != R.DPEND:         # mpg_eval_metrics reads the record as it stands
        per, mean = ops.eval_metrics(cfg.env_kind, rec['obs_traj'], rec['act_traj'], rec['rew_traj'])
        assert per.shape == (len(ops.EVAL_METRIC_KEYS[cfg.env_kind]), 2)
        assert torch.equal(per[0], rec['rew_traj'].double().sum(0))          # episode_return


@pytest.mark.parametrize('env_id', [R.PT, R.PD, R.DPEND], ids=['pt', 'pendulum', 'double-pendulum'])
def test_gap_to_mpc_on_a_fresh_policy(engine, env_id):
    from tests.test_model_rollout_gpu import model_evaluator
    mi = [m[0] for m in MODELS].index(env_id)
    ev = model_evaluator('MPG-v2' if env_id == R.PT else 'NADP', env_id, num_eval_agent=16)
    _, obs0, _, _, _, _ = input_set(mi, 25)
    obs0 = dev(obs0[16:32])
    gap = ev.gap_to_mpc(obs0, horizon=10, iters=100)
    print('   %s (%s): policy cost %s' % (env_id, engine, gap['policy_cost'].numpy()))
    print('   %s: MPC cost %s; mean gap %.6g' % (env_id, gap['mpc_cost'].numpy(), gap['mean_gap']))
    assert gap['policy_cost'].shape == gap['mpc_cost'].shape == gap['gap'].shape == (16,) and gap['policy_cost'].dtype == torch.float64
    assert (gap['mpc_cost'] <= gap['policy_cost']).all() and (gap['gap'] >= 0).all()
    pw = ev.policy_with_value
    act = ops.model_rollout(pw.cfg, pw.net('policy'), obs0, 10)[1]
    u_pi = act.permute(1, 0, 2).clamp(-1, 1).contiguous()
    assert same_bits(gap['policy_u'], u_pi) and gap['policy_u'].shape == (16, 10, pw.cfg.act_dim)
    want = M.model_mpc_cost_grad(pw.cfg, obs0, u_pi, want_grad=False)[0]
    assert torch.equal(gap['policy_cost'], want.double().cpu())
    assert same_bits(M.model_mpc_cost_grad(pw.cfg, obs0, gap['mpc_u'], want_grad=False)[0].double().cpu().float(), gap['mpc_cost'].float())
    assert math.isclose(gap['mean_gap'], float(gap['gap'].mean()))
    # horizon None: the stack's num_rollout_list_for_policy_update[-1]
    n = int(ev.args.num_rollout_list_for_policy_update[-1])
    assert ev.gap_to_mpc(obs0, iters=5)['policy_u'].shape[1] == n
