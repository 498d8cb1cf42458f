"""mpg_model_mpc_rollout, mpc.model_mpc_rollout, run_model_mpc(one_launch=True) and ModelEvaluator.gap_to_mpc_closed_loop on the GPU, on
both engines (tests/test_model_mpc_rollout.py says on the CPU why these input sets are worth running).

 1. The one launch against the chain it replaces, built here from M.model_mpc_solve, M.model_mpc_cost_grad at horizon 1 and M._shifted:
    every output and both carried buffers as 32-bit patterns.
 2. Nullable outputs, each on its own; sentinels round every output; cold, u_io untouched.
 3. Carry-over: 5 steps = 2 + 3; chunks of run_model_mpc(one_launch=True) under a small work cap.
 4. Row independence, also beside a NaN row.
 5. Invariants, bit for bit.
 6. The plant's step, teacher-forced, against the float64 oracle under tests/yardstick.check_values, and against ops.model_step.
 7. The Python layer.
Every figure is printed before it is asserted.  No test asserts a time.

Measured on an MI355X (both engines alike: the code has no matrix instruction): every bit comparison holds; the
plant's step, teacher-forced over 5 steps x 130 rows, relative L2 against the float64 oracle, next row / reward (float32 oracle):
    PathTracking 2.8e-8 (2.7e-8) / 6.2e-8 (7.2e-8), K = 3 2.6e-8 (2.6e-8) / 5.5e-8 (7.3e-8), pendulum 3.7e-8 (3.4e-8) / 6.9e-8 (6.9e-8),
    double pendulum 7.3e-8 (8.2e-8) / 1.4e-7 (1.3e-7); the launch's step against mpg_model_step at most 3.6e-8 / 1.2e-7
    a wave's rows at tol = 1e-3 leave the first solve after 10 .. 138 (PathTracking) and 5 .. 200 (pendulum) accepted iterations
    run_model_mpc, one launch against the loop over 3 steps: rew_traj within 7.3e-8 on PathTracking and the pendulum; on the double
    pendulum 1.2e-6 cold and 4.5e-5 warm, last_obs 4.5e-4 and 2.5e-2 (rounding through 20-iteration solves on a falling pendulum)"""
import ctypes
import math

import numpy as np
import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import mpc as M
from mpg_amd import ops
from tests import model_mpc_rollout_oracle as RO
from tests import model_rollout_oracle as R
from tests import yardstick as Y
from tests.test_model_mpc import MODEL_IDS, MODELS, wrap_to
from tests.test_model_mpc_rollout import ITERS, plant_noise, start_rows
from tests.test_model_mpc_rollout import start_point as start_pool
from tests.test_model_rollout_gpu import device_cfg
from tests.test_sac_gpu import engine  # noqa: F401  (the fixture: both builds of the library)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAME = 'mpg_model_mpc_rollout'
KEYS = ('obs_traj', 'plan_traj', 'rew_traj', 'cost_traj', 'pgnorm_traj', 'info_traj', 'last_obs', 'u_next')
ALL = range(len(MODELS))


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def cfg_of(mi):
    return device_cfg(*MODELS[mi])


def rows_of(mi, n):
    return dev(start_rows(mi)[:n])


def start_point(mi, n, h, kind):
    """the leading n rows of tests/test_model_mpc_rollout.start_point's pool: 'zeros', 'outside' (a fifth of the entries outside the
    box) or 'throttle'"""
    return dev(start_pool(mi, h, kind)[:n])


def noise(mi, steps, n, kind):
    if kind is None:
        return None
    if kind == 'zeros':
        return torch.zeros(steps, n, device=DEV)
    return dev(plant_noise(mi, steps)[:, :n])


def chain(cfg, obs, u0, steps, iters, tol, warm, eps):
    """the chain include/mpg_hip.h writes out for mpg_model_mpc_rollout, a launch per operation"""
    rec = {k: [] for k in KEYS[:6]}
    u_io = u0
    for t in range(steps):
        plan, cost, pg, info = M.model_mpc_solve(cfg, obs, u_io, iters, tol)
        if warm:
            u_io = M._shifted(plan)
        _, _, step_rec, rew = M.model_mpc_cost_grad(cfg, obs, plan[:, 0:1, :].contiguous(), None if eps is None else eps[t:t + 1],
                                                    want_grad=False, want_traj=True)
        for k, v in zip(KEYS[:6], (obs, plan, rew[:, 0], cost, pg, info)):
            rec[k].append(v)
        obs = step_rec[:, 1].contiguous()
    out = {k: torch.stack(v) for k, v in rec.items()}
    out.update(last_obs=obs, u_next=u_io.contiguous())
    return out


def launch(cfg, obs, u0, steps, iters=ITERS, tol=0., warm=False, eps=None):
    return dict(zip(KEYS, M.model_mpc_rollout(cfg, obs, u0, steps, iters, tol, warm, eps)))


def assert_same(a, b, what=''):
    for k in KEYS:
        assert same_bits(a[k], b[k]), (what, k)


# ---- 1: bit-identity to the chain ---------------------------------------------------------------------------------------------------
# (steps, horizon, warm, start point, tol, eps)
COMBOS = [(1, 1, True, 'zeros', 0., None), (2, 2, False, 'outside', 1e-3, 'zeros'), (5, 25, True, 'outside', 1e-3, 'drawn'),
          (5, 25, False, 'zeros', 0., 'drawn'), (2, 25, True, 'zeros', 0., None), (5, 2, False, 'outside', 0., 'drawn')]


def _against_the_chain(engine, mi, n, steps, h, warm, start, tol, eps_kind, iters=ITERS):
    cfg, obs = cfg_of(mi), rows_of(mi, n)
    u0, eps = start_point(mi, n, h, start), noise(mi, steps, n, eps_kind)
    keep = (obs.clone(), u0.clone())
    got = launch(cfg, obs, u0, steps, iters, tol, warm, eps)
    want = chain(cfg, obs, u0, steps, iters, tol, warm, eps)
    info = got['info_traj']
    print('   %s (%s) n %d steps %d horizon %d %s %s tol %g eps %s: info min %d max %d, rows of wave 0 that stopped early %d'
          % (MODEL_IDS[mi], engine, n, steps, h, 'warm' if warm else 'cold', start, tol, eps_kind, int(info.min()), int(info.max()),
             int((info[0, :64].abs() < iters).sum())))
    assert_same(got, want)
    assert same_bits(obs, keep[0]) and same_bits(u0, keep[1])        # nothing handed in is written
    assert same_bits(got['obs_traj'][0], obs)
    if not warm:
        assert same_bits(got['u_next'], u0)
    return got


@pytest.mark.parametrize('combo', range(len(COMBOS)), ids=['s%d-h%d-%s-%s-tol%g-eps_%s' % (s, h, 'warm' if w else 'cold', st, tol, e)
                                                            for s, h, w, st, tol, e in COMBOS])
@pytest.mark.parametrize('n', (1, 63, 65, 130))
@pytest.mark.parametrize('mi', ALL, ids=MODEL_IDS)
def test_one_launch_is_the_chain_bit_for_bit(engine, mi, n, combo):
    _against_the_chain(engine, mi, n, *COMBOS[combo])


@pytest.mark.parametrize('mi', ALL, ids=MODEL_IDS)
def test_horizon_31_and_no_iterations(engine, mi):
    """horizon 31: PathTracking's 102 272 bytes of LDS are asked for by name; iters 0: every plan is its clamped start"""
    _against_the_chain(engine, mi, 65, 2, 31, True, 'outside', 1e-3, 'drawn')
    got = _against_the_chain(engine, mi, 65, 2, 2, True, 'outside', 0., 'drawn', iters=0)
    u0 = start_point(mi, 65, 2, 'outside')
    assert same_bits(got['plan_traj'][0], u0.clamp(-1, 1)) and (got['info_traj'] == 0).all()
    assert same_bits(got['plan_traj'][1], M._shifted(u0.clamp(-1, 1)))
    # the 'throttle' start point: on PathTracking the plant is driven into both bounds of the v_x clamp, and the clamp is exact
    got = _against_the_chain(engine, mi, 65, 5, 2, True, 'throttle', 0., 'drawn', iters=0)
    if MODELS[mi][0] == R.PT:
        vx = torch.cat([got['obs_traj'][1:, :, 0], got['last_obs'][None, :, 0]])
        print('   %s (%s): (step, row) pairs at the upper bound %d, at the lower %d' % (MODEL_IDS[mi], engine, int((vx == 15.).sum()), int((vx == -19.).sum())))
        assert (vx == 15.).any() and (vx == -19.).any() and float(vx.max()) <= 15. and float(vx.min()) >= -19.


@pytest.mark.parametrize('mi', ALL, ids=MODEL_IDS)
def test_eps_zeros_is_eps_null_and_a_tolerance_splits_a_wave(engine, mi):
    cfg, obs, u0 = cfg_of(mi), rows_of(mi, 130), start_point(mi, 130, 25, 'zeros')
    a = launch(cfg, obs, u0, 3, 200 if MODELS[mi][0] != R.DPEND else ITERS, 1e-3, True, None)
    b = launch(cfg, obs, u0, 3, 200 if MODELS[mi][0] != R.DPEND else ITERS, 1e-3, True, noise(mi, 3, 130, 'zeros'))
    assert_same(a, b)
    info = a['info_traj'][:, :64].abs()
    print('   %s (%s): accepted iterations of wave 0, per step min %s max %s' % (MODEL_IDS[mi], engine, info.amin(1).tolist(), info.amax(1).tolist()))
    if MODELS[mi][0] != R.DPEND:         # rows of one wave leave the solve at different iterations
        assert (info.amin(1) < info.amax(1)).any()
    if MODELS[mi][0] != R.DPEND:         # a model with noise: a drawn eps changes the plant, and with it everything behind the first step
        c = launch(cfg, obs, u0, 3, ITERS, 0., True, noise(mi, 3, 130, 'drawn'))
        d = launch(cfg, obs, u0, 3, ITERS, 0., True, None)
        assert same_bits(c['plan_traj'][0], d['plan_traj'][0]) and not same_bits(c['obs_traj'][1], d['obs_traj'][1])


# ---- 2: nullable outputs, sentinels -------------------------------------------------------------------------------------------------
def _raw(cfg, n, steps, h, iters, tol, warm, obs, u0, eps, skip=()):
    """the entry point itself on exactly sized outputs between sentinels in one allocation; `skip`: the nullable outputs left out"""
    od, ad, S = cfg.obs_dim, cfg.act_dim, -7.
    sizes = dict(obs_io=n * od, u_io=n * h * ad, obs_traj=steps * n * od, plan_traj=steps * n * h * ad, rew_traj=steps * n, cost_traj=steps * n,
                 pgnorm_traj=steps * n, info_traj=steps * n)
    slab = torch.full((sum(sizes.values()) + 64 * (len(sizes) + 1),), S, device=DEV)
    inside = torch.zeros_like(slab, dtype=torch.bool)
    view, o = {}, 64
    for k, sz in sizes.items():
        view[k] = slab[o:o + sz]
        inside[o:o + sz] = True
        o += sz + 64
    view['obs_io'].copy_(obs.flatten())
    view['u_io'].copy_(u0.flatten())
    p = {k: (L.ptr(None) if k in skip else L.ptr(v)) for k, v in view.items()}
    L.call(NAME, ctypes.byref(cfg), L.c_int(n), L.c_int(steps), L.c_int(h), L.c_int(iters), L.c_float(tol), L.c_int(int(warm)), p['obs_io'],
           p['u_io'], L.ptr(eps), p['obs_traj'], p['plan_traj'], p['rew_traj'], p['cost_traj'], p['pgnorm_traj'], p['info_traj'], L.stream())
    assert (slab[~inside] == S).all()
    for k in skip:
        assert (view[k] == S).all(), k
    out = dict(obs_traj=view['obs_traj'].view(steps, n, od), plan_traj=view['plan_traj'].view(steps, n, h, ad), last_obs=view['obs_io'].view(n, od),
               u_next=view['u_io'].view(n, h, ad))
    for k in ('rew_traj', 'cost_traj', 'pgnorm_traj'):
        out[k] = view[k].view(steps, n)
    out['info_traj'] = view['info_traj'].view(steps, n).view(torch.int32)
    return out


@pytest.mark.parametrize('warm', [False, True], ids=['cold', 'warm'])
@pytest.mark.parametrize('mi', ALL, ids=MODEL_IDS)
def test_nullable_outputs_and_sentinels(engine, mi, warm):
    n, steps, h = 65, 2, 25
    cfg, obs, u0, eps = cfg_of(mi), rows_of(mi, n), start_point(mi, n, h, 'outside'), noise(mi, steps, n, 'drawn')
    full = launch(cfg, obs, u0, steps, ITERS, 1e-3, warm, eps)
    got = _raw(cfg, n, steps, h, ITERS, 1e-3, warm, obs, u0, eps)
    assert_same(got, full, 'all outputs')
    if not warm:
        assert same_bits(got['u_next'], u0)                          # cold: u_io is only read
    nullable = ('cost_traj', 'pgnorm_traj', 'info_traj')
    for skip in [(k,) for k in nullable] + [nullable]:
        part = _raw(cfg, n, steps, h, ITERS, 1e-3, warm, obs, u0, eps, skip)
        for k in KEYS:
            if k not in skip:
                assert same_bits(part[k], full[k]), (skip, k)


# ---- 3: carry-over ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('warm', [False, True], ids=['cold', 'warm'])
@pytest.mark.parametrize('mi', ALL, ids=MODEL_IDS)
def test_five_steps_are_two_and_three(engine, mi, warm):
    n, h = 65, 25
    cfg, obs, u0, eps = cfg_of(mi), rows_of(mi, n), start_point(mi, n, h, 'outside'), noise(mi, 5, n, 'drawn')
    whole = launch(cfg, obs, u0, 5, ITERS, 1e-3, warm, eps)
    a = launch(cfg, obs, u0, 2, ITERS, 1e-3, warm, eps[:2])
    b = launch(cfg, a['last_obs'], a['u_next'], 3, ITERS, 1e-3, warm, eps[2:])
    for k in KEYS[:6]:
        assert same_bits(torch.cat([a[k], b[k]]), whole[k]), k
    assert same_bits(b['last_obs'], whole['last_obs']) and same_bits(b['u_next'], whole['u_next'])


@pytest.mark.parametrize('warm', [False, True], ids=['cold', 'warm'])
@pytest.mark.parametrize('mi', ALL, ids=MODEL_IDS)
def test_chunks_of_run_model_mpc_equal_the_unchunked_record(engine, mi, warm):
    n, h, steps = 65, 5, 5
    cfg, obs, eps = cfg_of(mi), rows_of(mi, n), noise(mi, steps, n, 'drawn')
    whole = M.run_model_mpc(cfg, obs, steps, h, ITERS, 1e-3, warm, one_launch=True, eps=eps)
    assert M.model_rollout_chunk(steps, ITERS, M.MODEL_MAX_ROLLOUT_WORK[int(cfg.env_kind)]) == steps
    for cap in (ITERS, 2 * ITERS, 3 * ITERS):                       # chunks of 1, 2 and 3 steps
        part = M._run_model_mpc_one_launch(cfg, obs, steps, h, ITERS, 1e-3, warm, eps, work_cap=cap)
        assert sorted(part) == sorted(whole)
        for k in whole:
            assert same_bits(part[k], whole[k]), (cap, k)


# ---- 4: row independence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mi', ALL, ids=MODEL_IDS)
def test_a_row_does_not_depend_on_its_neighbours(engine, mi):
    n, h, steps = 130, 25, 3
    cfg, obs, u0, eps = cfg_of(mi), rows_of(mi, n), start_point(mi, n, h, 'outside'), noise(mi, steps, n, 'drawn')
    whole = launch(cfg, obs, u0, steps, ITERS, 1e-3, True, eps)

    def rows(rec, sel):
        return {k: (v[sel] if k in ('last_obs', 'u_next') else v[:, sel]) for k, v in rec.items()}

    for i in (0, 63, 64, 129):
        alone = launch(cfg, obs[i:i + 1].contiguous(), u0[i:i + 1].contiguous(), steps, ITERS, 1e-3, True, eps[:, i:i + 1].contiguous())
        assert_same(rows(whole, slice(i, i + 1)), alone, i)
    # one NaN row: info -1 at every step, its clamped start kept; the other rows keep their bits (cold, so that the start is the same)
    cold = launch(cfg, obs, u0, steps, ITERS, 1e-3, False, eps)
    bad = obs.clone()
    bad[70, 1] = float('nan')
    got = launch(cfg, bad, u0, steps, ITERS, 1e-3, False, eps)
    print('   %s (%s): the NaN row\'s info %s' % (MODEL_IDS[mi], engine, got['info_traj'][:, 70].tolist()))
    assert (got['info_traj'][:, 70] == -1).all()
    for t in range(steps):
        assert same_bits(got['plan_traj'][t, 70], u0[70].clamp(-1, 1))
    keep = [i for i in range(n) if i != 70]
    assert_same(rows(got, keep), rows(cold, keep))


# ---- 5: invariants ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('warm', [False, True], ids=['cold', 'warm'])
@pytest.mark.parametrize('mi', ALL, ids=MODEL_IDS)
def test_invariants(engine, mi, warm):
    n, h, steps = 130, 25, 3
    cfg, obs, u0, eps = cfg_of(mi), rows_of(mi, n), start_point(mi, n, h, 'outside'), noise(mi, steps, n, 'drawn')
    got = launch(cfg, obs, u0, steps, ITERS, 0., warm, eps)
    od, ad = cfg.obs_dim, cfg.act_dim
    at = M.model_mpc_cost_grad(cfg, got['obs_traj'].reshape(steps * n, od), got['plan_traj'].reshape(steps * n, h, ad), want_grad=False)[0]
    assert same_bits(at.reshape(steps, n), got['cost_traj'])
    starts = [u0.clamp(-1, 1)] + [(M._shifted(got['plan_traj'][t]) if warm else u0.clamp(-1, 1)) for t in range(steps - 1)]
    f0 = M.model_mpc_cost_grad(cfg, got['obs_traj'].reshape(steps * n, od), torch.stack(starts).reshape(steps * n, h, ad), want_grad=False)[0]
    print('   %s (%s, %s): cost_traj - cost(clamped start) max %.3g' % (MODEL_IDS[mi], engine, 'warm' if warm else 'cold',
                                                                        float((got['cost_traj'].flatten() - f0).max())))
    assert (got['cost_traj'].flatten() <= f0).all()
    assert float(got['plan_traj'].abs().max()) <= 1.
    for _ in range(20):
        assert_same(launch(cfg, obs, u0, steps, ITERS, 0., warm, eps), got)


# ---- 6: the plant's step, teacher-forced --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mi', ALL, ids=MODEL_IDS)
def test_plant_step_against_the_float64_oracle_and_model_step(engine, mi):
    env_id, K = MODELS[mi]
    ocfg = R.ocfg_of(env_id, K)
    n, h, steps = 130, 25, 5
    cfg, obs, u0, eps = cfg_of(mi), rows_of(mi, n), start_point(mi, n, h, 'zeros'), noise(mi, steps, n, 'drawn')
    got = launch(cfg, obs, u0, steps, ITERS, 0., True, eps)
    o = got['obs_traj'].reshape(steps * n, -1)
    a = got['plan_traj'][:, :, 0, :].reshape(steps * n, -1).contiguous()
    e = eps.reshape(steps * n)
    nxt = torch.cat([got['obs_traj'][1:], got['last_obs'][None]]).reshape(steps * n, -1).cpu().numpy()
    rew = got['rew_traj'].reshape(steps * n).cpu().numpy()
    o_np, a_np, e_np = o.cpu().numpy(), a.cpu().numpy(), e.cpu().numpy()
    n64, r64 = RO.plant_step(ocfg, o_np, a_np, e_np, torch.float64)
    n32, r32 = RO.plant_step(ocfg, o_np, a_np, e_np, torch.float32)
    ms_n, ms_r = (x.cpu().numpy() for x in ops.model_step(cfg, o, a, e))

    def angle(x):        # PathTracking's wrapped heading error is compared modulo 2 pi
        x = x.astype(np.float64).copy()
        if env_id == R.PT:
            x[:, 4] = wrap_to(x[:, 4], n64[:, 4])
        return x

    for tag, on, r in (('the launch', nxt, rew), ('mpg_model_step', ms_n, ms_r)):
        print('   %s (%s) %s: next row vs float64 %.2e (float32 oracle %.2e) vs float32 oracle %.2e; reward %.2e (%.2e) %.2e'
              % (MODEL_IDS[mi], engine, tag, Y.rel_l2(angle(on), n64), Y.rel_l2(angle(n32), n64), Y.rel_l2(angle(on), angle(n32)),
                 Y.rel_l2(r, r64), Y.rel_l2(r32, r64), Y.rel_l2(r, r32)))
    print('   %s: the launch\'s step vs mpg_model_step: next row %.2e reward %.2e' % (MODEL_IDS[mi], Y.rel_l2(angle(nxt), angle(ms_n)), Y.rel_l2(rew, ms_r)))
    for tag, on, r in (('the launch', nxt, rew), ('mpg_model_step', ms_n, ms_r)):
        Y.check_values(angle(on), angle(n32), n64, tag + ' next row')
        Y.check_values(r, r32, r64, tag + ' reward')
    # the two forms of the step agree to rounding: each is within the rule of the float64 oracle, and of the other at its 1e-4 bar
    assert Y.rel_l2(angle(nxt), angle(ms_n)) <= 1e-4 and Y.rel_l2(rew, ms_r) <= 1e-4
    # the row format: from the second row on what the step writes
    rest = torch.cat([got['obs_traj'][1:], got['last_obs'][None]])
    if env_id == R.PT and K:
        assert (rest[:, :, 6:] == rest[:, :, 3:4]).all()
    if env_id == R.DPEND:
        assert (rest[:, :, 8:] == 0).all() and (obs[:, 8:] != 0).any()


# ---- 7: the Python layer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('warm', [False, True], ids=['cold', 'warm'])
@pytest.mark.parametrize('mi', ALL, ids=MODEL_IDS)
def test_run_model_mpc_one_launch_has_the_loops_record_and_its_first_step(engine, mi, warm):
    n, h, steps = 5, 5, 3
    cfg, obs, eps = cfg_of(mi), rows_of(mi, 16)[11:16].contiguous(), noise(mi, steps, n, 'drawn')
    loop = M.run_model_mpc(cfg, obs, steps, h, ITERS, 1e-3, warm, eps=eps)
    one = M.run_model_mpc(cfg, obs, steps, h, ITERS, 1e-3, warm, one_launch=True, eps=eps)
    assert sorted(one) == sorted(loop)
    for k in loop:
        assert one[k].shape == loop[k].shape and one[k].dtype == loop[k].dtype, k
    for k in ('obs_traj', 'act_traj', 'cost', 'pgnorm', 'info'):
        assert same_bits(one[k][0], loop[k][0]), k
    print('   %s (%s): one launch vs the loop, rew_traj %.2e last_obs %.2e' % (MODEL_IDS[mi], engine, Y.rel_l2(one['rew_traj'].cpu(), loop['rew_traj'].cpu()),
                                                                               Y.rel_l2(one['last_obs'].cpu(), loop['last_obs'].cpu())))
    # the loop form with eps None is the loop as it was: tests/test_model_mpc_gpu.py holds it to the chain with ops.model_step


def test_refusals_reach_the_wrappers_callers_as_mpg_error(engine):
    cfg, obs = cfg_of(3), rows_of(3, 5)
    z = torch.zeros(5, 10, 1, device=DEV)
    with pytest.raises(L.MpgError, match=NAME + ': steps >= 1'):
        M.model_mpc_rollout(cfg, obs, z, 0)
    with pytest.raises(L.MpgError, match=NAME + ': steps \\* iters = 600'):
        M.model_mpc_rollout(cfg, obs, z, 3)
    with pytest.raises(L.MpgError, match=NAME + ': tol negative or NaN'):
        M.model_mpc_rollout(cfg, obs, z, 3, iters=10, tol=-1.)
    with pytest.raises(L.MpgError, match=NAME + ': horizon <= 31'):
        M.model_mpc_rollout(cfg, obs, torch.zeros(5, 32, 1, device=DEV), 3, iters=10)
    with pytest.raises(L.MpgError, match=NAME + ': iters <= 400 for env kind 2'):
        M.run_model_mpc(cfg, obs, 3, 10, iters=401, one_launch=True)
    # iters at the kind's cap: chunks of one step
    assert M.model_rollout_chunk(3, 400, M.MODEL_MAX_ROLLOUT_WORK[2]) == 1


@pytest.mark.parametrize('env_id', [R.PT, R.PD, R.DPEND], ids=['pt', 'pendulum', 'double-pendulum'])
def test_gap_to_mpc_closed_loop(engine, env_id):
    from tests.test_model_rollout_gpu import model_evaluator
    mi = [m[0] for m in MODELS].index(env_id)
    ev = model_evaluator('MPG-v2' if env_id == R.PT else 'NADP', env_id, num_eval_agent=16)
    obs0 = rows_of(mi, 32)[16:32].contiguous()
    steps, h = 4, 10
    eps = noise(mi, steps, 16, 'drawn')
    gap = ev.gap_to_mpc_closed_loop(obs0, steps=steps, horizon=h, iters=ITERS, eps=eps)
    print('   %s (%s): policy return %s' % (env_id, engine, gap['policy_return'].numpy()))
    print('   %s: MPC return %s; mean gap %.6g; mean iterations %.2f; failed share %.3f'
          % (env_id, gap['mpc_return'].numpy(), gap['mean_gap'], gap['mean_iters'], gap['failed_share']))
    for k in ('policy_return', 'mpc_return', 'gap'):
        assert gap[k].shape == (16,) and gap[k].dtype == torch.float64 and torch.isfinite(gap[k]).all() and not gap[k].is_cuda
        assert math.isclose(gap['mean_' + k], float(gap[k].mean()))
    assert 0. <= gap['mean_iters'] <= ITERS and 0. <= gap['failed_share'] <= 1.
    pw = ev.policy_with_value
    want = ops.model_rollout(pw.cfg, pw.net('policy'), obs0, steps, eps)[2]
    assert torch.equal(gap['policy_return'], want.double().sum(0).cpu())
    rec = M.run_model_mpc(pw.cfg, obs0, steps, h, ITERS, 1e-3, True, one_launch=True, eps=eps)
    assert torch.equal(gap['mpc_return'], rec['rew_traj'].double().sum(0).cpu())
    assert gap['mpc_record']['obs_traj'].shape == (steps, 16, pw.cfg.obs_dim)
    # the solver's invariant through the closed loop's first step: from the policy's own clamped actions, MPC's one-step reward plus
    # the rest of its plan's cost is not above the policy's horizon cost (noise at the means on both sides)
    u_pi = ops.model_rollout(pw.cfg, pw.net('policy'), obs0, h)[1].permute(1, 0, 2).clamp(-1, 1).contiguous()
    policy_cost = M.model_mpc_cost_grad(pw.cfg, obs0, u_pi, want_grad=False)[0].double()
    out = launch(pw.cfg, obs0, u_pi, 1, ITERS, 0., False, None)
    rest = M.model_mpc_cost_grad(pw.cfg, out['last_obs'], out['plan_traj'][0][:, 1:].contiguous(), want_grad=False)[0].double()
    mpc_side = -out['rew_traj'][0].double() + rest
    print('   %s: policy horizon cost %s' % (env_id, policy_cost.cpu().numpy()))
    print('   %s: MPC one-step reward plus the rest of its plan %s (cost_traj %s)' % (env_id, mpc_side.cpu().numpy(), out['cost_traj'][0].cpu().numpy()))
    assert (out['cost_traj'][0].double() <= policy_cost).all()
    assert (mpc_side <= policy_cost).all()
