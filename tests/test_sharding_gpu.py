"""Data-parallel gradient scaling of every learner, in ONE process (no process group, no spawned rank).

Every gradient entry point takes inv_b_global = 1 / (rows x world size): a rank computes sum-reduced partials of its shard already
scaled by the global batch, the flat [gradients | statistics] buffer is all-reduced once and clipped afterwards, and get_stats()
divides the summed statistics by batch_size * world size (mpg_amd/learners.py).  Three parts:

 1. entry points - the float32 sum of the partials of two UNEQUAL shards, each called with inv_b_global = 1 / B, against torch
    autograd in float64 on the concatenated batch, per parameter array under the rule of tests/yardstick.py (error against float64
    at most 4 x float32 autograd's own + FLOOR); the scalar sums at the bars of the single-process test of the same entry point;
    and the exact scaling identity: inv_b_global = 1 / (2 rows) returns 0.5 x the call with 1 / rows bit for bit on the gradient
    and the loss, and the statistic sums (unscaled) bit-identical.
 2. learners - two 32-row shards of the reference's 64-row fixtures through a two-rank harness made of monkeypatch (dist.world_size
    -> 2; dist.all_reduce_sum_ captures rank 1's buffer in pass A and adds it in pass B): what rank 0 of a two-rank run holds,
    checked exactly as the learner's single-process golden test checks the full batch (clip after the reduce, B * world).
 3. step driver - a mirrored world (dist.world_size -> W, all_reduce_sum_ -> flat *= W: W ranks holding the same streams) is
    bit-identical to the one-process run after ten steps, natively (learner versions 1 .. 5) and method by method (SAC included).

The transport itself, and the rank-dependent staging of the one-shot exchange, stay with tests/test_dist_gpu.py (MPG-v2)."""
import functools

import numpy as np
import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import dist as D
from mpg_amd import ops
from oracle import mpg_oracle as O
from tests import dp_oracle as DP
from tests import ndpg_oracle as N
from tests import sac_oracle as S
from tests import yardstick as Y
from tests.golden_inputs import mlp_weights_flat, reset_law_obs

pytestmark = pytest.mark.gpu
DEV = 'cuda'
H = 256
PD = 'InvertedPendulumConti-v0'
ALPHA = S.ALPHA


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(params=['split', 'f32'])
def engine(request):
    """both builds of the library (mpg_amd/_lib.py ENGINES): the split-fp16 product and the exact-fp32 engine"""
    with L.engine(request.param):
        yield request.param


# =============================================================================================================================
# 1. entry points
# =============================================================================================================================
RAGGED = (40, 17)            # B, first shard: 17 + 23 rows, both below the 16-row group's multiple (entry points that take any row count)
GROUPS = (48, 16)            # 16 + 32 rows: mpg_mpg_gradients' fused path and the all-steps rollouts (rows * M % 16 == 0)
ACROSS = (8208, 8192)        # 8192 + 16: the first shard takes the many-block _mb kernels + the finish job (ERR_MB_MIN_ROWS, learner_api.hip),
#                              the second the one-block kernels
NET_SHAPES = [(B, cut, K) for B, cut in (RAGGED, ACROSS) for K in (0, 3)]        # K = 0 / 3: both sides of backward_takes_thin


def check_arrays(sharded, whole, r32, r64, nets, where):
    """the rule of tests/yardstick.py per parameter array (as check_arrays of tests/test_sac_gpu.py uses it) on the sum of the shard
    partials; the unsharded device call on the same rows is printed beside it (the two may differ by summation order only).
    nets: [(name, din, dout), ...] in the order of the flat vectors.  Every figure is printed before anything is asserted."""
    sharded, whole, r32, r64 = [np.asarray(v).ravel() for v in (sharded, whole, r32, r64)]
    o, rows = 0, []
    for name, din, dout in nets:
        for shp in O.mlp_shapes(din, H, dout):
            n = int(np.prod(shp))
            e_ref, e_sh, e_wh = [Y.rel_l2(v[o:o + n], r64[o:o + n]) for v in (r32, sharded, whole)]
            allow = 4.0 * e_ref + Y.FLOOR
            print('   %s %-6s %-10s sharded sum %.2e  unsharded call %.2e  float32 autograd %.2e  allowance %.2e' % (where, name, shp, e_sh, e_wh, e_ref, allow))
            rows.append((name, shp, e_sh, e_ref, allow))
            o += n
    assert o == sharded.size == whole.size == r32.size == r64.size, (o, sharded.size, whole.size, r32.size, r64.size)
    for name, shp, e_sh, e_ref, allow in rows:
        assert e_sh <= allow, (where, name, shp, 'vs float64: sharded sum %.3e, float32 autograd %.3e' % (e_sh, e_ref))
    return max(r[2] / r[4] for r in rows)


def check_scaling(run, lo, hi, scaled, unscaled, where):
    """inv_b_global = 1 / (2 rows) against 1 / rows on the same rows: the outputs that carry the factor are EXACTLY halved (a power
    of two: no rounding anywhere in a linear chain, barring underflow), the others do not move a bit"""
    rows = hi - lo
    u, h = run(lo, hi, 1.0 / rows), run(lo, hi, 1.0 / (2 * rows))
    for k in scaled:
        assert torch.isfinite(u[k]).all() and u[k].abs().max().item() > 0, (where, k)
        assert torch.equal(h[k], 0.5 * u[k]), (where, k, 'rows %d .. %d: not exactly half' % (lo, hi), (h[k] - 0.5 * u[k]).abs().max().item())
    for k in unscaled:
        assert torch.equal(bits(h[k]), bits(u[k])), (where, k, 'rows %d .. %d: an unscaled output moved with inv_b_global' % (lo, hi))


def sharded(run, B, cut):
    """(the unsharded call with 1 / B, the two shard calls with 1 / B)"""
    return run(0, B, 1.0 / B), [run(0, cut, 1.0 / B), run(cut, B, 1.0 / B)]


def rows_of(t, lo, hi):
    """rows lo .. hi of a device tensor as an allocation of their own, like the batch a rank holds"""
    return t[lo:hi].clone()


def f64sum(parts, k):
    return sum(host(p[k]).astype(np.float64) for p in parts)


@functools.lru_cache(maxsize=None)
def net_case(seed, B, K):
    """(computed once per set of arguments and shared by the engines; nothing in it is written to later) random networks, observations
    from the reset law (+ K look-ahead entries), actions, critic targets, rewards, draws"""
    rng = np.random.Generator(np.random.PCG64(seed))
    od = 6 + K
    w = {'policy': mlp_weights_flat(rng, od, 4), 'Q1': mlp_weights_flat(rng, od + 2, 1), 'Q2': mlp_weights_flat(rng, od + 2, 1)}
    obs = np.concatenate([reset_law_obs(rng, B), rng.standard_normal((B, K)).astype(np.float32)], 1)
    return dict(rows=B, od=od, K=K, scale=list(O.OBS_SCALE_PT) + [1.] * K, w=w, obs=obs, act=rng.uniform(-1, 1, (B, 2)).astype(np.float32),
                y=rng.standard_normal(B).astype(np.float32), eps=rng.standard_normal((B, 2)).astype(np.float32),
                rew=(-rng.uniform(0, 5, B)).astype(np.float32), gamma=0.98)


def ocfg_of(c):
    return O.Cfg(obs_dim=c['od'], obs_scale=c['scale'])


# ---- mpg_q_loss_grad --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def q_loss_reference(seed, B, K):
    c, out = net_case(seed, B, K), {}
    for dt in (torch.float32, torch.float64):
        ws = O.unflatten(c['w']['Q1'], c['od'] + 2, H, 1, dtype=dt, requires_grad=True)
        po = O.process_obses(ocfg_of(c), torch.as_tensor(c['obs']).to(dt))
        q = O.mlp(ws, torch.cat([po, torch.as_tensor(c['act']).to(dt)], 1), 'linear')[:, 0]
        loss = 0.5 * torch.mean((q - torch.as_tensor(c['y']).to(dt)) ** 2)
        out[dt] = (np.concatenate([x.numpy().ravel() for x in torch.autograd.grad(loss, ws)]), loss.item())
    return out


@pytest.mark.parametrize('B,cut,K', NET_SHAPES)
def test_q_loss_grad_shards(engine, B, cut, K):
    """k_row_sums<QErrRow>: the one-block form, and the many-block form + the finish job (k_finish_parts where the backward is not thin, K = 3; the extra block of
    the weight-gradient launch's summation where it is, K = 0).  td is unscaled: a shard's td equals the same rows of the unsharded
    call bit for bit.  Loss bar: test_q_loss_grad_vs_oracle_autograd_ragged (rtol 2e-5)."""
    c, ref = net_case(100 + B + K, B, K), q_loss_reference(100 + B + K, B, K)
    cfg = ops.make_cfg(obs_dim=c['od'], obs_scale=c['scale'])
    wq, obs, act, y = dev(c['w']['Q1']), dev(c['obs']), dev(c['act']), dev(c['y'])

    def run(lo, hi, inv_b):
        loss, grad, td = ops.q_loss_grad(cfg, wq, rows_of(obs, lo, hi), rows_of(act, lo, hi), rows_of(y, lo, hi), inv_b_global=inv_b, want_td=True)
        return dict(loss=loss, grad=grad, td=td)
    whole, parts = sharded(run, B, cut)
    where = 'q_loss_grad B %d = %d + %d K %d (%s)' % (B, cut, B - cut, K, engine)
    assert torch.equal(bits(parts[0]['td']), bits(whole['td'][:cut])) and torch.equal(bits(parts[1]['td']), bits(whole['td'][cut:])), where
    loss = f64sum(parts, 'loss')[0]
    print('   %s: loss sharded sum rel %.2e, unsharded rel %.2e' % (where, abs(loss / ref[torch.float64][1] - 1), abs(whole['loss'].item() / ref[torch.float64][1] - 1)))
    check_arrays(host(parts[0]['grad'] + parts[1]['grad']), host(whole['grad']), ref[torch.float32][0], ref[torch.float64][0],
                 [('Q1', c['od'] + 2, 1)], where)
    np.testing.assert_allclose(loss, ref[torch.float64][1], rtol=2e-5)
    for lo, hi in ((0, cut), (cut, B)):
        check_scaling(run, lo, hi, ('loss', 'grad'), ('td',), where)


# ---- mpg_td3_policy_grad / mpg_dpg_policy_grad ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dpg_reference(seed, B, K, two_critics):
    """-mean min(Q1, Q2)(s~, pi(s~)) (td3.py:120-134) or -mean Q1(s~, pi(s~)) (ndpg.py:174-186) and its policy gradient"""
    c, out = net_case(seed, B, K), {}
    names = ('policy', 'Q1', 'Q2') if two_critics else ('policy', 'Q1')
    for dt in (torch.float32, torch.float64):
        ocfg = ocfg_of(c)
        nets = O.Nets(ocfg, {k: c['w'][k] for k in names}, dtype=dt)
        po = O.process_obses(ocfg, torch.as_tensor(c['obs']).to(dt))
        a = nets.compute_action(po)
        q = nets.q('Q1', po, a)
        if two_critics:
            q = torch.minimum(q, nets.q('Q2', po, a))
        out[dt] = (np.concatenate([x.numpy().ravel() for x in torch.autograd.grad(-q.mean(), nets.w['policy'])]), q.detach().numpy().astype(np.float64))
    return out


@pytest.mark.parametrize('B,cut,K', NET_SHAPES)
def test_td3_policy_grad_shards(engine, B, cut, K):
    """k_row_sums<Td3DyRow>, one block and many.  The statistic sums as the learner reports them (value_mean = sum / B, value_var = sqsum / B - mean^2)
    at the bars of test_td3_compute_gradient_vs_golden (rtol 1e-4 atol 1e-7; value_var rtol 2e-3)."""
    c, ref = net_case(200 + B + K, B, K), dpg_reference(200 + B + K, B, K, True)
    cfg = ops.make_cfg(obs_dim=c['od'], obs_scale=c['scale'])
    wp, q1, q2, obs = dev(c['w']['policy']), dev(c['w']['Q1']), dev(c['w']['Q2']), dev(c['obs'])

    def run(lo, hi, inv_b):
        stats, grad = ops.td3_policy_grad(cfg, wp, q1, q2, rows_of(obs, lo, hi), inv_b_global=inv_b)
        return dict(stats=stats, grad=grad)
    whole, parts = sharded(run, B, cut)
    where = 'td3_policy_grad B %d = %d + %d K %d (%s)' % (B, cut, B - cut, K, engine)
    q64 = ref[torch.float64][1]
    st, stw = f64sum(parts, 'stats'), host(whole['stats']).astype(np.float64)
    mean, var = st[0] / B, st[1] / B - (st[0] / B) ** 2
    print('   %s: qmin_sum rel %.2e (unsharded %.2e), qmin_sqsum rel %.2e (unsharded %.2e)' % (
        where, abs(st[0] / q64.sum() - 1), abs(stw[0] / q64.sum() - 1), abs(st[1] / (q64 ** 2).sum() - 1), abs(stw[1] / (q64 ** 2).sum() - 1)))
    check_arrays(host(parts[0]['grad'] + parts[1]['grad']), host(whole['grad']), ref[torch.float32][0], ref[torch.float64][0],
                 [('policy', c['od'], 4)], where)
    np.testing.assert_allclose(mean, q64.mean(), rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(var, q64.var(), rtol=2e-3)
    for lo, hi in ((0, cut), (cut, B)):
        check_scaling(run, lo, hi, ('grad',), ('stats',), where)


@pytest.mark.parametrize('B,cut,K', NET_SHAPES)
def test_dpg_policy_grad_shards(engine, B, cut, K):
    """k_row_sums<DpgDyRow>, one block and many.  q_sum / q_sqsum at the bar of test_dpg_policy_grad_vs_float64_autograd_and_vs_the_td3_entry_point
    (1e-6 relative)."""
    c, ref = net_case(300 + B + K, B, K), dpg_reference(300 + B + K, B, K, False)
    cfg = ops.make_cfg(obs_dim=c['od'], obs_scale=c['scale'])
    wp, q1, obs = dev(c['w']['policy']), dev(c['w']['Q1']), dev(c['obs'])

    def run(lo, hi, inv_b):
        stats, grad = ops.dpg_policy_grad(cfg, wp, q1, rows_of(obs, lo, hi), inv_b_global=inv_b)
        return dict(stats=stats, grad=grad)
    whole, parts = sharded(run, B, cut)
    where = 'dpg_policy_grad B %d = %d + %d K %d (%s)' % (B, cut, B - cut, K, engine)
    q64 = ref[torch.float64][1]
    st, stw = f64sum(parts, 'stats'), host(whole['stats']).astype(np.float64)
    e_sum, e_sq = abs(st[0] - q64.sum()) / abs(q64.sum()), abs(st[1] - (q64 ** 2).sum()) / (q64 ** 2).sum()
    print('   %s: q_sum rel %.2e (unsharded %.2e), q_sqsum rel %.2e (unsharded %.2e)' % (
        where, e_sum, abs(stw[0] / q64.sum() - 1), e_sq, abs(stw[1] / (q64 ** 2).sum() - 1)))
    check_arrays(host(parts[0]['grad'] + parts[1]['grad']), host(whole['grad']), ref[torch.float32][0], ref[torch.float64][0],
                 [('policy', c['od'], 4)], where)
    assert e_sum <= 1e-6 and e_sq <= 1e-6, (where, e_sum, e_sq)
    for lo, hi in ((0, cut), (cut, B)):
        check_scaling(run, lo, hi, ('grad',), ('stats',), where)


# ---- mpg_sac_policy_grad ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sac_reference(seed, B, K):
    from tests.test_sac_gpu import reference        # policy.py:179-204 and sac.py:119-136 in torch on the recorded draws
    c = net_case(seed, B, K)
    return reference(c, torch.float32, ALPHA), reference(c, torch.float64, ALPHA)


@pytest.mark.parametrize('B,cut,K', NET_SHAPES)
def test_sac_policy_grad_shards(engine, B, cut, K):
    """the head's - alpha * inv_b term (k_sac_dlogits), k_row_sums<Td3DyRow> (one block and many) under it, and the three statistic sums at the bars of
    test_sac_targets_and_policy_grad_vs_float64_autograd"""
    c = net_case(400 + B + K, B, K)
    r32, r64 = sac_reference(400 + B + K, B, K)
    cfg = ops.make_cfg(obs_dim=c['od'], obs_scale=c['scale'], policy_out_activation='linear', gamma=c['gamma'])
    wp, q1, q2, obs, eps = dev(c['w']['policy']), dev(c['w']['Q1']), dev(c['w']['Q2']), dev(c['obs']), dev(c['eps'])

    def run(lo, hi, inv_b):
        stats, grad = ops.sac_policy_grad(cfg, wp, q1, q2, rows_of(obs, lo, hi), rows_of(eps, lo, hi), ALPHA, inv_b_global=inv_b)
        return dict(stats=stats, grad=grad)
    whole, parts = sharded(run, B, cut)
    where = 'sac_policy_grad B %d = %d + %d K %d (%s)' % (B, cut, B - cut, K, engine)
    s, sw = f64sum(parts, 'stats'), host(whole['stats']).astype(np.float64)
    want = (r64['qmin'].sum(), (r64['qmin'] ** 2).sum(), r64['logp'].sum())
    print('   %s: qmin_sum / qmin_sqsum / logp_sum rel %s (unsharded %s)' % (
        where, ' '.join('%.2e' % abs(a / b - 1) for a, b in zip(s, want)), ' '.join('%.2e' % abs(a / b - 1) for a, b in zip(sw, want))))
    check_arrays(host(parts[0]['grad'] + parts[1]['grad']), host(whole['grad']), r32['grad'], r64['grad'], [('policy', c['od'], 4)], where)
    np.testing.assert_allclose(s[0], want[0], rtol=2e-5, atol=2e-5 * B)
    np.testing.assert_allclose(s[1], want[1], rtol=1e-4, atol=1e-6 * B)
    np.testing.assert_allclose(s[2], want[2], rtol=2e-5, atol=2e-5 * B)
    for lo, hi in ((0, cut), (cut, B)):
        check_scaling(run, lo, hi, ('grad',), ('stats',), where)


# ---- mpg_rollout_pg ---------------------------------------------------------------------------------------------------------
def shard_eps(eps, B, M, lo, hi):
    """the columns of eps [n][M * B] (copy m of row r at column m * B + r, mpg_learner.py:226-233) that belong to rows lo .. hi"""
    n = eps.shape[0]
    return np.ascontiguousarray(eps.reshape(n, M, B)[:, :, lo:hi].reshape(n, M * (hi - lo)))


@pytest.mark.parametrize('env,M,select', [(PD, 1, (0, 25)), ('pt', 2, (0, 5, 25))], ids=['pendulum-nadp', 'path-tracking-M2'])
def test_rollout_pg_all_steps_shards(engine, env, M, select):
    """all_steps_param_grad = 1 (rows * M must be a multiple of 16: B = 48 = 16 + 32).  'pendulum-nadp': NADP's own call, slices
    [0, 25] with weights [0, 1].  'path-tracking-M2': two copies per row - the coefficients carry inv_b / M (make_coefs) and
    launch_wgrad is handed inv_b / M.  Reference and bars: tests/test_slices_gpu.py (oracle_arrays; ret_sum / rows rtol 5e-5 atol 1e-6,
    ret_sqsum rtol 2e-4 atol 1e-6)."""
    from tests import test_slices_gpu as SL
    B, cut = GROUPS
    n = 25
    ocfg, wp, wq, obs, eps = SL.inputs('pd' if env == PD else 'pt', B, M, n, 0, 900 + M)
    w = np.array([0.0, 1.0], np.float32) if env == PD else SL.weights(select)
    ref = {dt: SL.oracle_arrays(ocfg, wp, wq, obs, eps, select, w, True, dtype=dt) for dt in (torch.float32, torch.float64)}
    flat = {dt: np.concatenate([g.ravel() for g in ref[dt][0]]) for dt in ref}
    cfg = SL.device_cfg(ocfg)
    pol, q1, o = dev(wp), dev(wq), dev(obs)

    def run(lo, hi, inv_b):
        rs, rq, grad = ops.rollout_pg(cfg, pol, q1, rows_of(o, lo, hi), dev(shard_eps(eps, B, M, lo, hi)), list(select), w, M=M, inv_b_global=inv_b,
                                      all_steps_param_grad=True)
        return dict(ret_sum=rs.clone(), ret_sqsum=rq.clone(), grad=grad)
    whole, parts = sharded(run, B, cut)
    where = 'rollout_pg all steps %s M %d B %d = %d + %d (%s)' % (env, M, B, cut, B - cut, engine)
    din, dout = ocfg.obs_dim, 2 * ocfg.act_dim
    rs, rq = f64sum(parts, 'ret_sum'), f64sum(parts, 'ret_sqsum')
    _, red, m2 = ref[torch.float64]
    print('   %s: ret_sum / B rel %.2e  ret_sqsum rel %.2e' % (where, np.abs(rs / B / red - 1).max(), np.abs(rq / m2 - 1).max()))
    check_arrays(host(parts[0]['grad'] + parts[1]['grad']), host(whole['grad']), flat[torch.float32], flat[torch.float64], [('policy', din, dout)], where)
    np.testing.assert_allclose(rs / B, red, rtol=5e-5, atol=1e-6)
    np.testing.assert_allclose(rq, m2, rtol=2e-4, atol=1e-6)
    for lo, hi in ((0, cut), (cut, B)):
        check_scaling(run, lo, hi, ('grad',), ('ret_sum', 'ret_sqsum'), where)


N_DP = 10        # horizon of the double pendulum's ragged case (tests/test_double_pendulum_gpu.py, test_rows_not_a_multiple_of_16)


def test_rollout_pg_double_pendulum_shards(engine):
    """the double-pendulum model in the form that accepts any row count (parameter gradient through the first evaluation), 40 = 17 + 23
    rows of the reference's fixture, weights (0.3, 0.7) on slices (0, 10) - the case, horizon, restatement and bars of
    test_rows_not_a_multiple_of_16 (DP.rollout_policy_update; return sums under Y.check_values)"""
    import os
    B, cut = RAGGED
    inp, _ = DP.load_case(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'), 256, 25)
    obs_np = inp['batch_obs'][:B]
    ref = {}
    for dt in (torch.float32, torch.float64):
        ocfg = DP.make_cfg(N_DP)
        nets = DP.nets_of(ocfg, inp, dt)
        red = DP.rollout_policy_update(ocfg, nets, torch.as_tensor(obs_np).to(dt), N_DP, all_steps_param_grad=False)
        loss = -(0.3 * red[0] + 0.7 * red[N_DP])
        ref[dt] = (np.concatenate([x.numpy().ravel() for x in torch.autograd.grad(loss, nets.w['policy'])]),
                   np.array([red[0].item(), red[N_DP].item()]) * B)
    cfg = ops.make_cfg(DP.ENV_ID)
    pol, q1, obs = dev(inp['w_policy']), dev(inp['w_Q1']), dev(obs_np)

    def run(lo, hi, inv_b):
        rs, rq, grad = ops.rollout_pg(cfg, pol, q1, rows_of(obs, lo, hi), None, [0, N_DP], [0.3, 0.7], n=N_DP, inv_b_global=inv_b)
        return dict(ret_sum=rs.clone(), ret_sqsum=rq.clone(), grad=grad)
    whole, parts = sharded(run, B, cut)
    where = 'rollout_pg double pendulum B %d = %d + %d (%s)' % (B, cut, B - cut, engine)
    check_arrays(host(parts[0]['grad'] + parts[1]['grad']), host(whole['grad']), ref[torch.float32][0], ref[torch.float64][0], [('policy', 11, 2)], where)
    Y.check_values(f64sum(parts, 'ret_sum'), ref[torch.float32][1], ref[torch.float64][1], what='return sums ' + where)
    for lo, hi in ((0, cut), (cut, B)):
        check_scaling(run, lo, hi, ('grad',), ('ret_sum', 'ret_sqsum'), where)


# ---- mpg_mpg_gradients ------------------------------------------------------------------------------------------------------
MG_ITERATION = 4500      # lam = 1: the rule gives every slice the same weight, so each one matters (tests/test_slices_gpu.py)
# The three fused critic bodies that multiply by inv_b (fused_kernels.hip; launch_critic_fused / launch_qloss_fused):
#   k_qloss_fused    n_select != 2 (rows % 16 == 0, M == 1):                                    the (0, 5, 25) cases at B = 48
#   k_critic_fused   n_select == 2, and fewer than 256 row groups or no packed weight images:   the (0, 25) cases at B = 48, and the 16-row
#                    shard (and the unsharded 4112-row call: 257 groups, not a multiple of 4) of the B = 4112 case
#   k_critic_fused4  n_select == 2, packed images of both critics, >= 256 row groups, a multiple of 4: the 4096-row shard of the
#                    B = 4112 case (both in the sharded sum and, with two scales, in the scaling identity); two critics there, so the
#                    split target (y finished inside the critic launch) runs with it
MG_CASES = [(48, 16, 1, (0, 25), False), (48, 16, 2, (0, 25), False), (48, 16, 1, (0, 5, 25), False), (48, 16, 2, (0, 5, 25), False),
            (4112, 4096, 2, (0, 25), True)]


@functools.lru_cache(maxsize=None)
def mg_case(B, n_q, select):
    """Inputs and the float32 / float64 references of one mpg_mpg_gradients case (the oracle functions of
    test_mpg_gradients_with_one_and_three_slices; a 25-step rollout of 4112 rows takes about two seconds in float64).

    Seed: that test's formula, B + 10 n_q + n_select - but 1071 instead of 71 for (48, 2, (0, 5, 25)), by a condition on the inputs
    that the oracle alone decides.  The rule measures the device against ONE float32 autograd run, which has to be representative of
    float32 arithmetic on the inputs.  `assoc` holds the error against float64 of the float32 policy gradient taken two ways: one
    autograd pass over the weighted loss, and slice by slice (summed afterwards).  On seeds 60, 70, 61, 4134 and 1071 both are
    2.3e-7 .. 1.5e-6 and within 15 % of each other, on two hosts.  On seed 71 they are 3.7e-6 / 4.0e-6 on one host (slice 25 alone: 4.2e-6) while the one-pass run of another host
    landed at 8.2e-7 (per array 3.2e-7 .. 8.2e-7): float32 is ten times noisier on that input than elsewhere and a single run of it
    says little.  (The device on seed 71, both engines, sharded sum and unsharded call alike: 3.8e-6 .. 7.9e-6 on the policy arrays -
    inside four times the first host's float32 run, outside four times the second's.)"""
    seed = {(48, 2, (0, 5, 25)): 1071}.get((B, n_q, select), B + 10 * n_q + len(select))
    rng = np.random.Generator(np.random.PCG64(seed))
    names = ['Q1', 'policy'] if n_q == 1 else ['Q1', 'Q2', 'policy']
    w = {nm: mlp_weights_flat(rng, 6, 4) if nm == 'policy' else mlp_weights_flat(rng, 8, 1) for nm in names}
    obs, obs2 = reset_law_obs(rng, B), reset_law_obs(rng, B)
    act, rew = rng.uniform(-1, 1, (B, 2)).astype(np.float32), rng.uniform(-30, 0, B).astype(np.float32)
    eps = rng.standard_normal((25, B)).astype(np.float32)
    ocfg = O.Cfg(select=list(select), clip=1e30)
    ws = O.rule_based_weights(MG_ITERATION, ocfg.total_ite, ocfg.eta, ocfg.select).numpy()        # float32, as the learners hand them over
    assert ws.min() > 0.2 / len(select)
    ref = {}
    for dt in (torch.float32, torch.float64):
        nets = O.Nets(ocfg, w, target_scale=0.97, dtype=dt)
        t = lambda x: torch.as_tensor(x).to(dt)
        if n_q == 2:
            y = O.clipped_double_q_target(ocfg, nets, t(rew), t(obs2))
        else:       # one critic: r~ + gamma * Q1_target(s', pi_target(s'))  (mpg_learner.py:126-134 without the second critic)
            with torch.no_grad():
                po1 = O.process_obses(ocfg, t(obs2))
                y = O.process_rewards(ocfg, t(rew)) + ocfg.gamma * nets.q('Q1_target', po1, nets.compute_target_action(po1))
        q_losses, q_grads = O.q_forward_and_backward(ocfg, nets, t(obs), t(act), y, names[:-1])
        reduced, _, allret = O.model_rollout_for_policy_update(ocfg, nets, t(obs), t(eps))
        by_slice = [torch.autograd.grad(-float(wk) * reduced[k], nets.w['policy'], retain_graph=True) for wk, k in zip(ws, select)]
        pg = torch.autograd.grad(-sum(float(wk) * reduced[k] for wk, k in zip(ws, select)), nets.w['policy'])
        ref[dt] = dict(pg=np.concatenate([g.numpy().ravel() for g in pg]),
                       pg_by_slice=sum(np.concatenate([g.numpy().ravel() for g in gs]) for gs in by_slice), grad=np.concatenate([g.numpy().ravel() for gl in q_grads for g in gl] + [g.numpy().ravel() for g in pg]),
                       y=y.numpy(), losses=np.array([l.item() for l in q_losses]), red=reduced[list(select)].detach().numpy(),
                       m2=(allret[list(select)] ** 2).sum(1).detach().numpy())
    r32, r64 = ref[torch.float32], ref[torch.float64]
    assoc = (Y.rel_l2(r32['pg'], r64['pg']), Y.rel_l2(r32['pg_by_slice'], r64['pg']))
    return dict(seed=seed, assoc=assoc, names=names, w=w, obs=obs, obs2=obs2, act=act, rew=rew, eps=eps, ws=ws, ref=ref)


@pytest.mark.parametrize('B,cut,n_q,select,packed', MG_CASES)
def test_mpg_gradients_shards(engine, B, cut, n_q, select, packed):
    """the one-call MPG gradient (targets computed inside): every array of the complete [Q1 | (Q2) | policy] gradient, the critic
    losses (scaled), y_out of a shard against the reference's rows, the slice statistics (unscaled) - the scalar bars of
    test_mpg_gradients_with_one_and_three_slices.  Which case reaches which fused critic body: the comment above MG_CASES."""
    c = mg_case(B, n_q, select)
    names, ws, ns, r32, r64 = c['names'], c['ws'], len(select), c['ref'][torch.float32], c['ref'][torch.float64]
    cfg = ops.make_cfg()
    params = dev(np.concatenate([c['w'][nm] for nm in names]))
    targets = dev(np.concatenate([(c['w'][nm] * np.float32(0.97)).astype(np.float32) for nm in names]))
    if packed:       # the packed images of both flat vectors hang in the cfg for the calls (kept alive by `caches`)
        dims = [(6, 4) if nm == 'policy' else (8, 1) for nm in names]
        caches = [ops.WeightCache(params, dims), ops.WeightCache(targets, dims)]
        cfg.wcache[0], cfg.wcache[1] = caches[0].pointer, caches[1].pointer
    obs, act, rew, obs2 = dev(c['obs']), dev(c['act']), dev(c['rew']), dev(c['obs2'])

    def run(lo, hi, inv_b):
        grad, stats, y_out = torch.zeros(params.numel(), device=DEV), torch.zeros(16, device=DEV), torch.zeros(hi - lo, device=DEV)
        ops.mpg_gradients(cfg, n_q, params, targets, rows_of(obs, lo, hi), rows_of(act, lo, hi), rows_of(rew, lo, hi), rows_of(obs2, lo, hi), None, list(select), ws, grad, stats, y_out,
                          eps=dev(c['eps'][:, lo:hi]), inv_b_global=inv_b)
        return dict(grad=grad, loss=stats[:n_q].clone(), sums=stats[2:2 + 2 * ns].clone(), y=y_out)
    whole, parts = sharded(run, B, cut)
    torch.cuda.synchronize()
    where = 'mpg_gradients B %d = %d + %d nq %d sel %s (%s)' % (B, cut, B - cut, n_q, list(select), engine)
    print('   %s: seed %d; float32 policy gradient vs float64, one pass %.2e, slice by slice %.2e' % ((where, c['seed']) + c['assoc']))
    losses, sums = f64sum(parts, 'loss'), f64sum(parts, 'sums')
    print('   %s: losses %s vs %s; ret_sum / B rel %.2e  ret_sqsum rel %.2e' % (
        where, losses, r64['losses'], np.abs(sums[:ns] / B / r64['red'] - 1).max(), np.abs(sums[ns:] / r64['m2'] - 1).max()))
    nets = [(nm, 6, 4) if nm == 'policy' else (nm, 8, 1) for nm in names]
    check_arrays(host(parts[0]['grad'] + parts[1]['grad']), host(whole['grad']), r32['grad'], r64['grad'], nets, where)
    for p, (lo, hi) in zip(parts, ((0, cut), (cut, B))):
        np.testing.assert_allclose(host(p['y']), r64['y'][lo:hi], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(losses, r64['losses'], rtol=5e-5, atol=1e-6)
    np.testing.assert_allclose(sums[:ns] / B, r64['red'], rtol=5e-5, atol=1e-6)
    np.testing.assert_allclose(sums[ns:], r64['m2'], rtol=2e-4, atol=1e-6)
    for lo, hi in ((0, cut), (cut, B)):
        check_scaling(run, lo, hi, ('grad', 'loss'), ('sums', 'y'), where)
    if packed:
        del caches


# =============================================================================================================================
# 2. learners: two 32-row shards of the reference's 64-row fixtures, in one process
# =============================================================================================================================
BATCH_KEYS = ('batch_obs', 'batch_actions', 'batch_rewards', 'batch_obs_tp1', 'batch_dones')
SHARDS = ((0, 32), (32, 64))


def on_two_ranks(monkeypatch, make_learner, compute):
    """What rank 0 of a two-rank run holds after compute_gradient.  dist.world_size answers 2.  Pass A: a learner on shard 1, with
    dist.all_reduce_sum_ handing back the flat [gradients | statistics] buffer unchanged after keeping a copy.  Pass B: a fresh learner
    with the same weights on shard 0, with dist.all_reduce_sum_ adding pass A's copy (rank order 0 + 1, the one-shot exchange's
    association).  compute(learner, lo, hi) calls compute_gradient on rows lo .. hi.  Returns (rank 0's learner, its gradient list)."""
    monkeypatch.setattr(D, 'world_size', lambda: 2)
    held = []

    def capture(flat, **kw):
        held.append(flat.clone())
        return flat

    def add(flat, **kw):
        flat.add_(held[-1])
        return flat
    monkeypatch.setattr(D, 'all_reduce_sum_', capture)
    compute(make_learner(), *SHARDS[1])
    assert len(held) == 1
    monkeypatch.setattr(D, 'all_reduce_sum_', add)
    mine = make_learner()
    assert mine.batch_size * D.world_size() == 64
    return mine, compute(mine, *SHARDS[0])


def shard_batch(g, lo, hi):
    return [dev(g[k][lo:hi]) for k in BATCH_KEYS]


def flat_of(grads):
    return torch.cat([x.reshape(-1) for x in grads]).cpu().numpy()


def nets_of(pw):
    return [(n,) + tuple(pw.dims[n]) for n in pw.names]


def load_weights(learner, w, target_scale):
    pw = learner.policy_with_value
    flat = np.concatenate([w[n] for n in pw.names]).astype(np.float32)
    pw.set_flat(flat, (flat * np.float32(target_scale)).astype(np.float32))
    return learner


@pytest.mark.parametrize('version,K', [('v2', 0), ('v1', 0), ('v2', 3)])
def test_mpg_learner_two_shards_vs_reference_golden(golden, monkeypatch, engine, version, K):
    """MPG-v2 (the control against the spawned ranks of tests/test_dist_gpu.py) and MPG-v1: the asserts of
    tests/test_learner_gpu.py::test_compute_gradient_vs_reference_golden.  The targets and the td error are per process: against
    the fixture's rows of the shard.  K = 3 (observations 9 wide) leaves mpg_mpg_gradients' fused kernels for its fall-back, which
    hands inv_b_global on to mpg_q_loss_grad and mpg_rollout_pg."""
    from mpg_amd.config import default_args
    from mpg_amd.learners import MPGLearner
    from mpg_amd.policy import PolicyWithQs
    g = golden('mpg_%s_H256_B64%s.npz' % (version, '_K%d' % K if K else ''))

    def make_learner():
        learner = MPGLearner(PolicyWithQs, default_args('MPG-' + version, replay_batch_size=32, num_batch_reuse=1, num_future_data=K))
        assert learner.policy_with_value.cfg.obs_dim == 6 + K
        return load_weights(learner, {n: g['w_' + n] for n in learner.policy_with_value.names}, g['target_scale'])
    for it in (100, 9000):
        learner, grads = on_two_ranks(monkeypatch, make_learner, lambda ln, lo, hi: ln.compute_gradient(
            shard_batch(g, lo, hi), None, None, it, eps=dev(g['eps'][:, lo:hi])))
        pw = learner.policy_with_value
        assert len(grads) == (18 if version == 'v2' else 12)
        p = 'it%d_' % it
        Y.check_gradients(flat_of(grads), g[p + 'grads'], g[p + 'grads_f64'], nets_of(pw), where='MPG-%s K=%d it %d two shards (%s)' % (version, K, it, engine))
        st = learner.get_stats()
        for k in ('value_mean', 'policy_total_loss', 'policy_gradient_norm', 'q_loss1', 'q_gradient_norm1', 'q_loss2', 'q_gradient_norm2'):
            if p + k in g:
                np.testing.assert_allclose(st[k], g[p + k], rtol=2e-5, atol=1e-6, err_msg=k)
        np.testing.assert_allclose(st['w_list'], g[p + 'w_list'], rtol=1e-5, atol=1e-9)
        np.testing.assert_allclose(st['all_losses'], g[p + 'all_losses'], rtol=2e-5, atol=1e-6)
        lo, hi = SHARDS[0]
        Y.check_values(host(learner.batch_data['batch_targets']), g[p + 'targets'][lo:hi], g[p + 'targets_f64'][lo:hi], what='targets MPG-%s' % version)
    np.testing.assert_allclose(host(learner.compute_td_error()), g['td_error'][lo:hi], rtol=1e-4, atol=2e-5)


def test_nadp_learner_two_shards_vs_reference_golden(golden, monkeypatch, engine):
    """NADP on the pendulum model: the asserts of tests/test_config34_gpu.py::test_pendulum_model_rollout_q_target_and_nadp_gradient_vs_golden
    (its helper _check_list and its bars); the Q target of the shard against the float64 oracle's rows of the shard"""
    from mpg_amd.config import default_args
    from mpg_amd.learners import NADPLearner
    from mpg_amd.policy import PolicyWithQs
    from tests.test_config34_gpu import _check_list
    g = golden('nadp_H256_B64.npz')

    def make_learner():
        return load_weights(NADPLearner(PolicyWithQs, default_args('NADP', replay_batch_size=32)), {n: g['w_' + n] for n in ('Q1', 'policy')},
                            g['target_scale'])

    def compute(ln, lo, hi):
        obs, z = dev(g['batch_obs'][lo:hi]), torch.zeros(hi - lo, device=DEV)
        return ln.compute_gradient([obs, dev(g['batch_actions'][lo:hi]), z, obs, z], None, None, 0, eps_q=dev(g['eps_q'][:, lo:hi]),
                                   eps_pi=dev(g['eps_pi'][:, lo:hi]))
    learner, grads = on_two_ranks(monkeypatch, make_learner, compute)
    st = learner.get_stats()
    for k in ('q_loss', 'policy_loss', 'value_mean', 'q_gradient_norm', 'policy_gradient_norm'):
        np.testing.assert_allclose(st[k], g[k], rtol=3e-4, atol=1e-6, err_msg=k)
    _check_list(grads, g['grads'], learner.policy_with_value, 2e-4)
    ocfg = O.Cfg(env=PD, select=[25], delay_update=1)
    nets = O.Nets(ocfg, {k: g['w_' + k] for k in ('Q1', 'policy')}, target_scale=g['target_scale'], dtype=torch.float64)
    _, ost = O.nadp_compute_gradient(ocfg, nets, [g['batch_obs'], g['batch_actions']], g['eps_q'], g['eps_pi'])
    lo, hi = SHARDS[0]
    np.testing.assert_allclose(host(learner.batch_data['batch_targets']), ost['targets'][lo:hi], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize('n', [25, 10])
def test_nadp_double_pendulum_two_shards_vs_reference(monkeypatch, engine, n):
    """NADP on the double pendulum: the asserts of tests/test_double_pendulum_gpu.py::test_nadp_gradient_vs_reference"""
    import os
    from mpg_amd.config import default_args
    from mpg_amd.learners import NADPLearner
    from mpg_amd.policy import PolicyWithQs
    inp, g = DP.load_case(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'), 256, n)
    dp_nets = [('Q1', 12, 1), ('policy', 11, 2)]

    def make_learner():
        args = default_args('NADP', env_id=DP.ENV_ID, replay_batch_size=32, num_rollout_list_for_policy_update=[n], num_rollout_list_for_q_estimation=[n])
        return load_weights(NADPLearner(PolicyWithQs, args), {'Q1': inp['w_Q1'], 'policy': inp['w_policy']}, inp['target_scale'])

    def compute(ln, lo, hi):
        obs, z = dev(inp['batch_obs'][lo:hi]), torch.zeros(hi - lo, device=DEV)
        return ln.compute_gradient([obs, dev(inp['batch_actions'][lo:hi]), z, obs, z], None, None, 0)
    learner, grads = on_two_ranks(monkeypatch, make_learner, compute)
    st = learner.get_stats()
    where = '%s n=%d two shards' % (engine, n)
    worst = Y.check_gradients(host(learner.flat_grad), g['grads'], g['grads_f64'], dp_nets, where=where, small64=g['small64'])
    print('%s: worst error / allowance %.3f' % (where, worst))
    lo, hi = SHARDS[0]
    Y.check_values(host(learner.batch_data['batch_targets']), g['targets'][lo:hi], g['targets_f64'][lo:hi], what='targets')
    for k in ('q_loss', 'policy_loss', 'value_mean', 'q_gradient_norm', 'policy_gradient_norm'):
        Y.check_values(st[k], g[k], g[k + '_f64'], what=k)
    assert learner.policy_with_value.check_status() == 0


def test_td3_learner_two_shards_vs_reference_golden(golden, monkeypatch, engine):
    """TD3: the asserts of tests/test_config34_gpu.py::test_td3_compute_gradient_vs_golden; the td error is per process"""
    from mpg_amd.config import default_args
    from mpg_amd.learners import TD3Learner
    from mpg_amd.policy import PolicyWithQs
    from tests.test_config34_gpu import _check_list
    g = golden('td3_H256_B64.npz')

    def make_learner():
        return load_weights(TD3Learner(PolicyWithQs, default_args('TD3', replay_batch_size=32)), {n: g['w_' + n] for n in ('Q1', 'Q2', 'policy')},
                            g['target_scale'])
    learner, grads = on_two_ranks(monkeypatch, make_learner, lambda ln, lo, hi: ln.compute_gradient(
        shard_batch(g, lo, hi), None, None, 0, smooth_eps=dev(g['smooth_eps'][lo:hi])))
    st = learner.get_stats()
    for k in ('q_loss1', 'q_loss2', 'policy_loss', 'value_mean', 'q_gradient_norm1', 'q_gradient_norm2', 'policy_gradient_norm'):
        np.testing.assert_allclose(st[k], g[k], rtol=1e-4, atol=1e-7, err_msg=k)
    np.testing.assert_allclose(st['value_var'], g['value_var'], rtol=2e-3)
    _check_list(grads, g['grads'], learner.policy_with_value, 1e-4)
    lo, hi = SHARDS[0]
    np.testing.assert_allclose(host(learner.compute_td_error()), g['td_error'][lo:hi], rtol=1e-4, atol=3e-6)


def check_clipped_norms(got, pw, stats, fixture, keys, clip):
    """the norms of the returned arrays: min(clip, the reference's norm) per network (the bars of the NDPG / SAC golden tests)"""
    off = np.cumsum([0] + list(pw.sizes))
    for i, k in enumerate(keys):
        n = np.linalg.norm(got[off[i]:off[i + 1]].astype(np.float64))
        np.testing.assert_allclose(n, min(clip, float(fixture[k])), rtol=1e-5 if float(fixture[k]) > clip else 1e-4, err_msg=k)


@pytest.mark.parametrize('K', [0, 3])
def test_ndpg_learner_two_shards_vs_reference_golden(golden, monkeypatch, engine, K):
    """NDPG: the asserts of tests/test_ndpg_gpu.py::test_compute_gradient_vs_reference_golden.  Per process, against the fixture's rows
    of the shard: the targets, mb_targets_mean (learners.py: 'this process's batch'), the sampler's rewards / last observation, the td
    error."""
    from mpg_amd.config import default_args
    from mpg_amd.learners import NDPGLearner
    from mpg_amd.policy import PolicyWithQs
    g = golden('ndpg_H256_B64%s.npz' % ('_K%d' % K if K else ''))

    def make_learner():
        learner = NDPGLearner(PolicyWithQs, default_args('NDPG', replay_batch_size=32, num_batch_reuse=1, num_future_data=K))
        assert learner.policy_with_value.names == ['Q1', 'policy']
        return load_weights(learner, N.fixture_weights(int(g['weights_seed']), K), g['target_scale'])
    learner, grads = on_two_ranks(monkeypatch, make_learner, lambda ln, lo, hi: ln.compute_gradient(shard_batch(g, lo, hi), None, None, 0))
    pw = learner.policy_with_value
    assert len(grads) == 12
    got = flat_of(grads)
    where = 'NDPG K=%d two shards (%s)' % (K, engine)
    worst = Y.check_gradients(got, g['grads'], g['grads_f64'], nets_of(pw), where=where, small64=g['small64'])
    print(where, 'worst error / allowance %.3f' % worst)
    lo, hi = SHARDS[0]
    Y.check_values(host(learner.batch_data['batch_targets']), g['targets'][lo:hi], g['targets_f64'][lo:hi], what='targets ' + where)
    batch = shard_batch(g, lo, hi)
    ro = learner.sample(batch[0], batch[1])
    np.testing.assert_allclose(host(ro['all_rewards']), g['nstep_all_rewards'][:, lo:hi], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(host(ro['last_obs']), g['nstep_last_obs'][lo:hi], rtol=0, atol=2e-3)
    st = learner.get_stats()
    for k in ('q_loss', 'policy_loss', 'value_mean', 'q_gradient_norm', 'policy_gradient_norm'):
        np.testing.assert_allclose(st[k], g[k], rtol=1e-4, atol=1e-7, err_msg=k)
    np.testing.assert_allclose(st['mb_targets_mean'], g['targets'][lo:hi].mean(), rtol=1e-4, atol=1e-7, err_msg='mb_targets_mean of the shard')
    assert st['q_gradient_norm'] > 3.0                                # the clip is exercised - after the reduce
    mean, var = float(g['value_mean_f64']), float(g['value_var_f64'])
    np.testing.assert_allclose(st['value_var'], g['value_var'], rtol=1e-4 * (var + 3 * mean * mean) / var)
    off = np.cumsum([0] + list(pw.sizes))
    nq, npi = np.linalg.norm(got[off[0]:off[1]].astype(np.float64)), np.linalg.norm(got[off[1]:off[2]].astype(np.float64))
    np.testing.assert_allclose(nq, min(3.0, float(g['q_gradient_norm'])), rtol=1e-5)
    np.testing.assert_allclose(npi, min(3.0, float(g['policy_gradient_norm'])), rtol=1e-4)
    np.testing.assert_allclose(host(learner.compute_td_error()), g['td_error'][lo:hi], rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize('K', [0, 3])
def test_sac_learner_two_shards_vs_reference_golden(golden, monkeypatch, engine, K):
    """SAC (fixed temperature): the asserts of tests/test_sac_gpu.py::test_compute_gradient_vs_reference_golden.  Per process, against
    the fixture's rows of the shard: the targets, mb_targets_mean, the head's log-densities."""
    from mpg_amd.config import default_args
    from mpg_amd.learners import SACLearner
    from mpg_amd.policy import PolicyWithQs
    g = golden('sac_H256_B64%s.npz' % ('_K%d' % K if K else ''))

    def make_learner():
        learner = SACLearner(PolicyWithQs, default_args('SAC', replay_batch_size=32, num_future_data=K, gradient_clip_norm=S.CLIP))
        pw = learner.policy_with_value
        assert pw.names == ['Q1', 'Q2', 'policy'] and pw.alpha == S.ALPHA
        return load_weights(learner, S.fixture_weights(int(g['weights_seed']), K), g['target_scale'])
    learner, grads = on_two_ranks(monkeypatch, make_learner, lambda ln, lo, hi: ln.compute_gradient(
        shard_batch(g, lo, hi), None, None, 0, eps_target=dev(g['eps_target'][lo:hi]), eps_policy=dev(g['eps_policy'][lo:hi])))
    pw = learner.policy_with_value
    assert len(grads) == 18
    got = flat_of(grads)
    where = 'SAC K=%d two shards (%s)' % (K, engine)
    worst = Y.check_gradients(got, g['grads'], g['grads_f64'], nets_of(pw), where=where, small64=g['small64'])
    print(where, 'worst error / allowance %.3f' % worst)
    lo, hi = SHARDS[0]
    Y.check_values(host(learner.batch_data['batch_targets']), g['targets'][lo:hi], g['targets_f64'][lo:hi], what='targets ' + where)
    for key, obs_key, eps_key in (('logp_target', 'batch_obs_tp1', 'eps_target'), ('logp_policy', 'batch_obs', 'eps_policy')):
        logp = host(pw.compute_action(dev(g[obs_key][lo:hi]), dev(g[eps_key][lo:hi]))[1])
        Y.check_values(logp, g[key][lo:hi], g[key + '_f64'][lo:hi], what=key + ' ' + where)
    st = learner.get_stats()
    for k in ('q_loss1', 'q_loss2', 'policy_loss', 'policy_entropy', 'value_mean', 'q_gradient_norm1', 'q_gradient_norm2', 'policy_gradient_norm'):
        np.testing.assert_allclose(st[k], g[k], rtol=1e-4, atol=1e-7, err_msg=k)
    np.testing.assert_allclose(st['mb_targets_mean'], g['targets'][lo:hi].mean(), rtol=1e-4, atol=1e-7, err_msg='mb_targets_mean of the shard')
    mean, var = float(g['value_mean_f64']), float(g['value_var_f64'])
    np.testing.assert_allclose(st['value_var'], g['value_var'], rtol=1e-4 * (var + 3 * mean * mean) / var)
    assert max(st['q_gradient_norm1'], st['q_gradient_norm2']) > S.CLIP > st['policy_gradient_norm']
    check_clipped_norms(got, pw, st, g, ('q_gradient_norm1', 'q_gradient_norm2', 'policy_gradient_norm'), S.CLIP)


# =============================================================================================================================
# 3. the step drivers: a mirrored world is bit-identical to one process
# =============================================================================================================================
STEPS = 10
TINY = 2.0 ** -120         # no nonzero entry of the one-process run's pre-exchange buffer below it: a quarter of it is still a normal float32


def build_stack(kind, fused, always_exchange):
    """the small stacks of the native-versus-method tests (tests/test_learner_gpu.py, test_config34_gpu.py, test_ndpg_gpu.py,
    test_sac_gpu.py), sampling every third iteration"""
    from mpg_amd.buffer import PrioritizedReplayBuffer, ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import MPGLearner, NADPLearner, NDPGLearner, SACLearner, TD3Learner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    sizes = dict(num_agent=64, batch_size=128, replay_batch_size=96, replay_starts=512, max_buffer_size=1000)
    per = kind == 'TD3-per'
    if kind in ('MPG-v1', 'MPG-v2'):
        cls, args = MPGLearner, default_args(kind, num_batch_reuse=2 if kind == 'MPG-v1' else 1, **sizes)
    elif kind == 'NADP':
        cls, args = NADPLearner, default_args('NADP', **sizes)
    elif kind in ('TD3', 'TD3-per'):
        cls, args = TD3Learner, default_args('TD3', buffer_type='priority' if per else 'normal', **sizes)
    elif kind == 'NDPG':
        cls, args = NDPGLearner, default_args('NDPG', num_agent=8, batch_size=128, replay_batch_size=64, replay_starts=256, max_buffer_size=1024,
                                              num_batch_reuse=2)
    else:
        cls, args = SACLearner, default_args('SAC', seed=5, num_agent=64, batch_size=64, replay_batch_size=128, replay_starts=256, max_buffer_size=1024)
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    learner = cls(PolicyWithQs, args)
    rb = (PrioritizedReplayBuffer if per else ReplayBuffer)(args, 0)
    opt = SingleProcessOffPolicyOptimizer(worker, learner, rb, None, args, sampling_interval=3, fused=fused, always_exchange=always_exchange)
    assert (opt._fused is not None) == fused, kind
    return opt


def snapshot(opt):
    """everything a step moves: parameters, targets, Adam moments, norms, the reduced and clipped gradient (the statistics slots behind it hold W times
    the one-process sums in a world of W - they are compared through get_stats(), which divides by batch_size * W), the replay ring
    (and the priority trees), the worker's observations; every counter; get_stats()"""
    pw, rb, w, ln = opt.worker.policy_with_value, opt.replay_buffer, opt.worker, opt.learner
    torch.cuda.synchronize()
    tensors = dict(params=pw.params, targets=pw.targets, adam_m=pw.m, adam_v=pw.v, norms=ln.norms, grad=ln.flat[:ln.n_grad], ring_obs=rb.obs, ring_act=rb.act,
                   ring_rew=rb.rew, ring_obs2=rb.obs2, ring_done=rb.done, worker_obs=w.obs)
    for k in ('_it_sum', '_it_min', '_max_priority'):
        if hasattr(rb, k):
            tensors['per' + k] = getattr(rb, k)
    counters = dict(opt_steps=dict(pw.opt_steps), ring_next=rb._next_idx, ring_len=len(rb), replay_times=rb.replay_times, noise_ctr=w._noise_ctr,
                    env_ctr=getattr(w.env, '_ctr', None), learner_counter=ln.counter, sample_ctr=getattr(pw, '_sample_ctr', None),
                    num_sampled_steps=opt.num_sampled_steps, iteration=opt.iteration)
    return {k: v.clone() for k, v in tensors.items()}, counters, ln.get_stats()


def run_world(monkeypatch, kind, fused, world):
    """STEPS optimizer steps.  world 1: the one-process run (natively with always_exchange, so that it takes the exchanged form of the
    step like the mirrored run); dist.all_reduce_sum_ only looks at the buffer.  world W: dist.world_size answers W and
    dist.all_reduce_sum_ multiplies the buffer by W - W ranks that hold the same streams and so the same partials.
    Returns (snapshot, the smallest nonzero magnitude the exchange saw)."""
    smallest = []

    def exchange(flat, **kw):
        nz = flat[flat != 0].abs()
        smallest.append(nz.min().item() if nz.numel() else float('inf'))
        assert torch.isfinite(flat).all()
        if world > 1:
            flat.mul_(world)
        return flat
    monkeypatch.setattr(D, 'world_size', lambda: world)
    monkeypatch.setattr(D, 'all_reduce_sum_', exchange)
    opt = build_stack(kind, fused, always_exchange=(world == 1))
    if fused:
        assert opt._fused.c.world_size == world and opt._fused.c.grads_exchanged == 1
    for _ in range(STEPS):
        opt.step()
    assert len(smallest) == STEPS, 'one exchange per step'
    return snapshot(opt), min(smallest)


def check_mirrored_worlds(monkeypatch, kind, fused):
    (ta, ca, sa), smallest = run_world(monkeypatch, kind, fused, 1)
    # the condition of the exactness argument: 1 / (B W) = (1 / B) / W exactly, every product with it is an exact division by a power of
    # two and the multiplication by W undoes it - as long as no value leaves the normal range on the way down
    assert smallest >= TINY, (kind, 'a nonzero entry of the pre-exchange buffer is below 2^-120', smallest)
    assert all(torch.isfinite(ta[k]).all() for k in ('params', 'targets', 'adam_m', 'adam_v', 'norms', 'grad'))
    assert ta['grad'].abs().max().item() > 0 and ta['norms'].min().item() > 0
    for world in (2, 4):
        (tb, cb, sb), _ = run_world(monkeypatch, kind, fused, world)
        assert ca == cb, (kind, world, ca, cb)
        for k in ta:
            assert torch.equal(ta[k], tb[k]), (kind, 'world %d' % world, k, (ta[k].float() - tb[k].float()).abs().max().item())
        assert sa.keys() == sb.keys()
        for k in sa:
            assert sa[k] == sb[k], (kind, 'world %d' % world, k, sa[k], sb[k])


@pytest.mark.parametrize('kind', ['MPG-v1', 'MPG-v2', 'NADP', 'TD3', 'TD3-per', 'NDPG'])
def test_native_step_driver_in_a_mirrored_world(monkeypatch, engine, kind):
    """mpg_step_begin / mpg_step_end, learner versions 1 .. 5 (TD3 with uniform and with prioritized replay): train_step.cpp forms
    1 / (batch * world_size) once per version.  Worlds of 2 and 4 only: powers of two keep the argument exact."""
    check_mirrored_worlds(monkeypatch, kind, True)


@pytest.mark.parametrize('kind', ['MPG-v1', 'MPG-v2', 'NADP', 'TD3', 'TD3-per', 'NDPG', 'SAC'])
def test_method_path_in_a_mirrored_world(monkeypatch, engine, kind):
    """compute_gradient + apply_gradients of every learner (SAC has no native path): learners.py forms 1 / (rows * world) per
    learner and get_stats() divides by batch_size * world"""
    check_mirrored_worlds(monkeypatch, kind, False)
