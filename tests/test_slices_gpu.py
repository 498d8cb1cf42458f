"""mpg_rollout_pg and mpg_mpg_gradients at slice lists and horizons other than [0, 25] against the float64 oracle: intermediate
slices in the forward sweep (XQ / GK of a middle slice) and in the reverse sweep (GXQ injected into the chain at 0 < t < n, rho[t]
with several slices behind step t), n > max(select), unsorted lists, MAXSEL slices, horizons 1, 2 and MAXN - 1, the packed-image
(THIN) reverse sweep, gamma / rew_shift other than the defaults.

Bars (tests/test_rollout_gpu.py): every gradient array <= 5e-5 relative L2 against float64 (an exactly-zero reference array: exactly
zero), ret_sum / rows rtol 5e-5 atol 1e-6, ret_sqsum rtol 2e-4 atol 1e-6.  The oracle's own float32 run is at most 2.9e-6 (gradients)
and 8.5e-7 (returns) from its float64 run on every case here, so the bar sits more than 15 x above the reference arithmetic's own
error.  Slice weights np.linspace(0.2, 0.5, n_select): comparable sizes, every slice matters (see the condition test)."""
import functools

import numpy as np
import pytest
import torch

from oracle import mpg_oracle as O
from tests import dp_oracle as DP
from tests import yardstick as Y

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PD = 'InvertedPendulumConti-v0'
H = 256


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).to(DEV)


def weights(select):
    return np.linspace(0.2, 0.5, len(select)).astype(np.float32)


def check_arrays(got, ref, din, dout, tol, tag=''):
    """per array: relative L2 <= tol; an exactly-zero reference array must be exactly zero.  Prints every figure first."""
    o, rows = 0, []
    for shp in O.mlp_shapes(din, H, dout):
        n = int(np.prod(shp))
        r, g = ref[o:o + n], got[o:o + n]
        rows.append((shp, None if np.linalg.norm(r) == 0 else rel_l2(g, r), float(np.abs(g).max())))
        o += n
    assert o == got.size == ref.size, (o, got.size, ref.size)
    print('   %s: %s' % (tag, '  '.join('%s %s' % (shp, 'zero' if e is None else '%.2e' % e) for shp, e, _ in rows)))
    for shp, e, mx in rows:
        if e is None:
            assert mx == 0.0, (tag, shp, 'the reference array is exactly zero')
        else:
            assert e <= tol, (tag, shp, e)


# ---- inputs and the float64 reference, computed once per case --------------------------------------------------------------
def seed_of(rows, n, select, K):
    return 5 if (rows, n, tuple(select), K) == (48, 25, (0, 5, 25), 0) else rows * 7 + n


@functools.lru_cache(maxsize=None)
def inputs(env, rows, M, n, K, seed, gamma=0.98, rew_shift=0.0):
    """(ocfg, policy weights, Q1 weights, start observations, eps [n][rows * M]); draw order: policy, Q1, obs, eps"""
    rng = np.random.Generator(np.random.PCG64(seed))
    from tests.golden_inputs import mlp_weights_flat, reset_law_obs
    if env == 'pt':
        ocfg = O.Cfg(M=M, n=n, obs_dim=6 + K, obs_scale=list(O.OBS_SCALE_PT) + [1.] * K, gamma=gamma, rew_shift=rew_shift)
        wp, wq = mlp_weights_flat(rng, 6 + K, 4), mlp_weights_flat(rng, 8 + K, 1)
        obs = reset_law_obs(rng, rows)
        if K:       # look-ahead entries of a start observation: near delta_y, not equal to it
            obs = np.concatenate([obs, obs[:, 3:4] + 0.3 * rng.standard_normal((rows, K)).astype(np.float32)], 1).astype(np.float32)
    else:
        ocfg = O.Cfg(env=PD, M=M, n=n, gamma=gamma, rew_shift=rew_shift)
        wp, wq = mlp_weights_flat(rng, 4, 2), mlp_weights_flat(rng, 5, 1)
        obs = rng.uniform(-0.1, 0.1, (rows, 4)).astype(np.float32)
    eps = rng.standard_normal((n, rows * M)).astype(np.float32)
    return ocfg, wp, wq, obs, eps


def device_cfg(ocfg):
    from mpg_amd import ops
    if ocfg.env == PD:
        return ops.make_cfg(PD, gamma=ocfg.gamma, rew_shift=ocfg.rew_shift)
    return ops.make_cfg(obs_dim=ocfg.obs_dim, obs_scale=ocfg.obs_scale, gamma=ocfg.gamma, rew_shift=ocfg.rew_shift)


def oracle_arrays(ocfg, wp, wq, obs, eps, select, w, all_steps, dtype=torch.float64):
    """gradient arrays of -sum_k w_k * reduced[select_k], the selected mean returns, the selected sums of squared returns"""
    nets = O.Nets(ocfg, {'policy': wp, 'Q1': wq}, dtype=dtype)
    reduced, _, allret = O.model_rollout_for_policy_update(ocfg, nets, torch.as_tensor(obs).to(dtype), torch.as_tensor(eps).to(dtype),
                                                           rollout_policy='policy' if all_steps else 'policy_rollout')
    loss = -sum(float(wk) * reduced[k] for wk, k in zip(w, select))
    grads = [x.numpy().astype(np.float64) for x in torch.autograd.grad(loss, nets.w['policy'])]
    sel = list(select)
    return grads, reduced[sel].detach().numpy(), (allret[sel] ** 2).sum(1).detach().numpy()


@functools.lru_cache(maxsize=None)
def reference(env, rows, M, n, select, K, all_steps, gamma=0.98, rew_shift=0.0):
    ocfg, wp, wq, obs, eps = inputs(env, rows, M, n, K, seed_of(rows, n, select, K), gamma, rew_shift)
    grads, red, m2 = oracle_arrays(ocfg, wp, wq, obs, eps, select, weights(select), all_steps)
    return np.concatenate([g.ravel() for g in grads]), red, m2


def check_case(out, ref, rows, din, dout, tag):
    ret_sum, ret_sq, grad = [x.cpu().numpy() for x in out]
    g64, red, m2 = ref
    print('   %s: ret_sum / rows rel %.2e  ret_sqsum rel %.2e' % (tag, np.abs(ret_sum / rows / red - 1).max(), np.abs(ret_sq / m2 - 1).max()))
    np.testing.assert_allclose(ret_sum / rows, red, rtol=5e-5, atol=1e-6)
    np.testing.assert_allclose(ret_sq, m2, rtol=2e-4, atol=1e-6)
    check_arrays(grad, g64, din, dout, 5e-5, tag)


def packed_run(cfg_of, wp, wq, din, dout, call):
    """the same launch with the policy's packed image registered: the networks are views of one flat [Q1 | policy] vector
    (test_weight_cache_is_bit_identical_to_the_strided_path), its WeightCache hangs in the cfg for the call"""
    from mpg_amd import ops
    flat = dev(np.concatenate([wq, wp]))
    cfg = cfg_of()
    wc = ops.WeightCache(flat, [(din + dout // 2, 1), (din, dout)])
    cfg.wcache[0] = wc.pointer
    out = [x.clone() for x in call(cfg, flat[wq.size:], flat[:wq.size])]
    torch.cuda.synchronize()
    del wc
    return out


def assert_thin_ran(plain_grad, cached_grad, din, tag):
    """Stands for "the cached launch took the THIN reverse sweep": the packed image alone changes no bit of any result
    (test_weight_cache_is_bit_identical_to_the_strided_path), while THIN accumulates the first layer's gradient (dW1, db1) inside
    the sweep, step by step per workgroup, instead of in the weight-gradient launch - another summation order, other last bits.
    Bit-equal first-layer arrays therefore mean that mpg_rollout_pg dropped the thin partials and ran the plain sweep."""
    first = din * H + H
    assert not torch.equal(plain_grad[:first], cached_grad[:first]), (tag, 'the cached launch did not reach the THIN reverse sweep')


PT, STEP0, ALL = 'pt', False, True
CASES = [                                                   # (env, rows, M, n, select, look-ahead K, all-steps mode)
    (PT, 48, 1, 25, (0, 5, 25), 0, STEP0), (PT, 48, 1, 25, (0, 5, 25), 0, ALL),
    (PT, 50, 1, 25, (0, 1, 24, 25), 0, STEP0),              # adjacent slices, MAXSEL, ragged rows
    (PT, 48, 1, 25, (25, 0, 5), 0, STEP0),                  # unsorted
    (PT, 33, 2, 25, (3, 17), 0, STEP0),                     # n > max(select), M = 2, ragged
    (PT, 48, 1, 25, (10,), 0, STEP0),                       # a single middle slice
    (PT, 48, 1, 1, (0, 1), 0, STEP0), (PT, 48, 1, 1, (0, 1), 0, ALL), (PT, 17, 1, 1, (1,), 0, STEP0),
    (PT, 48, 1, 2, (0, 1, 2), 0, STEP0), (PT, 48, 1, 2, (0, 1, 2), 0, ALL),
    (PT, 48, 1, 31, (0, 16, 31), 0, STEP0), (PT, 48, 1, 31, (0, 16, 31), 0, ALL), (PT, 33, 1, 31, (31,), 0, STEP0),
    (PT, 48, 1, 31, (7, 31), 0, ALL), (PT, 48, 1, 30, (0, 10, 20, 30), 0, STEP0),
    (PT, 48, 1, 25, (0, 5, 25), 3, STEP0), (PT, 48, 1, 25, (0, 5, 25), 3, ALL),
    (PT, 17, 1, 25, (2, 25), 10, STEP0), (PT, 32, 2, 25, (0, 5, 25), 10, ALL),
    ('pd', 48, 1, 25, (0, 5, 25), 0, ALL), ('pd', 50, 1, 12, (4, 12), 0, STEP0), ('pd', 48, 1, 1, (1,), 0, ALL),
]


def case_id(c):
    return '%s-rows%d-M%d-n%d-sel%s-K%d-%s' % (c[0], c[1], c[2], c[3], '_'.join(str(k) for k in c[4]), c[5], 'all' if c[6] else 'step0')


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_rollout_pg_slices_vs_oracle(case):
    """Every all-steps case without look-ahead entries runs twice: with a plain cfg, and with the policy's packed image registered,
    which is what sends the launch to the THIN reverse sweep (see assert_thin_ran for what the bit-inequality stands for).  Both
    runs go against the oracle."""
    from mpg_amd import ops
    env, rows, M, n, select, K, all_steps = case
    ocfg, wp, wq, obs, eps = inputs(env, rows, M, n, K, seed_of(rows, n, select, K))
    din, dout = ocfg.obs_dim, 2 * ocfg.act_dim
    ref = reference(*case)
    w = weights(select)

    def call(cfg, pol, q1):
        return ops.rollout_pg(cfg, pol, q1, dev(obs), dev(eps), list(select), w, M=M, all_steps_param_grad=all_steps)
    plain = [x.clone() for x in call(device_cfg(ocfg), dev(wp), dev(wq))]
    check_case(plain, ref, rows, din, dout, case_id(case))
    if all_steps and K == 0:
        cached = packed_run(lambda: device_cfg(ocfg), wp, wq, din, dout, call)
        check_case(cached, ref, rows, din, dout, case_id(case) + ' packed')
        assert_thin_ran(plain[2], cached[2], din, case_id(case))


def test_unsorted_list_equals_the_sorted_one():
    """select = [25, 0, 5] against [0, 5, 25] with the weights permuted alike: the same loss, so the statistics are the sorted
    launch's after reordering and the gradient meets the bar (the unsorted launch against the oracle: the case list above)."""
    from mpg_amd import ops
    ocfg, wp, wq, obs, eps = inputs(PT, 48, 1, 25, 0, seed_of(48, 25, (25, 0, 5), 0))
    w = weights((25, 0, 5))
    cfg = device_cfg(ocfg)
    a = [x.clone() for x in ops.rollout_pg(cfg, dev(wp), dev(wq), dev(obs), dev(eps), [25, 0, 5], w)]
    b = [x.clone() for x in ops.rollout_pg(cfg, dev(wp), dev(wq), dev(obs), dev(eps), [0, 5, 25], w[[1, 2, 0]])]
    order = [2, 0, 1]                       # slices (25, 0, 5) inside the sorted launch's outputs
    print('   unsorted vs sorted: gradient rel L2 %.2e' % rel_l2(a[2].cpu().numpy(), b[2].cpu().numpy()))
    assert torch.equal(a[0], b[0][order]) and torch.equal(a[1], b[1][order])
    check_arrays(a[2].cpu().numpy(), b[2].cpu().numpy().astype(np.float64), 6, 4, 5e-5, 'unsorted vs sorted')


@pytest.mark.parametrize('all_steps', [STEP0, ALL], ids=['step0', 'all'])
def test_every_slice_of_0_5_25_matters_to_every_array(all_steps):
    """Condition on the inputs of the [0, 5, 25] case, by the oracle alone: dropping any one slice, or moving slice 5 to 4 or to
    6, moves EVERY gradient array by at least 1e-2 relative (measured: at least 4.2e-2 in step-0 mode, 5 -> 6; 1.6e-2 in all-steps
    mode, dropping slice 0).  So the 5e-5 bar of the case is a test of the slice logic and not of magnitudes."""
    ocfg, wp, wq, obs, eps = inputs(PT, 48, 1, 25, 0, seed_of(48, 25, (0, 5, 25), 0))
    w = weights((0, 5, 25))
    base = oracle_arrays(ocfg, wp, wq, obs, eps, (0, 5, 25), w, all_steps)[0]
    for name, sel, ws in (('drop 0', (5, 25), w[1:]), ('drop 5', (0, 25), w[[0, 2]]), ('drop 25', (0, 5), w[:2]),
                          ('5 -> 4', (0, 4, 25), w), ('5 -> 6', (0, 6, 25), w)):
        g = oracle_arrays(ocfg, wp, wq, obs, eps, sel, ws, all_steps)[0]
        moves = [rel_l2(a, b) for a, b in zip(g, base)]
        print('   %s: smallest move of any array %.2e' % (name, min(moves)))
        assert min(moves) >= 1e-2, (name, moves)


@pytest.fixture(params=['split', 'f32'])
def engine(request):
    """both builds of the library (mpg_amd/_lib.py ENGINES): the split-fp16 product and the exact-fp32 engine"""
    from mpg_amd import _lib as L
    with L.engine(request.param):
        yield request.param


def test_double_pendulum_three_slices(engine):
    """(50, 1, 10, [0, 4, 10]) on the double pendulum's sweeps (ENV::fold in the middle of the chain), step-0 mode, by the rule of
    DP.check_arrays; horizon 10 for the reason in test_double_pendulum_gpu.test_rows_not_a_multiple_of_16's docstring."""
    import os
    from mpg_amd import ops
    golden_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    inp, _ = DP.load_case(golden_dir, 256, 25)
    n, select = 10, [0, 4, 10]
    w = weights(select)
    obs = inp['batch_obs'][:50]
    cfg = ops.make_cfg(DP.ENV_ID)
    rs, _, grad = ops.rollout_pg(cfg, dev(inp['w_policy']), dev(inp['w_Q1']), dev(obs), None, select, w, n=n)
    ref = {}
    for dt in (torch.float32, torch.float64):
        ocfg = DP.make_cfg(n)
        nets = DP.nets_of(ocfg, inp, dt)
        red = DP.rollout_policy_update(ocfg, nets, torch.as_tensor(obs).to(dt), n, all_steps_param_grad=False)
        loss = -sum(float(wk) * red[k] for wk, k in zip(w, select))
        ref[dt] = (np.concatenate([x.numpy().ravel() for x in torch.autograd.grad(loss, nets.w['policy'])]),
                   red[select].detach().numpy() * 50)
    worst = DP.check_arrays(grad.cpu().numpy(), ref[torch.float32][0], ref[torch.float64][0], [('policy', 11, 2)], 256, engine + ' dp [0, 4, 10]')
    print('%s double pendulum [0, 4, 10]: worst error / allowance %.3f' % (engine, worst))
    Y.check_values(rs.cpu().numpy(), ref[torch.float32][1], ref[torch.float64][1], what='return sums')


def test_several_row_groups_per_workgroup_with_a_middle_slice():
    """4096 + 16 * 3 + 5 rows = 260 row groups on 256 workgroups, the last one ragged: a workgroup's second group must find
    the slice state (selmask, the injection steps) as its first did.  Against the oracle, and two launches bit-identical."""
    from mpg_amd import ops
    case = (PT, 4096 + 16 * 3 + 5, 1, 25, (0, 5, 25), 0, STEP0)
    env, rows, M, n, select, K, all_steps = case
    ocfg, wp, wq, obs, eps = inputs(env, rows, M, n, K, seed_of(rows, n, select, K))
    cfg = device_cfg(ocfg)
    runs = [[x.clone() for x in ops.rollout_pg(cfg, dev(wp), dev(wq), dev(obs), dev(eps), list(select), weights(select))] for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    check_case(runs[0], reference(*case), rows, 6, 4, case_id(case))


def test_gamma_and_reward_shift_other_than_the_defaults():
    """gamma = 0.9, rew_shift = 0.5 (cfg fields of every rollout kernel): mpg_rollout_pg at [0, 5, 25], then the same cfg through
    mpg_rollout_q_target (bar of test_q_estimation_rollout_vs_reference: 2e-5 relative L2) and mpg_q_targets (bar of
    test_policy_action_and_clipped_double_q_target_vs_golden: rtol 2e-5, atol 2e-6), each against the float64 oracle."""
    from mpg_amd import ops
    from tests.golden_inputs import mlp_weights_flat, reset_law_obs
    case = (PT, 48, 1, 25, (0, 5, 25), 0, STEP0, 0.9, 0.5)
    env, rows, M, n, select, K, all_steps, gamma, shift = case
    ocfg, wp, wq, obs, eps = inputs(env, rows, M, n, K, seed_of(rows, n, select, K), gamma, shift)      # the inputs of the default case
    cfg = device_cfg(ocfg)
    assert abs(cfg.gamma - 0.9) < 1e-7 and cfg.rew_shift == 0.5
    out = [x.clone() for x in ops.rollout_pg(cfg, dev(wp), dev(wq), dev(obs), dev(eps), list(select), weights(select))]
    grads, red, m2 = oracle_arrays(ocfg, wp, wq, obs, eps, select, weights(select), all_steps)
    check_case(out, (np.concatenate([g.ravel() for g in grads]), red, m2), rows, 6, 4, 'gamma 0.9 shift 0.5')
    # and the defaults give something else: the fields are really read
    base = reference(PT, 48, 1, 25, (0, 5, 25), 0, STEP0)
    assert rel_l2(red, base[1]) > 1e-2
    rng = np.random.Generator(np.random.PCG64(78))
    wq2 = mlp_weights_flat(rng, 8, 1)
    act = rng.uniform(-1, 1, (rows, 2)).astype(np.float32)
    rew, obs2 = rng.uniform(-30, 0, rows).astype(np.float32), reset_law_obs(rng, rows)
    nets = O.Nets(ocfg, {'policy': wp, 'Q1': wq, 'Q2': wq2}, target_scale=0.97, dtype=torch.float64)
    tgt = lambda f: (f * np.float32(0.97)).astype(np.float32)
    y = ops.rollout_q_target(cfg, dev(wp), dev(tgt(wq)), dev(obs), dev(act), dev(eps)).cpu().numpy()
    ref = O.model_rollout_for_q_estimation(ocfg, nets, torch.as_tensor(obs), torch.as_tensor(act), torch.as_tensor(eps), [n]).numpy()
    print('   rollout_q_target rel L2 %.2e' % rel_l2(y, ref))
    assert rel_l2(y, ref) <= 2e-5
    y = ops.q_targets(cfg, dev(tgt(wp)), dev(tgt(wq)), dev(tgt(wq2)), dev(rew), dev(obs2)).cpu().numpy()
    ref = O.clipped_double_q_target(ocfg, nets, torch.as_tensor(rew).double(), torch.as_tensor(obs2).double()).numpy()
    print('   q_targets max abs %.2e' % np.abs(y - ref).max())
    np.testing.assert_allclose(y, ref, rtol=2e-5, atol=2e-6)


def test_in_kernel_noise_with_three_slices():
    """(100, 1, 25, [0, 5, 25]) with eps = NULL equals the launch fed the oracle's Philox draws (tests/test_noise_gpu.py) to 1e-7"""
    from mpg_amd import ops
    ocfg, wp, wq, obs, _ = inputs(PT, 100, 1, 25, 0, seed_of(100, 25, (0, 5, 25), 0))
    cfg, w = device_cfg(ocfg), weights((0, 5, 25))
    seed, ctr = 4242, (3 << 32) + 17
    a = [x.clone() for x in ops.rollout_pg(cfg, dev(wp), dev(wq), dev(obs), None, [0, 5, 25], w, n=25, noise_seed=seed, noise_ctr=ctr)]
    eps = O.model_noise_philox(25, 100, seed, ctr)
    b = ops.rollout_pg(cfg, dev(wp), dev(wq), dev(obs), dev(eps), [0, 5, 25], w)
    e = [rel_l2(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(a, b)]
    print('   in-kernel noise vs oracle draws: returns %.1e squares %.1e gradient %.1e' % tuple(e))
    assert max(e) <= 1e-7, e


# ---- mpg_mpg_gradients with one and three slices ---------------------------------------------------------------------------
MG_ITERATION = 4500      # lam = 1: the rule gives every slice the same weight, so each one matters


@pytest.mark.parametrize('rows,n_q,select,given_y', [(64, 1, (25,), False), (64, 1, (0, 5, 25), False), (64, 2, (25,), False),
                                                     (64, 2, (0, 5, 25), False), (64, 2, (0, 5, 25), True), (50, 1, (25,), True),
                                                     (50, 1, (0, 5, 25), False), (50, 2, (25,), False), (50, 2, (0, 5, 25), False)])
def test_mpg_gradients_with_one_and_three_slices(rows, n_q, select, given_y):
    """n_select != 2 leaves the kernels built for two slices (k_critic_fused4, k_qslice_fused2, the split target) for
    launch_qloss_fused + k_qslice_fused, where a row's slice is gr / R; rows = 64 takes that fused path, rows = 50 the fine-grained
    fallback.  Reference: O.mpg_compute_gradient in float64 with cfg.select and a clip so large that nothing is scaled (two critics);
    with one critic, or targets handed in (y_in), the same oracle functions with those targets.  Checked: the complete gradient per
    array, y_out where the call computes it (bar of the q_targets golden test), the critic losses and the slice statistics."""
    from mpg_amd import ops
    from tests.golden_inputs import mlp_weights_flat, reset_law_obs
    rng = np.random.Generator(np.random.PCG64(rows + 10 * n_q + len(select)))
    names = ['Q1', 'policy'] if n_q == 1 else ['Q1', 'Q2', 'policy']
    w = {nm: mlp_weights_flat(rng, 6, 4) if nm == 'policy' else mlp_weights_flat(rng, 8, 1) for nm in names}
    obs, obs2 = reset_law_obs(rng, rows), reset_law_obs(rng, rows)
    act, rew = rng.uniform(-1, 1, (rows, 2)).astype(np.float32), rng.uniform(-30, 0, rows).astype(np.float32)
    eps = rng.standard_normal((25, rows)).astype(np.float32)
    y_given = (0.3 * rng.standard_normal(rows) - 0.5).astype(np.float32) if given_y else None
    ocfg = O.Cfg(select=list(select), clip=1e30)
    ws = O.rule_based_weights(MG_ITERATION, ocfg.total_ite, ocfg.eta, ocfg.select).numpy()        # float32, as the learners hand them over
    assert ws.min() > 0.2 / len(select)

    # ---- float64 reference ----
    dt = torch.float64
    nets = O.Nets(ocfg, w, target_scale=0.97, dtype=dt)
    t = lambda x: torch.as_tensor(x).to(dt)
    if n_q == 2 and not given_y:
        grads, st = O.mpg_compute_gradient(ocfg, nets, [obs, act, rew, obs2, None], eps, MG_ITERATION)
        np.testing.assert_allclose(st['w_list'], ws, rtol=1e-6)
        ref_grad, y_ref = np.concatenate([g.ravel() for g in grads]), st['targets']
        q_losses = [st['q_loss1'], st['q_loss2']]
    else:
        if given_y:
            y_ref = y_given.astype(np.float64)
        elif n_q == 2:
            y_ref = O.clipped_double_q_target(ocfg, nets, t(rew), t(obs2)).numpy()
        else:       # one critic: r~ + gamma * Q1_target(s', pi_target(s'))  (mpg_learner.py:126-134 without the second critic)
            with torch.no_grad():
                po1 = O.process_obses(ocfg, t(obs2))
                y_ref = (O.process_rewards(ocfg, t(rew)) + ocfg.gamma * nets.q('Q1_target', po1, nets.compute_target_action(po1))).numpy()
        q_losses, q_grads = O.q_forward_and_backward(ocfg, nets, t(obs), t(act), t(y_ref), names[:-1])
        reduced, _, _ = O.model_rollout_for_policy_update(ocfg, nets, t(obs), t(eps))
        pg = torch.autograd.grad(-sum(float(wk) * reduced[k] for wk, k in zip(ws, select)), nets.w['policy'])
        ref_grad = np.concatenate([g.numpy().ravel() for gl in q_grads for g in gl] + [g.numpy().ravel() for g in pg])
        q_losses = [l.numpy() for l in q_losses]
    with torch.no_grad():
        nets2 = O.Nets(ocfg, w, target_scale=0.97, dtype=dt)
        reduced, _, allret = O.model_rollout_for_policy_update(ocfg, nets2, t(obs), t(eps))
    red, m2 = reduced[list(select)].numpy(), (allret[list(select)] ** 2).sum(1).numpy()

    # ---- device ----
    cfg = ops.make_cfg()
    params = dev(np.concatenate([w[nm] for nm in names]))
    targets = dev(np.concatenate([(w[nm] * np.float32(0.97)).astype(np.float32) for nm in names]))
    grad, stats, y_out = torch.zeros(params.numel(), device=DEV), torch.zeros(16, device=DEV), torch.zeros(rows, device=DEV)
    ops.mpg_gradients(cfg, n_q, params, targets, dev(obs), dev(act), dev(rew), dev(obs2), dev(y_given) if given_y else None, list(select), ws,
                      grad, stats, y_out, eps=dev(eps))
    got, stats = grad.cpu().numpy(), stats.cpu().numpy()
    ns = len(select)
    tag = 'rows%d nq%d sel%s%s' % (rows, n_q, list(select), ' y_in' if given_y else '')
    print('   %s: losses %s vs %s; ret_sum / rows rel %.2e  ret_sqsum rel %.2e' % (
        tag, stats[:n_q], np.array(q_losses), np.abs(stats[2:2 + ns] / rows / red - 1).max(), np.abs(stats[2 + ns:2 + 2 * ns] / m2 - 1).max()))
    if not given_y:
        np.testing.assert_allclose(y_out.cpu().numpy(), y_ref, rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(stats[:n_q], np.array(q_losses, np.float64), rtol=5e-5, atol=1e-6)
    np.testing.assert_allclose(stats[2:2 + ns] / rows, red, rtol=5e-5, atol=1e-6)
    np.testing.assert_allclose(stats[2 + ns:2 + 2 * ns], m2, rtol=2e-4, atol=1e-6)
    o = 0
    for nm in names:
        din, dout = (6, 4) if nm == 'policy' else (8, 1)
        size = ops.net_size(din, dout)
        check_arrays(got[o:o + size], ref_grad[o:o + size], din, dout, 5e-5, tag + ' ' + nm)
        o += size
    assert o == got.size == ref_grad.size
