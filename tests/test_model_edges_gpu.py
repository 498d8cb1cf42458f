"""The rollout sweeps at the models' clamp, wrap and large angles, both engines, against the float64 oracle.

Every other device test of the sweeps starts from the reset law (v_x in [15, 25], heading error N(0, pi / 9)) or within +-0.1 rad of
the upright pendulum, where PathTracking::finish() never clamps, pre() never wraps, vjp() never closes its gate and the pendulum's
sincosf / determinant / sin(theta)-weighted adjoint terms stay near one point.  The inputs here (tests/model_edge_inputs.py) reach
all of them; tests/test_model_edges.py asserts on the CPU that they do, that the float32 oracle stays 15 x inside every bar below and
that a sweep without the clamp, without the wrap or with an ungated adjoint misses the bars by 20 x or more.

Entry points and forms: mpg_rollout_pg in step-0 and all-steps mode, plain and with the packed weight image (all-steps + packed +
K = 0: the THIN reverse sweep), K = 0 and K = 3 (the WIDE forms), a ragged M = 2 launch at n = 31, in-kernel noise; mpg_ampc_pg;
mpg_rollout_q_estimation (M = 1, 2) and mpg_rollout_q_target; the fused path of mpg_mpg_gradients; the pendulum sweeps.

Bars (tests/test_slices_gpu.py): every gradient array <= 5e-5 relative L2 against float64, an exactly-zero reference array exactly
zero, ret_sum / rows rtol 5e-5 atol 1e-6, ret_sqsum rtol 2e-4 atol 1e-6; the rollouts without a gradient under
tests/yardstick.check_values; y_out and the critic losses of mpg_mpg_gradients under the bars of
tests/test_slices_gpu.test_mpg_gradients_with_one_and_three_slices.

Measured on the MI355X (worst gradient array / mean returns / squared returns, relative; split engine | exact-fp32 engine):
  pt-rows48-M1-n25-sel0_5_25-K0-step0-plain          3.1e-07 / 1.2e-07 / 3.1e-07 | 1.5e-07 / 5.6e-07 / 1.3e-07
  pt-rows48-M1-n25-sel0_5_25-K0-step0-packed         3.1e-07 / 1.2e-07 / 3.1e-07 | 1.5e-07 / 5.6e-07 / 1.3e-07
  pt-rows48-M1-n25-sel0_5_25-K0-all-plain            2.3e-07 / 1.2e-07 / 3.1e-07 | 2.3e-07 / 5.6e-07 / 1.3e-07
  pt-rows48-M1-n25-sel0_5_25-K0-all-packed           2.4e-07 / 1.2e-07 / 3.1e-07 | 2.4e-07 / 5.6e-07 / 1.3e-07
  pt-rows48-M1-n25-sel0_5_25-K3-step0-plain          8.6e-07 / 2.7e-07 / 1.5e-07 | 6.4e-07 / 2.7e-07 / 2.4e-07
  pt-rows48-M1-n25-sel0_5_25-K3-step0-packed         8.6e-07 / 2.7e-07 / 1.5e-07 | 6.4e-07 / 2.7e-07 / 2.4e-07
  pt-rows48-M1-n25-sel0_5_25-K3-all-plain            9.7e-07 / 2.7e-07 / 1.5e-07 | 7.1e-07 / 2.7e-07 / 2.4e-07
  pt-rows48-M1-n25-sel0_5_25-K3-all-packed           9.7e-07 / 2.7e-07 / 1.5e-07 | 7.1e-07 / 2.7e-07 / 2.4e-07
  pt-rows33-M2-n31-sel0_16_31-K0-step0-plain         4.0e-07 / 9.7e-08 / 1.3e-07 | 3.6e-07 / 4.4e-07 / 1.0e-07
  pt-rows48-M1-n25-sel0_5_25-K0-step0-plain-philox   2.4e-07 / 2.9e-07 / 4.5e-07 | 4.3e-07 / 5.6e-07 / 1.3e-07
  pd-rows48-M1-n25-sel0_5_25-K0-step0-plain          1.8e-06 / 2.7e-07 / 1.0e-07 | 1.7e-06 / 5.1e-07 / 8.8e-08
  pd-rows48-M1-n25-sel0_5_25-K0-step0-packed         1.8e-06 / 2.7e-07 / 1.0e-07 | 1.7e-06 / 5.1e-07 / 8.8e-08
  pd-rows48-M1-n25-sel0_5_25-K0-all-plain            4.1e-07 / 2.7e-07 / 1.0e-07 | 1.6e-07 / 5.1e-07 / 8.8e-08
  pd-rows48-M1-n25-sel0_5_25-K0-all-packed           5.0e-07 / 2.7e-07 / 1.0e-07 | 1.7e-07 / 5.1e-07 / 8.8e-08
  ampc plain                                         3.4e-07 / 7.7e-09 / 1.0e-07 | 2.8e-07 / 7.7e-09 / 1.7e-07
  ampc packed                                        4.5e-07 / 7.7e-09 / 1.0e-07 | 4.5e-07 / 7.7e-09 / 1.7e-07
  q estimation M=1                                   2.8e-07 (float32 oracle: 3.3e-07) | 3.0e-07 (float32 oracle: 3.3e-07)
  q estimation M=2                                   2.7e-07 (float32 oracle: 2.3e-07) | 2.9e-07 (float32 oracle: 2.3e-07)
  q target M=1                                       2.8e-07 (float32 oracle: 3.2e-07) | 2.7e-07 (float32 oracle: 3.2e-07)
  mpg_gradients                                      1.1e-06 / 1.2e-07 / 1.1e-07 | 5.2e-07 / 4.5e-07 / 1.7e-07
(q rows: relative L2 against float64, the float32 oracle's own beside it.)  The worst of all: 1.8e-6 of 5e-5, the pendulum's step-0 case."""

import numpy as np
import pytest
import torch

from tests import model_edge_inputs as E
from tests import yardstick as Y
from tests.test_sac_gpu import engine  # noqa: F401  (the fixture: both builds of the library)
from tests.test_slices_gpu import assert_thin_ran, check_arrays, check_case, dev, device_cfg, packed_run, rel_l2

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('case', E.PG_CASES, ids=E.pg_id)
def test_rollout_pg_at_the_models_edges(engine, case):
    """mpg_rollout_pg against float64 autograd.  The packed cases register the policy's weight image; the one that reaches the THIN
    reverse sweep (all-steps, no look-ahead entries) also runs plain, for assert_thin_ran."""
    from mpg_amd import ops
    env, rows, M, n, select, K, all_steps, packed, philox = case
    ocfg, wp, wq, obs, eps = E.pg_inputs(case)
    din, dout = ocfg.obs_dim, 2 * ocfg.act_dim
    ref = E.pg_reference(env, rows, M, n, select, K, all_steps, philox)
    w = E.weights(select)
    tag = '%s (%s)' % (E.pg_id(case), engine)

    def call(cfg, pol, q1):
        if philox:          # eps = NULL: the sweeps draw what O.model_noise_philox restates (tests/test_noise_gpu.py)
            return ops.rollout_pg(cfg, pol, q1, dev(obs), None, list(select), w, M=M, all_steps_param_grad=all_steps, n=n,
                                  noise_seed=E.PHILOX[0], noise_ctr=E.PHILOX[1])
        return ops.rollout_pg(cfg, pol, q1, dev(obs), dev(eps), list(select), w, M=M, all_steps_param_grad=all_steps)
    if not packed:
        check_case([x.clone() for x in call(device_cfg(ocfg), dev(wp), dev(wq))], ref, rows, din, dout, tag)
        return
    cached = packed_run(lambda: device_cfg(ocfg), wp, wq, din, dout, call)
    check_case(cached, ref, rows, din, dout, tag)
    if all_steps and K == 0:
        plain = [x.clone() for x in call(device_cfg(ocfg), dev(wp), dev(wq))]
        assert_thin_ran(plain[2], cached[2], din, tag)


def test_ampc_pg_at_the_models_edges(engine):
    """mpg_ampc_pg (every step through the policy, no critic, no discount) against tests/ampc_oracle.py in float64: the base sweeps
    and, with the packed image, the THIN reverse sweep"""
    from mpg_amd import ops
    ocfg, wp, wq, obs, eps = E.inputs(*E.BASE, E.seed_of(*E.BASE))
    rows = obs.shape[0]
    g64, rsum = E.ampc_reference()
    outs = {}
    for form in ('plain', 'packed'):
        cfg, pol = device_cfg(ocfg), dev(wp)
        if form == 'packed':
            wc = ops.WeightCache(pol, [(6, 4)])
            cfg.wcache[0] = wc.pointer
        rs, rq, grad = [x.clone() for x in ops.ampc_pg(cfg, pol, dev(obs), dev(eps), M=1, n=ocfg.n)]
        torch.cuda.synchronize()
        outs[form] = grad
        tag = 'ampc %s (%s)' % (form, engine)
        rs, rq = float(rs), float(rq)
        print('   %s: ret_sum / rows rel %.2e  ret_sqsum rel %.2e' % (tag, abs(rs / rsum.sum() - 1), abs(rq / (rsum ** 2).sum() - 1)))
        np.testing.assert_allclose(rs / rows, rsum.mean(), rtol=5e-5, atol=1e-6)
        np.testing.assert_allclose(rq, (rsum ** 2).sum(), rtol=2e-4, atol=1e-6)
        check_arrays(grad.cpu().numpy(), g64, 6, 4, 5e-5, tag)
    assert_thin_ran(outs['plain'], outs['packed'], 6, 'ampc (%s)' % engine)


@pytest.mark.parametrize('kind,M', E.Q_CASES)
def test_q_rollouts_at_the_models_edges(engine, kind, M):
    """mpg_rollout_q_estimation / mpg_rollout_q_target from the edge rows with first actions U(-1.2, 1.2), against
    O.model_rollout_for_q_estimation (select = [n]: the n-step target) under the rule of tests/yardstick.py"""
    from mpg_amd import ops
    ocfg, wp, wq, obs, act, eps = E.q_inputs(M)
    cfg = device_cfg(ocfg)
    if kind == 'estimation':
        y = ops.rollout_q_estimation(cfg, dev(wp), dev(wq), dev(obs), dev(act), dev(eps), list(E.Q_SELECT), M=M)
    else:
        y = ops.rollout_q_target(cfg, dev(wp), dev(wq), dev(obs), dev(act), dev(eps))
    y = y.cpu().numpy()
    r32, r64 = E.q_reference(kind, M, torch.float32), E.q_reference(kind, M)
    print('   q %s M=%d (%s): vs float64 %.2e  float32 oracle %.2e  vs the float32 oracle %.2e' % (
        kind, M, engine, rel_l2(y, r64), rel_l2(r32, r64), rel_l2(y, r32)))
    Y.check_values(y, r32, r64, what='q %s M=%d' % (kind, M))


def test_mpg_gradients_fused_path_at_the_models_edges(engine):
    """mpg_mpg_gradients, 48 rows, M = 1, two critics, slices (0, 25): the fused path, with the edge rows as batch observations.
    Checked as tests/test_slices_gpu.test_mpg_gradients_with_one_and_three_slices checks it: the complete gradient per array, y_out,
    the critic losses and the slice statistics."""
    from mpg_amd import ops
    w, obs, act, rew, obs2, eps = E.mg_inputs()
    ref_grad, st, red, m2, ws = E.mg_reference()
    rows, ns, names = obs.shape[0], len(E.MG_SELECT), ['Q1', 'Q2', 'policy']
    cfg = ops.make_cfg()
    assert rows % 16 == 0 and ops.mpg_gradients_supported(cfg, rows, 1, 25, ns, 2)        # (rows % 16 == 0 and M == 1: fused)
    params = dev(np.concatenate([w[nm] for nm in names]))
    targets = dev(np.concatenate([(w[nm] * np.float32(0.97)).astype(np.float32) for nm in names]))
    grad, stats, y_out = torch.zeros(params.numel(), device=DEV), torch.zeros(16, device=DEV), torch.zeros(rows, device=DEV)
    ops.mpg_gradients(cfg, 2, params, targets, dev(obs), dev(act), dev(rew), dev(obs2), None, list(E.MG_SELECT), ws, grad, stats, y_out,
                      eps=dev(eps))
    got, stats = grad.cpu().numpy(), stats.cpu().numpy()
    q_losses = np.array([st['q_loss1'], st['q_loss2']], np.float64)
    tag = 'mpg_gradients (%s)' % engine
    print('   %s: losses %s vs %s; ret_sum / rows rel %.2e  ret_sqsum rel %.2e' % (
        tag, stats[:2], q_losses, np.abs(stats[2:2 + ns] / rows / red - 1).max(), np.abs(stats[2 + ns:2 + 2 * ns] / m2 - 1).max()))
    np.testing.assert_allclose(y_out.cpu().numpy(), st['targets'], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(stats[:2], q_losses, rtol=5e-5, atol=1e-6)
    np.testing.assert_allclose(stats[2:2 + ns] / rows, red, rtol=5e-5, atol=1e-6)
    np.testing.assert_allclose(stats[2 + ns:2 + 2 * ns], m2, rtol=2e-4, atol=1e-6)
    o = 0
    for nm in names:
        din, dout = (6, 4) if nm == 'policy' else (8, 1)
        size = ops.net_size(din, dout)
        check_arrays(got[o:o + size], ref_grad[o:o + size], din, dout, 5e-5, tag + ' ' + nm)
        o += size
    assert o == got.size == ref_grad.size
