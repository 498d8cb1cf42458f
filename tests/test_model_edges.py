"""The conditions that make tests/test_model_edges_gpu.py worth running, by the oracle alone (CPU).  For every PathTracking case of
that file, on the float64 trajectory of its inputs (tests/model_edge_inputs.py):

  * at least 5 clamped (trajectory, step) pairs at each end of [1, 35], at least 3 wraps of the heading error in each direction, at
    least 2 trajectories that enter the clamp and are out of it again at the last step (the gate of the adjoint closes AND opens);
  * no raw v_x within 1e-3 of 1 or 35 and no raw heading error within 1e-3 of +-pi: a float32 trajectory is about 1e-5 from the
    float64 one on these quantities, so the device falls on the same side of every threshold (the float32 oracle is checked too);
  * the float32 oracle is within 1 / 15 of every bar of the device test from the float64 one (the margin tests/test_slices_gpu.py
    states for itself): the bars test the kernel and not the arithmetic;
  * three wrong models - no clamp, no wrap, the clamp with an ungated adjoint - each move EVERY gradient array by at least 20 x its
    bar, and the first two move the mean returns behind slice 0 (the Q estimates of the rollouts without a gradient) by at least
    20 x theirs.

For the pendulum cases: |theta| > 2 with cos(theta) < 0 in at least a quarter of the (trajectory, step) pairs, and the same
float32-against-float64 condition.  Every figure is printed (the condition table) before anything is asserted."""
import numpy as np
import pytest
import torch

from oracle import mpg_oracle as O
from tests import model_edge_inputs as E
from tests import yardstick as Y

GRAD_BAR, RET_BAR, SQ_BAR, VALUE_BAR = 5e-5, (5e-5, 1e-6), (2e-4, 1e-6), 1e-4      # the bars of tests/test_model_edges_gpu.py
MARGIN, BITE = 15., 20.


def over_bar(got, ref, bar):
    """the largest |got - ref| / (atol + rtol |ref|) of np.testing.assert_allclose: <= 1 passes"""
    rtol, atol = bar
    got, ref = np.atleast_1d(got).astype(np.float64), np.atleast_1d(ref).astype(np.float64)
    return float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max())


def array_moves(a, b):
    return [Y.rel_l2(x, y) for x, y in zip(a, b)]


def path_tracking_conditions(tag, run, gradient, model_outputs):
    """run(dtype, variant, log) -> (list of arrays under the relative-L2 bar, {name: (values, (rtol, atol))} under allclose bars).
    gradient: the arrays are a gradient (bar 5e-5, the ungated-adjoint variant applies); otherwise values under the yardstick's 1e-4.
    model_outputs: the names in the dict that depend on the model."""
    log64, log32 = [], []
    base, vals = run(torch.float64, None, log64)
    b32, v32 = run(torch.float32, None, log32)
    c = E.branch_counts(log64)
    bar = GRAD_BAR if gradient else VALUE_BAR
    own = max(array_moves(b32, base))
    own_vals = {k: over_bar(v32[k][0], vals[k][0], vals[k][1]) for k in vals}
    print('%s\n   clamped hi / lo %d / %d   wraps down / up %d / %d   leave the clamp again %d   nearest raw value to a threshold: v_x %.1e '
          'heading %.1e   largest |raw heading| %.3f' % (tag, c['clamp_hi'], c['clamp_lo'], c['wrap_down'], c['wrap_up'], c['leave'],
                                                         c['near_vx'], c['near_dphi'], c['max_abs_dphi']))
    print('   float32 oracle vs float64: worst array %.1e (bar / 15 = %.1e)   %s' % (
        own, bar / MARGIN, '  '.join('%s %.3f of its bar' % (k, v) for k, v in own_vals.items())))
    moved = {}
    for variant in E.VARIANTS if gradient else E.VARIANTS[:2]:
        g, v = run(torch.float64, variant, None)
        mv = array_moves(g, base)
        mo = {k: over_bar(v[k][0], vals[k][0], vals[k][1]) for k in model_outputs}
        moved[variant] = (min(mv), mo)
        print('   %-16s moves the arrays by %.1e ... %.1e%s' % (variant, min(mv), max(mv), ''.join('   %s by %.0f x its bar' % kv for kv in mo.items())))
    assert c['clamp_hi'] >= 5 and c['clamp_lo'] >= 5, (tag, c)
    assert c['wrap_down'] >= 3 and c['wrap_up'] >= 3, (tag, c)
    assert c['leave'] >= 2, (tag, c)
    assert c['near_vx'] >= 1e-3 and c['near_dphi'] >= 1e-3, (tag, c)
    for (a64, d64), (a32, d32) in zip(log64, log32):         # the float32 trajectory takes every branch as the float64 one
        assert np.array_equal(a64 > 35., a32 > 35.) and np.array_equal(a64 < 1., a32 < 1.), tag
        assert np.array_equal(d64 > np.pi, d32 > np.pi) and np.array_equal(d64 <= -np.pi, d32 <= -np.pi), tag
    assert own <= bar / MARGIN, (tag, own)
    assert max(own_vals.values(), default=0.) <= 1. / MARGIN, (tag, own_vals)
    for variant, (least, mo) in moved.items():
        assert least >= BITE * bar, (tag, variant, least)
        if variant != 'ungated adjoint':
            assert all(x >= BITE for x in mo.values()), (tag, variant, mo)
    return c


def distinct(cases):
    """the cases without the weight-image form: the oracle does not know it"""
    out = []
    for c in cases:
        c = c[:7] + (False,) + c[8:]
        if c not in out:
            out.append(c)
    return out


@pytest.mark.parametrize('case', distinct([c for c in E.PG_CASES if c[0] == E.PT]), ids=E.pg_id)
def test_rollout_pg_cases_reach_every_branch(case):
    env, rows, M, n, select, K, all_steps, _, philox = case
    ocfg, wp, wq, obs, eps = E.pg_inputs(case)
    assert np.abs(obs[:, 4]).max() > 3.3           # a start observation outside the principal range
    w = E.weights(select)
    later = [i for i, k in enumerate(select) if k > 0]

    def run(dtype, variant, log):
        g, red, m2 = E.pg_arrays(ocfg, wp, wq, obs, eps, select, w, all_steps, dtype, variant, log)
        return g, {'returns': (red[later], RET_BAR), 'squares': (m2[later], SQ_BAR), 'return 0': (red[:1], RET_BAR)}
    path_tracking_conditions(E.pg_id(case), run, True, ('returns',))


def test_ampc_case_reaches_every_branch():
    ocfg, wp, wq, obs, eps = E.inputs(*E.BASE, E.seed_of(*E.BASE))

    def run(dtype, variant, log):
        g, rsum = E.ampc_arrays(ocfg, wp, obs, eps, dtype, variant, log)
        return g, {'ret_sum': (rsum.sum(), (RET_BAR[0], 0.)), 'ret_sqsum': ((rsum ** 2).sum(), (SQ_BAR[0], 0.))}
    path_tracking_conditions('ampc', run, True, ('ret_sum',))


@pytest.mark.parametrize('kind,M', E.Q_CASES)
def test_q_rollout_cases_reach_every_branch(kind, M):
    """first actions U(-1.2, 1.2): another first step than the policy's, so another trajectory - its own conditions"""
    ocfg, wp, wq, obs, act, eps = E.q_inputs(M)
    select = E.Q_SELECT if kind == 'estimation' else (ocfg.n,)
    rows = obs.shape[0]

    def run(dtype, variant, log):
        y = E.q_values(ocfg, wp, wq, obs, act, eps, select, M, dtype, variant, log)
        return [y[i * rows:(i + 1) * rows] for i, k in enumerate(select) if k > 0], {}
    path_tracking_conditions('q %s M=%d' % (kind, M), run, False, ())


def test_mpg_gradients_case_reaches_every_branch():
    """the policy part of mpg_mpg_gradients: slices (0, 25) under the rule-based weights of iteration MG_ITERATION (the critics'
    gradients do not see the model)"""
    ocfg, wp, wq, obs, eps = E.inputs(*E.BASE, E.seed_of(*E.BASE))
    mcfg = O.Cfg(select=list(E.MG_SELECT))
    ws = O.rule_based_weights(E.MG_ITERATION, mcfg.total_ite, mcfg.eta, mcfg.select).numpy()
    assert ws.min() > 0.2 / len(E.MG_SELECT)

    def run(dtype, variant, log):
        g, red, m2 = E.pg_arrays(ocfg, wp, wq, obs, eps, E.MG_SELECT, ws, E.STEP0, dtype, variant, log)
        return g, {'returns': (red[1:], RET_BAR), 'squares': (m2[1:], SQ_BAR)}
    path_tracking_conditions('mpg_gradients', run, True, ('returns',))


@pytest.mark.parametrize('case', distinct([c for c in E.PG_CASES if c[0] == E.PD]), ids=E.pg_id)
def test_pendulum_cases_cover_the_circle(case):
    env, rows, M, n, select, K, all_steps, _, philox = case
    ocfg, wp, wq, obs, eps = E.pg_inputs(case)
    w = E.weights(select)
    log = []
    g64, red64, sq64 = E.pg_arrays(ocfg, wp, wq, obs, eps, select, w, all_steps, torch.float64, None, log)
    g32, red32, sq32 = E.pg_arrays(ocfg, wp, wq, obs, eps, select, w, all_steps, torch.float32)
    th = np.stack(log)
    far = float(((np.abs(th) > 2.) & (np.cos(th) < 0.)).mean())
    own = max(array_moves(g32, g64))
    print('%s\n   |theta| > 2 and cos(theta) < 0 in %.2f of the (trajectory, step) pairs, largest |theta| %.2f\n   float32 oracle vs float64: '
          'worst array %.1e (bar / 15 = %.1e)   returns %.3f of their bar   squares %.3f' % (
              E.pg_id(case), far, np.abs(th).max(), own, GRAD_BAR / MARGIN, over_bar(red32, red64, RET_BAR), over_bar(sq32, sq64, SQ_BAR)))
    assert far >= 0.25, far
    assert own <= GRAD_BAR / MARGIN, own
    assert over_bar(red32, red64, RET_BAR) <= 1. / MARGIN and over_bar(sq32, sq64, SQ_BAR) <= 1. / MARGIN
