"""The conditions that make tests/test_env_edges_gpu.py worth running, by the oracle alone (CPU), on the float32 oracle's own 30-step
closed loop over the start rows of tests/env_edge_inputs.py, for K = 0 and K = 3 look-ahead entries:

  * the branches of step_agent are reached: sub-steps clamped at each end of [1, 35], x wrapped in both directions (also by agents
    that start inside the period: 'period' and 'backwards'), heading and delta_phi wrapped in both directions, path arguments beyond
    200 and below 0 at a last sub-step, agents that enter the clamp at 35 and leave it again;
  * done_intended is 0 and 1 often enough, and each of its four terms decides alone somewhere;
  * no (agent, step) pair sits within rounding of a threshold (near() is false everywhere): the device test may cap its exclusions;
  * the float32 oracle is inside every bar of bars() from its float64 restatement, one step from the same state: the bars test the
    kernel and not the arithmetic;
  * every wrong-branch variant moves some output by >= 20 x its bar in >= 10 pairs (done_intended: >= 10 flips).

Every figure is printed (the condition table) before anything is asserted."""
import numpy as np
import pytest

from oracle import mpg_oracle as O
from tests import env_edge_inputs as E

BITE, BITE_PAIRS = 20., 10
# which output each variant is expected to move (all are measured and printed; the assertion is on the best one)
OUTPUTS = ('obs', 'full', 'rew', 'di')


def test_the_restatement_is_the_oracle_bit_for_bit():
    """LoggingEnvOracle in float32 == PathTrackingEnvOracle on the edge rows, closed loop, every output"""
    K = 3
    obs0, act = E.inputs(K)
    ref = O.PathTrackingEnvOracle(E.N, K)
    ref.reset(init_obs=obs0.copy())
    tr = E.trajectory(K)
    for t, rec in enumerate(tr['rec']):
        o, r, d, _ = ref.step(rec['act'])
        for got, want in ((rec['obs'], o), (rec['rew'], r), (rec['state'], ref.veh_state), (rec['full'], ref.veh_full_state)):
            assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), np.asarray(want, np.float32).view(np.int32)), t
        assert np.array_equal(rec['done'], d) and d.all()
        assert np.isfinite(o).all() and np.isfinite(r).all()


@pytest.mark.parametrize('K', [0, 3])
def test_the_edge_rows_reach_every_branch(K):
    obs0, act = E.inputs(K)
    assert obs0.shape == (E.N, 6 + K) and E.N % 16 and E.N % 64
    assert (obs0[E.rows_of('backwards'), 4] > np.pi).any() and obs0[E.ROW_SLOW, 0] + 20 < 1 and obs0[E.ROW_FAST, 0] + 20 > 35
    tr = E.trajectory(K)
    log, rec = tr['log'], tr['rec']
    c = E.branch_counts(log)
    inside = E.branch_counts(log, E.in_range_rows())
    di = np.stack([r['di'] for r in rec])
    terms = {k: np.stack([r['terms'][k] for r in rec]) for k in ('geo', 'alpha_f', 'alpha_r', 'r')}
    alone = {k: int((v & ~np.any([terms[j] for j in terms if j != k], 0)).sum()) for k, v in terms.items()}
    cmps = [r['cmp'] for r in rec]
    nr = E.near(log, cmps)
    cx, cphi, crel = E.closest(log, cmps)
    print('\nenv edges K=%d seed %d: %d agents x %d steps' % (K, E.SEED, E.N, len(rec)))
    print('   sub-steps clamped at 35 / 1: %d / %d   x wraps down / up %d / %d (agents starting inside the period: %d / %d)' % (
        c['clamp_hi'], c['clamp_lo'], c['x_down'], c['x_up'], inside['x_down'], inside['x_up']))
    print('   heading wraps down / up %d / %d   delta_phi wraps down / up %d / %d' % (c['phi_down'], c['phi_up'], c['dphi_down'], c['dphi_up']))
    print('   at the LAST sub-step: x %d / %d   heading %d / %d   delta_phi %d / %d   clamped %d / %d' % (
        inside['last_x_down'], inside['last_x_up'], c['last_phi_down'], c['last_phi_up'], c['last_dphi_down'], c['last_dphi_up'],
        c['last_clamp_hi'], c['last_clamp_lo']))
    print('   pairs with a path argument beyond 200: %d   agents with x_u < 0: %d   agents that leave the clamp at 35: %d' % (
        c['far_arg'], c['neg_x_agents'], c['leave_hi']))
    print('   done_intended 0 in %.1f %% of the pairs, 1 in %.1f %%; the only true term: %s' % (
        100 * (~di).mean(), 100 * di.mean(), ', '.join('%s %d' % kv for kv in alone.items())))
    print('   near pairs %d; closest approaches: x %.1e m, heading / delta_phi %.1e rad, a done comparison %.1e relative' % (
        nr.sum(), cx, cphi, crel))
    for k, least in E.CPU_MINIMUMS.items():
        assert c[k] >= least, (k, c[k], least)
    assert inside['x_down'] >= 10 and inside['x_up'] >= 10, inside
    # what the bit-identity tests of the device need at least once: a wrap of each kind at the last sub-step
    assert min(inside['last_x_down'], inside['last_x_up'], c['last_phi_down'], c['last_phi_up'], c['last_dphi_down'],
               c['last_dphi_up']) >= 1, (inside, c)
    assert c['leave_hi'] >= 2, c
    assert (~di).mean() >= 0.15 and di.mean() >= 0.15
    assert min(alone.values()) >= 3, alone
    assert not nr.any(), np.argwhere(nr)[:5]


@pytest.mark.parametrize('K', [0, 3])
def test_float32_oracle_is_inside_the_bars_from_float64(K):
    """one step from each state of the float32 closed loop, in float64: the worst |f32 - f64| / bar per entry"""
    tr = E.trajectory(K)
    wo, wf, wr = np.zeros(6 + K), np.zeros(6), 0.
    flips = 0
    for rec in tr['rec']:
        o64, lg = E.one_step(K, rec['before'], rec['act'], np.float64)
        xm = E.x_magnitude(lg, rec['before'][1][:, 5])
        ro, rf, rr = E.ratios(rec['obs'], rec['full'], rec['rew'], o64['obs'], o64['full'], o64['rew'], xm)
        wo, wf, wr = np.maximum(wo, ro.max(0)), np.maximum(wf, rf.max(0)), max(wr, rr.max())
        flips += int((o64['di'] != rec['di']).sum())
    names = E.ENTRY + tuple('ahead %d' % k for k in range(K))
    print('\nfloat32 oracle vs float64, K=%d, worst error / bar per entry' % K)
    print('   observation: ' + '  '.join('%s %.3f' % kv for kv in zip(names, wo)))
    print('   state:       ' + '  '.join('%s %.3f' % kv for kv in zip(E.FULL_ENTRY, wf)))
    print('   reward %.3f   done_intended flips %d' % (wr, flips))
    assert wo.max() <= 0.5 and wf.max() <= 0.5 and wr <= 0.5, (wo, wf, wr)
    assert flips == 0


@pytest.mark.parametrize('variant', E.VARIANTS + E.NO_BITE)
def test_every_wrong_branch_bites(variant):
    """one step of the wrong oracle from each state of the true closed loop (what the device test does with the kernel)"""
    K = 3
    tr = E.trajectory(K)
    pairs = dict.fromkeys(OUTPUTS, 0)
    for t, rec in enumerate(tr['rec']):
        w, _ = E.one_step(K, rec['before'], rec['act'], np.float32, variant)
        xm = E.x_magnitude(tr['log'][t], rec['before'][1][:, 5])
        with np.errstate(invalid='ignore'):
            ro, rf, rr = E.ratios(w['obs'], w['full'], w['rew'], rec['obs'].astype(np.float64), rec['full'].astype(np.float64), rec['rew'], xm)
        pairs['obs'] += int((np.nan_to_num(ro, nan=np.inf).max(1) >= BITE).sum())
        pairs['full'] += int((np.nan_to_num(rf, nan=np.inf).max(1) >= BITE).sum())
        pairs['rew'] += int((np.nan_to_num(rr, nan=np.inf) >= BITE).sum())
        pairs['di'] += int((w['di'] != rec['di']).sum())
    print('\n%-20s pairs moved by >= %.0f x the bar: observation %d, state %d, reward %d; done_intended flips %d' % (
        variant, BITE, pairs['obs'], pairs['full'], pairs['rew'], pairs['di']))
    if variant in E.NO_BITE:                         # measured and printed only: the reason it is not in the list
        assert max(pairs.values()) < BITE_PAIRS, (variant, pairs)
    else:
        assert max(pairs.values()) >= BITE_PAIRS, (variant, pairs)
