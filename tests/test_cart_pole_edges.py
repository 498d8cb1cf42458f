"""The conditions that make tests/test_cart_pole_edges_gpu.py worth running, by the oracle alone (CPU), on the float32 oracle's own
30-step closed loop over the start rows of tests/cart_pole_edge_inputs.py:

  * the logging restatement in float32 is InvertedPendulumContiOracle(n, np.float32) bit for bit, and every state stays finite;
  * `done` is 0 and 1 often enough, each of its two terms decides alone somewhere, the action is clipped at both ends and sits exactly
    at +-3 unclipped, sine and cosine see |theta + theta0| > 50 and the sub-steps |thetadot| > 15;
  * no (agent, step) pair sits within rounding of a done bound (near() is false everywhere): the device test leaves out nothing;
  * the float32 oracle is inside half of every bar of bars() from its float64 restatement, one step from the same state, and
    ARG_ULPS is what the house rule makes of that measurement: the bars test the kernel and not the arithmetic;
  * every wrong-term variant moves some output by >= 20 x its bar in >= 10 pairs, or flips `done` in >= 10 pairs;
  * tests/test_env_gpu.py::test_cart_pole_env_vs_float64_restatement leaves out at most 1 % of its pairs as near a bound, shown on the
    float64 oracle under the same action draws.

Every figure is printed (the condition table) before anything is asserted."""
import math

import numpy as np
import pytest

from oracle import mpg_oracle as O
from tests import cart_pole_edge_inputs as E

BITE, BITE_PAIRS = 20., 10


def _stacked(tr):
    return np.stack([r['obs'] for r in tr['rec']]), np.stack([r['done'] for r in tr['rec']])


def test_the_restatement_is_the_oracle_bit_for_bit():
    """LoggingCartPoleOracle in float32 == InvertedPendulumContiOracle(n, np.float32) on the edge rows, closed loop, every output;
    in float64 == the float64 oracle"""
    obs0, act = E.inputs()
    for dtype, view in ((np.float32, np.int32), (np.float64, np.int64)):
        ref = O.InvertedPendulumContiOracle(E.N, dtype)
        ref.reset(init_obs=obs0)
        tr = E.trajectory(dtype=dtype)
        with np.errstate(invalid='ignore', over='ignore'):
            for t, rec in enumerate(tr['rec']):
                o, r, d, _ = ref.step(act)
                for got, want in ((rec['obs'], o), (rec['rew'], r)):
                    assert got.dtype == dtype and np.array_equal(got.view(view), np.asarray(want, dtype).view(view)), (dtype, t)
                assert np.array_equal(rec['done'], d), t
                assert np.isfinite(o).all() and np.isfinite(r).all(), t


def test_the_edge_rows_reach_every_branch():
    obs0, act = E.inputs()
    assert obs0.shape == (E.N, 4) and act.shape == (E.N,) and E.N % 16 and E.N % 64 and E.PAIRS == 3900
    assert np.float32(np.pi) in obs0[E.rows_of('circle'), 1] and (np.abs(obs0[E.rows_of('wound'), 1]) >= 50).all()
    assert (np.abs(obs0[E.rows_of('spin'), 3]) >= 15).all() and (np.abs(obs0[E.rows_of('runaway'), 0]) >= 20).all()
    assert np.isinf(act[E.rows_of('clamp')]).sum() == 2 and set(E.CLAMP_ACTIONS) == set(act[E.rows_of('clamp')].tolist())
    tr = E.trajectory()
    obs, done = _stacked(tr)
    c = E.branch_counts(tr['log'], obs, done)
    nr = E.near(obs)
    cp, cth = E.closest(obs)
    # the threshold groups did what they were picked for, at the first step
    th, p = obs[0, E.rows_of('threshold theta'), 1].astype(np.float64), obs[0, E.rows_of('threshold p'), 0].astype(np.float64)
    th_in, th_out = (np.abs(th) < 0.2) & (np.abs(th) > 0.2 - E.TH0), (np.abs(th) > 0.2) & (np.abs(th) < 0.2 + E.TH0)
    p_in, p_out = (np.abs(p) < 2.) & (np.abs(p) > 1.98), (np.abs(p) > 2.) & (np.abs(p) < 2.02)
    # the two closed loops part: how many done flags the float64 oracle's own closed loop gives differently (what "a handful" is)
    obs64, done64 = _stacked(E.trajectory(dtype=np.float64))
    c64 = E.branch_counts(E.trajectory(dtype=np.float64)['log'], obs64.astype(np.float32), done64)
    print('\ncart-pole edges, seed %d (%d tried): %d agents x %d steps = %d pairs' % (E.SEED, E.SEEDS_TRIED, E.N, len(tr['rec']), E.PAIRS))
    print('   done 0 in %d pairs (%.1f %%), 1 in %d (%.1f %%); |p| >= 2 alone %d, |theta| > 0.2 alone %d' % (
        c['done0'], 100. * c['done0'] / E.PAIRS, c['done1'], 100. * c['done1'] / E.PAIRS, c['p_alone'], c['theta_alone']))
    print('   action clipped at +3 / -3 in %d / %d pairs, exactly +3 / -3 unclipped in %d / %d' % (c['clip_hi'], c['clip_lo'], c['at_hi'], c['at_lo']))
    print('   pairs with |theta + theta0| > 50 going into a sub-step: %d; with |thetadot| > 15: %d' % (c['wound'], c['fast']))
    print('   after 30 steps: |p| <= %.1f, |theta| <= %.1f, |pdot| <= %.1f, |thetadot| <= %.1f; over all steps |thetadot| <= %.1f' % (
        *np.abs(obs[-1]).max(0), np.abs(obs[..., 3]).max()))
    print('   threshold theta at step 0: %d inside (signs +%d / -%d), %d outside (+%d / -%d); threshold p: %d inside, %d outside' % (
        th_in.sum(), (th[th_in] > 0).sum(), (th[th_in] < 0).sum(), th_out.sum(), (th[th_out] > 0).sum(), (th[th_out] < 0).sum(), p_in.sum(), p_out.sum()))
    print('   near pairs %d; closest approaches, relative: |p| to 2 %.1e, |theta| to 0.2 %.1e' % (nr.sum(), cp, cth))
    print('   the float64 closed loop counts: ' + '  '.join('%s %d' % (k, c64[k]) for k in E.CPU_MINIMUMS))
    assert np.isfinite(obs).all()
    for k, least in E.CPU_MINIMUMS.items():
        assert c[k] >= least, (k, c[k], least)
    assert th_in.sum() == 8 and th_out.sum() == 8 and p_in.sum() == 8 and p_out.sum() == 8
    assert min((th[th_in] > 0).sum(), (th[th_in] < 0).sum(), (th[th_out] > 0).sum(), (th[th_out] < 0).sum()) >= 2
    assert not nr.any(), np.argwhere(nr)[:5]


def measured_arg_ulps():
    """one step from each state of the float32 closed loop, in float64: per entry the worst |f32 - f64| / plain bar, and the worst
    error in ulps of the sincos argument over the pairs beyond half of the plain bar"""
    tr = E.trajectory()
    plain, ulps, rew, flips = np.zeros(4), np.zeros(4), 0., 0
    small_arg = np.zeros(4)
    for rec in tr['rec']:
        o64, lg = E.one_step(rec['before'], rec['act'], np.float64)
        err = np.abs(rec['obs'].astype(np.float64) - o64['obs'])
        r = err / E.bars(o64['obs'])
        plain = np.maximum(plain, r.max(0))
        small_arg = np.maximum(small_arg, r[lg['arg'] <= np.pi + 0.01].max(0))
        in_ulps = np.where(r > 0.5, err / E._ulp32(lg['arg'])[:, None], 0.)
        ulps = np.maximum(ulps, in_ulps.max(0))
        rew = max(rew, E.ratios(rec['obs'], rec['rew'], o64['obs'], o64['rew'], None)[1].max())
        flips += int((o64['done'] != rec['done']).sum())
    return plain, small_arg, ulps, rew, flips


def house_rule(worst):
    """twice the oracle's own worst, rounded up to two significant digits; 0 where the plain bar already holds the oracle twice"""
    if worst == 0.:
        return 0.
    e = 10. ** (math.floor(math.log10(2 * worst)) - 1)
    return round(math.ceil(2 * worst / e - 1e-9) * e, 12)


def test_float32_oracle_is_inside_the_bars_from_float64():
    plain, small_arg, ulps, rew, flips = measured_arg_ulps()
    print('\nfloat32 oracle vs float64, one step from the same state, per entry (%s)' % ', '.join(E.ENTRY))
    print('   worst error / plain bar (3e-6 relative to scale): ' + '  '.join('%.3f' % x for x in plain))
    print('   ... over the pairs with |theta + theta0| <= pi:     ' + '  '.join('%.3f' % x for x in small_arg))
    print('   worst error in ulp32(max |theta + theta0|) beyond half a plain bar: ' + '  '.join('%.3f' % x for x in ulps))
    print('   house rule -> ARG_ULPS ' + '  '.join('%s %g' % (e, house_rule(u)) for e, u in zip(E.ENTRY, ulps)))
    wo, wr = np.zeros(4), 0.
    per_group = {}
    tr = E.trajectory()
    for rec, lg in zip(tr['rec'], tr['log']):
        o64, lg64 = E.one_step(rec['before'], rec['act'], np.float64)
        ro, rr = E.ratios(rec['obs'], rec['rew'], o64['obs'], o64['rew'], lg64['arg'])
        wo, wr = np.maximum(wo, ro.max(0)), max(wr, rr.max())
        for i in range(E.N):
            per_group[E.group_of(i)] = max(per_group.get(E.group_of(i), 0.), ro[i].max())
    print('   with ARG_ULPS: worst error / bar ' + '  '.join('%s %.3f' % kv for kv in zip(E.ENTRY, wo)) + '   reward %.3f   done flips %d' % (wr, flips))
    print('   per group: ' + '  '.join('%s %.3f' % kv for kv in per_group.items()))
    for e, u in zip(E.ENTRY, ulps):
        assert E.ARG_ULPS[e] == house_rule(u), (e, E.ARG_ULPS[e], house_rule(u), u)
    assert wo.max() <= 0.5 and wr <= 0.5, (wo, wr)
    assert small_arg.max() <= 0.5, small_arg            # the widening is for the wound angles alone
    assert flips == 0


@pytest.mark.parametrize('variant', E.VARIANTS + E.NO_BITE)
def test_every_wrong_term_bites(variant):
    """one step of the wrong oracle from each state of the true closed loop (what the device test does with the kernel)"""
    tr = E.trajectory()
    pairs = dict(obs=0, rew=0, done=0)
    wound = dict(obs=0., rew=0.)
    for t, rec in enumerate(tr['rec']):
        w, _ = E.one_step(rec['before'], rec['act'], np.float32, variant)
        with np.errstate(invalid='ignore'):
            ro, rr = E.ratios(w['obs'], w['rew'], rec['obs'], rec['rew'], tr['log'][t]['arg'])
        ro, rr = np.nan_to_num(ro, nan=np.inf), np.nan_to_num(rr, nan=np.inf)
        pairs['obs'] += int((ro.max(1) >= BITE).sum())
        pairs['rew'] += int((rr >= BITE).sum())
        pairs['done'] += int((w['done'] != rec['done']).sum())
        wound = dict(obs=max(wound['obs'], ro[E.rows_of('wound')].max()), rew=max(wound['rew'], rr[E.rows_of('wound')].max()))
    print('\n%-26s pairs moved by >= %.0f x the bar: observation %d, reward %d; done flips %d' % (variant, BITE, pairs['obs'], pairs['rew'], pairs['done']))
    if variant == 'reduce theta':                      # measured and printed only
        print('%-26s at the wound rows: worst observation error / bar %.3f, reward %.3f' % ('', wound['obs'], wound['rew']))
    elif variant in E.NO_BITE:                         # a flip needs a value exactly on its bound; no pair is even near one
        assert pairs == dict(obs=0, rew=0, done=0), (variant, pairs)
    else:
        assert max(pairs.values()) >= BITE_PAIRS, (variant, pairs)


def test_the_existing_random_walk_leaves_out_few_pairs_on_the_oracle():
    """tests/test_env_gpu.py::test_cart_pole_env_vs_float64_restatement drops the pairs within 1e-4 of a done bound and asserts that
    they are at most 1 % of all.  The float64 oracle's closed loop from that test's own starts (the device's reset draw, seed 3,
    counter 0) under its own action draws (PCG64(11), U(-3.5, 3.5), n = 1, 64, 1000 in turn, 50 steps, no reset) leaves out far
    fewer: a window of 2e-4 around each of four bounds, against states that spread over radians and metres."""
    rng = np.random.Generator(np.random.PCG64(11))
    left_out = pairs = 0
    for n in (1, 64, 1000):
        ora = O.InvertedPendulumContiOracle(n)
        ora.reset(init_obs=O.cart_pole_reset_philox(n, 3, 0))
        for _ in range(50):
            a = rng.uniform(-3.5, 3.5, (n, 1)).astype(np.float32)
            o, _, _, _ = ora.step(a[:, 0].astype(np.float64))
            left_out += int(((np.abs(np.abs(o[:, 0]) - 2.0) < 1e-4) | (np.abs(np.abs(o[:, 1]) - 0.2) < 1e-4)).sum())
            pairs += n
    print('\nthe 50-step random walk on the float64 oracle: %d of %d pairs within 1e-4 of a done bound (%.3f %%)' % (left_out, pairs, 100. * left_out / pairs))
    assert left_out <= 0.005 * pairs, (left_out, pairs)         # half of what the device test allows
