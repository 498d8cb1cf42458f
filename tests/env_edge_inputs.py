"""Start rows and actions that drive the REAL path-tracking env (mpg_amd/csrc/env_path_tracking.hip, step_agent) through its own
branches, and the oracle restatement that logs what enters them and says what a wrong branch would cost.  Shared by
tests/test_env_edges.py (CPU: the conditions that make the device test worth running) and tests/test_env_edges_gpu.py (the kernels
against the oracle on these inputs).  A plain helper module.

step_agent clamps v_x to [1, 35] inside each of its 20 sub-steps, wraps x into (0, 1200] and the heading into (-pi, pi] after each,
and wraps delta_phi, formed from the PRE-wrap heading and x of the last sub-step.  sincos_bounded takes the library routine beyond
|a| = 200, i.e. for a path argument x * 2 pi / 200 with x > 6366.  One step moves v_x by at most 0.3 and x by about 2 m and the reset
law starts with x in (0, 600), v_x in [15, 25] and a heading error of N(0, pi / 9), so inputs drawn from that law reach none of them."""
import functools

import numpy as np
import torch

from oracle import mpg_oracle as O
from tests.golden_inputs import reset_law_obs

G = 16                                                    # agents per group
GROUPS = ('brake', 'accelerate', 'period', 'backwards', 'spin left', 'spin right', 'far x', 'negative x', 'calm')
N_GROUPED = G * len(GROUPS)                               # 144
ROW_SLOW, ROW_FAST = N_GROUPED, N_GROUPED + 1             # two single rows: a start v_x of 0.5 and of 40
N = N_GROUPED + 2                                         # 146: no multiple of 64 or of 16
STEPS = 30
SEED = 28                                                 # chosen by tests/test_env_edges.py's conditions (near() false everywhere)
FAR_ARG_X = 200. * 200. / (2 * np.pi)                     # x beyond which the 200 m curve's path argument exceeds 200: 6366.2
VARIANTS = ('no v_x clamp', 'no x wrap', 'no heading wrap', 'no delta_phi wrap', 'unclipped reward', 'pre-step others')
# Stated by the oracle below, measured by tests/test_env_edges.py and NOT in the list, because they cannot bite:
#   'post-step others' (alpha_f, alpha_r and r_bounds from the state after the last sub-step instead of the one entering it): one
#   sub-step of 5 ms moves them by about 1e-3 relative, which flips done_intended in 0 of the 4380 pairs;
#   "delta_phi from the wrapped heading": before its own wrap it differs from the true delta_phi by exactly 2 pi wherever the heading
#   wrapped, and the wrap of delta_phi takes that away again.
# 'pre-step others' (those three from the state entering the FIRST sub-step, i.e. taken once before the loop) is what does bite
# on done_intended.
NO_BITE = ('post-step others',)


def rows_of(group):
    g = GROUPS.index(group)
    return slice(g * G, (g + 1) * G)


def in_range_rows():
    """the agents whose x starts inside (0, 1200]: every group but 'far x' and 'negative x', and the two single rows"""
    m = np.ones(N, bool)
    m[rows_of('far x')] = m[rows_of('negative x')] = False
    return m


# ---- start rows --------------------------------------------------------------------------------------------------------------
def edge_rows(rng, K=0):
    """(start observations [N][6 + K], actions [N][2] in the env's normalised units, held over a trajectory - see actions_at).
    Eight groups of 16 agents and a calm one, (v_x, delta_phi, x | steer, a_x):
      brake        1.5 .. 4      +-0.2        0 .. 600          | +-0.2        -1.2 .. -0.6   into the clamp at 1 (a_x beyond the clip)
      accelerate   33 .. 34.9    +-0.2        0 .. 600          | +-0.1        0.6 .. 1.2     into the clamp at 35
      period       15 .. 25      +-0.3        1150 .. 1199      | +-0.3        +-0.5          x > 1200 -> x - 1200
      backwards    15 .. 25      2.9 .. 3.3   0.5 .. 40         | +-0.1        +-0.5          x <= 0 -> x + 1200; a start heading error
                                                                                              partly beyond pi (no wrap at a reset)
      spin left    8 .. 15       +-3.1        0 .. 1200         | 0.7 .. 1.2   +-0.3          heading and delta_phi wraps at +pi
      spin right   8 .. 15       +-3.1        0 .. 1200         | -1.2 .. -0.7 +-0.3          ... at -pi
      far x        15 .. 25      +-0.3        5000 .. 29000 (8) | +-0.3        +-0.5          back by one period per sub-step; the
                                              29300 .. 40000 (8)                              second half keeps x_u > 6366 at the last
                                                                                              sub-step of step 0 (the sincosf branch)
      negative x   15 .. 25      +-0.3        -3000 .. -1 (8)   | +-0.3        +-0.5          negative path arguments at the reset; up by
                                              -40000 .. -24500 (8)                            one period per sub-step, so only the second
                                                                                              half still has x_u < 0 at the last sub-step
                                                                                              of step 0 (x0 + 19 periods; also sincosf)
      calm         the reset law (calm_rows)                    | +-0.1        +-0.1          done_intended false somewhere
    v_y ~ N(0, 0.2), r ~ U(-0.1, 0.1), delta_y ~ N(0, 0.5) in the eight groups.  Then one row that starts at v_x = 0.5 (braking) and one
    at v_x = 40 (accelerating): mpg_env_reset_from_obs takes both as they are.  Look-ahead entries (drawn last: the base entries do not
    depend on K) near delta_y; the env never reads them."""
    u = lambda lo, hi, n=G: rng.uniform(lo, hi, n)
    pm = lambda a, n=G: rng.uniform(-a, a, n)
    obs = reset_law_obs(rng, N).astype(np.float64)
    act = np.zeros((N, 2))
    table = [('brake', u(1.5, 4), pm(0.2), u(0, 600), pm(0.2), u(-1.2, -0.6)),
             ('accelerate', u(33, 34.9), pm(0.2), u(0, 600), pm(0.1), u(0.6, 1.2)),
             ('period', u(15, 25), pm(0.3), u(1150, 1199), pm(0.3), pm(0.5)),
             ('backwards', u(15, 25), u(2.9, 3.3), u(0.5, 40), pm(0.1), pm(0.5)),
             ('spin left', u(8, 15), pm(3.1), u(0, 1200), u(0.7, 1.2), pm(0.3)),
             ('spin right', u(8, 15), pm(3.1), u(0, 1200), u(-1.2, -0.7), pm(0.3)),
             ('far x', u(15, 25), pm(0.3), np.concatenate([u(5000, 29000, G // 2), u(29300, 40000, G // 2)]), pm(0.3), pm(0.5)),
             ('negative x', u(15, 25), pm(0.3), np.concatenate([u(-3000, -1, G // 2), u(-40000, -24500, G // 2)]), pm(0.3), pm(0.5))]
    for name, vx, dphi, x, steer, ax in table:
        s = rows_of(name)
        obs[s, 0], obs[s, 4], obs[s, 5] = vx - 20., dphi, x
        obs[s, 1], obs[s, 2], obs[s, 3] = rng.normal(0, 0.2, G), pm(0.1), rng.normal(0, 0.5, G)
        act[s, 0], act[s, 1] = steer, ax
    s = rows_of('calm')
    obs[s], act[s] = calm_rows(rng)
    obs[ROW_SLOW, 0], obs[ROW_SLOW, 1], act[ROW_SLOW] = 0.5 - 20., 0.02, (0.05, -0.5)
    obs[ROW_FAST, 0], act[ROW_FAST] = 40. - 20., (-0.05, 0.5)
    if K:
        obs = np.concatenate([obs, obs[:, 3:4] + 0.3 * rng.standard_normal((N, K))], 1)
    return np.ascontiguousarray(obs, np.float32), np.ascontiguousarray(act, np.float32)


def calm_rows(rng, pool=16384):
    """(observations [16][6], actions [16][2]): rows of the reset law with actions U(-0.1, 0.1), picked from a pool of such rows by
    the oracle's first step - four after which the front slip angle is the ONLY true term of done_intended, four the rear one, each
    comparison 2 % clear of its threshold, and the first eight of the others.  Why picked: in steady cornering |alpha_r| passes its
    bound where v r > 3 miu g and |r| > r_bounds already where v r > miu g, so a slip-angle term decides alone only in the transient
    after a start with a large side slip, which the law (beta ~ N(0, 0.15)) draws for about one row in thirty."""
    cand = reset_law_obs(rng, pool)
    a = rng.uniform(-0.1, 0.1, (pool, 2)).astype(np.float32)
    ora = LoggingEnvOracle(pool)
    ora.reset(init_obs=cand.copy())
    ora.step(a)
    cmp = ora.comparisons()
    fires = {k: l > r + 0.02 * np.abs(r) for k, (l, r) in cmp.items()}
    quiet = {k: l < r - 0.02 * np.abs(r) for k, (l, r) in cmp.items()}
    only = lambda k: np.flatnonzero(fires[k] & np.all([quiet[j] for j in quiet if j != k], 0))[:G // 4]
    pick = np.concatenate([only('alpha_f'), only('alpha_r')])
    assert len(pick) == G // 2, len(pick)
    rest = np.setdiff1d(np.arange(pool), pick)[:G - len(pick)]
    pick = np.concatenate([pick, rest])
    return cand[pick], a[pick]


def actions_at(act, t, steps=STEPS):
    """the actions of step t: constant per agent, but the last quarter of 'accelerate' reverses a_x for the second half of the
    trajectory, so that those agents enter the clamp at 35 and leave it again"""
    a = act.copy()
    if t >= steps // 2:
        s = rows_of('accelerate')
        a[s.stop - G // 4:s.stop, 1] *= -1
    return a


@functools.lru_cache(maxsize=None)
def inputs(K, seed=SEED):
    """edge_rows of the PCG64 stream `seed`; computed once and shared: nothing in it is written to later"""
    obs, act = edge_rows(np.random.Generator(np.random.PCG64(seed)), K)
    obs.setflags(write=False)
    act.setflags(write=False)
    return obs, act


# ---- the oracle with its branches switchable ---------------------------------------------------------------------------------
def _path_y(x):
    y = np.zeros_like(x)
    for A, T, s in O.CURVES:
        y += A * np.sin((x - s) * 2 * np.pi / T)
    return y


def _path_phi(x):
    d = np.zeros_like(x)
    for A, T, s in O.CURVES:
        d += A * 2 * np.pi / T * np.cos((x - s) * 2 * np.pi / T)
    return np.arctan(d)


class LoggingEnvOracle(O.PathTrackingEnvOracle):
    """PathTrackingEnvOracle with _simulation restated, operation by operation, so that
      * every sub-step's raw v_x (before the clamp), heading, x and delta_phi (before their wraps) go to self.log: one dict of
        [20][n] arrays per step;
      * dtype = np.float32 computes what the parent computes, bit for bit (tests/test_env_edges.py); np.float64 is the yardstick;
      * load() sets the two state arrays directly (reset(init_obs) rebuilds y and phi from the observation and would lose the
        device's bits);
      * done_terms() / done_intended() state "the evidently intended test" of include/mpg_hip.h from the oracle's own `others`;
      * variant (one of VARIANTS) takes one branch wrongly."""

    def __init__(self, num_agent, num_future_data=0, dtype=np.float32, variant=None):
        super().__init__(num_agent, num_future_data)
        assert variant is None or variant in VARIANTS + NO_BITE, variant
        self.dtype, self.variant = np.dtype(dtype), variant
        self.tdtype = torch.float32 if self.dtype == np.float32 else torch.float64
        self.log, self.others = [], None

    def load(self, veh_state, veh_full_state):
        self.veh_state = np.array(veh_state, self.dtype)
        self.veh_full_state = np.array(veh_full_state, self.dtype)
        return self

    def _get_obs(self, veh_state, veh_full_state=None):                 # the parent's, in self.dtype
        o = veh_state.copy()
        o[:, 0] = veh_state[:, 0] - O.EXPECTED_VS
        if self.num_future_data == 0:
            return o
        v_xs, ys, xs = veh_full_state[:, 0], veh_full_state[:, 3], veh_full_state[:, 5]
        x_ = xs.copy()
        fut = []
        for _ in range(self.num_future_data):
            x_ += v_xs * 1. / 200 * 20 * 2
            fut.append(ys - _path_y(x_))
        return np.concatenate([o, np.stack(fut, 1)], 1)

    def step(self, action):
        action = np.asarray(action, self.dtype)
        scaled = np.stack([action[:, 0] * 1.2 * np.pi / 9, action[:, 1] * 3], 1)
        hi = self.ACT_HIGH if self.dtype == np.float32 else np.array([1.2 * np.pi / 9, 3])
        clipped = np.clip(scaled, -hi, hi)
        st = torch.as_tensor(self.veh_state, dtype=self.tdtype)
        at = torch.as_tensor(clipped, dtype=self.tdtype)
        rew_action = torch.as_tensor(scaled, dtype=self.tdtype) if self.variant == 'unclipped reward' else at
        reward = O.compute_rewards_pt(st, rew_action).numpy()
        entering = self.veh_state
        self.veh_state, self.veh_full_state, self.others = self._simulate(self.veh_state, self.veh_full_state, at)
        if self.variant in ('post-step others', 'pre-step others'):   # alpha_f, alpha_r and r_bounds of another state than the last sub-step's
            src = self.veh_state if self.variant == 'post-step others' else entering
            _, post = O.f_xu(torch.as_tensor(src, dtype=self.tdtype), at, 1 / 200)
            post = post.numpy()
            self.others = np.stack([post[:, 0], post[:, 1], self.others[:, 2], self.others[:, 3], self.others[:, 4], post[:, 5]], 1)
        self.done = self._judge_done(self.veh_state, self.others)
        self.obs = self._get_obs(self.veh_state, self.veh_full_state)
        return self.obs, reward, self.done, {}

    def _simulate(self, states, full_states, actions, base_freq=200, simu_times=20):   # PathTrackingEnvOracle._simulation
        v = self.variant
        states, full_states = states.copy(), full_states.copy()
        rec = dict(vx=[], phi=[], x=[], dphi=[])
        for _ in range(simu_times):
            st = torch.as_tensor(states.copy(), dtype=self.tdtype)
            st, others = O.f_xu(st, actions, 1 / base_freq)
            states = st.numpy().copy()
            others = others.numpy()
            rec['vx'].append(states[:, 0].copy())
            if v != 'no v_x clamp':
                states[:, 0] = np.clip(states[:, 0], 1, 35)
            v_xs, v_ys, rs, phis = full_states[:, 0], full_states[:, 1], full_states[:, 2], full_states[:, 4]
            # NB: phis is a VIEW - y and x are integrated with the already-updated phi
            full_states[:, 4] += rs / base_freq
            full_states[:, 3] += (v_xs * np.sin(phis) + v_ys * np.cos(phis)) / base_freq
            full_states[:, -1] += (v_xs * np.cos(phis) - v_ys * np.sin(phis)) / base_freq
            full_states[:, 0:3] = states[:, 0:3].copy()
            py, pphi = _path_y(full_states[:, -1]), _path_phi(full_states[:, -1])
            states[:, 4] = full_states[:, 4] - pphi
            states[:, 3] = full_states[:, 3] - py
            rec['phi'].append(full_states[:, 4].copy())
            rec['x'].append(full_states[:, -1].copy())
            rec['dphi'].append(states[:, 4].copy())
            if v != 'no heading wrap':
                full_states[:, 4][full_states[:, 4] > np.pi] -= 2 * np.pi
                full_states[:, 4][full_states[:, 4] <= -np.pi] += 2 * np.pi
            if v != 'no x wrap':
                full_states[:, -1][full_states[:, -1] > O.PERIOD] -= O.PERIOD
                full_states[:, -1][full_states[:, -1] <= 0] += O.PERIOD
            states[:, -1] = full_states[:, -1]
            if v != 'no delta_phi wrap':
                states[:, 4][states[:, 4] > np.pi] -= 2 * np.pi
                states[:, 4][states[:, 4] <= -np.pi] += 2 * np.pi
        self.log.append({k: np.stack(a).astype(np.float64) for k, a in rec.items()})
        return states, full_states, others

    def comparisons(self):
        """the six comparisons of done_intended as (left, right) pairs, left > right being the term; the first three are `geo`"""
        vs, (alpha_f, alpha_r, r, afb, arb, rb) = self.veh_state.astype(np.float64), self.others.T.astype(np.float64)
        n = len(vs)
        return dict(delta_y=(np.abs(vs[:, 3]), np.full(n, 3.)), delta_phi=(np.abs(vs[:, 4]), np.full(n, np.pi / 4.)),
                    v_x=(-vs[:, 0], np.full(n, -2.)), alpha_f=(np.abs(alpha_f), np.abs(afb)), alpha_r=(np.abs(alpha_r), np.abs(arb)),
                    r=(np.abs(r), rb))

    def done_terms(self):
        c = {k: a > b for k, (a, b) in self.comparisons().items()}
        return dict(geo=c['delta_y'] | c['delta_phi'] | c['v_x'], alpha_f=c['alpha_f'], alpha_r=c['alpha_r'], r=c['r'])

    def done_intended(self):
        """geo | |alpha_f| > |alpha_f_bounds| | |alpha_r| > |alpha_r_bounds| | |r| > r_bounds (include/mpg_hip.h, mpg_env_step)"""
        t = self.done_terms()
        return t['geo'] | t['alpha_f'] | t['alpha_r'] | t['r']


# ---- what a log holds --------------------------------------------------------------------------------------------------------
def branch_counts(log, rows=None):
    """log of a LoggingEnvOracle ([steps] dicts of [20][n]) -> dict of counts; rows: a selection of agents.
    Sub-steps: clamped at either end, x / heading / delta_phi wrapped in either direction ('up': + a period, 'down': - a period).
    (agent, step) pairs: a wrap at the LAST sub-step (what the step's outputs depend on), a last-sub-step x_u whose path argument lies
    beyond 200.  Agents: x_u < 0 at some last sub-step; clamped at 35 at some sub-step and below 35 again at the very last."""
    sel = slice(None) if rows is None else rows
    vx, phi, x, dphi = [np.stack([s[k][:, sel] for s in log]) for k in ('vx', 'phi', 'x', 'dphi')]      # [steps][20][n]
    hi, lo = vx > 35., vx < 1.
    c = dict(clamp_hi=hi.sum(), clamp_lo=lo.sum(), x_down=(x > O.PERIOD).sum(), x_up=(x <= 0.).sum(),
             phi_down=(phi > np.pi).sum(), phi_up=(phi <= -np.pi).sum(), dphi_down=(dphi > np.pi).sum(), dphi_up=(dphi <= -np.pi).sum(),
             last_x_down=(x[:, -1] > O.PERIOD).sum(), last_x_up=(x[:, -1] <= 0.).sum(),
             last_phi_down=(phi[:, -1] > np.pi).sum(), last_phi_up=(phi[:, -1] <= -np.pi).sum(),
             last_dphi_down=(dphi[:, -1] > np.pi).sum(), last_dphi_up=(dphi[:, -1] <= -np.pi).sum(),
             last_clamp_hi=hi[:, -1].sum(), last_clamp_lo=lo[:, -1].sum(),
             far_arg=(np.abs(x[:, -1]) > FAR_ARG_X).sum(), neg_x_agents=(x[:, -1] < 0.).any(0).sum(),
             leave_hi=(hi.any((0, 1)) & ~hi[-1, -1]).sum())
    return {k: int(v) for k, v in c.items()}


CPU_MINIMUMS = dict(clamp_hi=100, clamp_lo=100, x_up=10, x_down=10, phi_up=5, phi_down=5, dphi_up=20, dphi_down=20, far_arg=4,
                    neg_x_agents=8)


def x_magnitude(step_log, x_before):
    """[n]: the largest |x| the step's arithmetic passed through - the x it started from and every sub-step's x before its wrap"""
    return np.maximum(np.abs(step_log['x']).max(0), np.abs(np.asarray(x_before, np.float64)))


def near(log, others):
    """[steps][n] bool: the (agent, step) pairs that sit within rounding of a threshold, where two correct float32 evaluations may
    fall on different sides.  log: of a LoggingEnvOracle; others: its comparisons() after each of those steps.  True where, at the LAST
    sub-step, x before its wrap is within 8 ulp (of the period, the largest |x| a wrap meets from inside) of 0 or 1200, or the heading
    or delta_phi before their wraps within 1e-5 of +-pi, or where a comparison of done_intended has its two sides within 1e-5 relative.
    Only the last sub-step counts: an earlier sub-step's wrap side changes nothing downstream, because the next sub-step wraps again
    and sine and cosine are periodic - x and the heading enter the later sub-steps through them alone."""
    out = []
    for s, cmp in zip(log, others):
        x, phi, dphi = s['x'][-1], s['phi'][-1], s['dphi'][-1]
        ulp = np.spacing(np.maximum(np.abs(x), O.PERIOD).astype(np.float32)).astype(np.float64)
        m = (np.abs(x) <= 8 * ulp) | (np.abs(x - O.PERIOD) <= 8 * ulp)
        m |= (np.abs(np.abs(phi) - np.pi) <= 1e-5) | (np.abs(np.abs(dphi) - np.pi) <= 1e-5)
        for a, b in cmp.values():
            m |= np.abs(a - b) <= 1e-5 * np.maximum(np.abs(a), np.abs(b))
        out.append(m)
    return np.stack(out)


def closest(log, others):
    """the closest approaches behind near(): (x to 0 / 1200 in m, heading and delta_phi to +-pi in rad, a done comparison, relative)"""
    x, phi, dphi = [np.stack([s[k][-1] for s in log]) for k in ('x', 'phi', 'dphi')]
    rel = min(float((np.abs(a - b) / np.maximum(np.abs(a), np.abs(b))).min()) for cmp in others for a, b in cmp.values())
    return (float(np.minimum(np.abs(x), np.abs(x - O.PERIOD)).min()),
            float(np.minimum(np.abs(np.abs(phi) - np.pi), np.abs(np.abs(dphi) - np.pi)).min()), rel)


# ---- the bars ----------------------------------------------------------------------------------------------------------------
ATOL = 5e-6
REW_BAR = (1e-5, 2e-6)                                   # (rtol, atol) of tests/test_env_gpu.py's reward comparisons
# The bar terms that the float32 ORACLE alone (against its float64 restatement, one step from the same state, tests/test_env_edges.py)
# exceeded half of, and the factor each is widened by: twice the oracle's measured worst error / bar, rounded up (v_x 5.74, v_y 1.04, delta_y 1.91,
# delta_phi 0.507, x 2.38, look-ahead 2.03, y 1.14; r 0.21 and phi 0.37 stay).  20 sub-steps round v_x at 35 (ulp 3.8e-6) and x at
# up to 40000 twenty times each; the 5e-6 of tests/test_env_gpu.py is sized for v_x in [15, 25] and x below 1200.  Never derived from
# a device's output.  DESIGN.md section 2 carries both numbers.
WIDENED = dict(obs=dict(v_x=11.5, v_y=2.1, delta_y=4.0, delta_phi=1.05, x=4.9, ahead=4.2), full=dict(v_x=11.5, v_y=2.1, y=2.4, x=4.9))


def _ulp32(a):
    return np.spacing(np.abs(np.asarray(a)).astype(np.float32)).astype(np.float64)


def bars(ref_obs, ref_full, x_mag=None):
    """(tolerance of the observation [n][6 + K], tolerance of veh_full_state [n][6]) around a reference.
    The observation's is the array of tests/test_env_gpu.py::_close_obs, restated: 5e-6 absolute everywhere, 4 ulp of x on x, 0.4 and
    0.02 of the x term on delta_y and delta_phi (|path slope| <= 0.37).  Added for these trajectories: 4 ulp of the float32 |y| on
    delta_y = y - path_y(x) and on every look-ahead entry y - path_y(x + k adv) - |y| reaches about 80 here, where one ulp, 7.6e-6,
    already exceeds the 5e-6 term - and the path-slope share of the x term on the look-ahead entries too.
    x_mag (x_magnitude()): the ulp of x is taken at the largest |x| the step passed through where that exceeds the result - a wrap
    makes x small AFTER the additions that rounded it at 1200, and the far rows come down from 40000.  Without it: the ulp of the
    result, as _close_obs.
    The state's: v_x, v_y, r, phi 5e-6; y 5e-6 + 4 ulp of |y|; x as in the observation."""
    ref_obs, ref_full = np.asarray(ref_obs, np.float64), np.asarray(ref_full, np.float64)
    xm = np.abs(ref_obs[:, 5]) if x_mag is None else np.maximum(np.abs(ref_obs[:, 5]), x_mag)
    tol = np.full(ref_obs.shape, ATOL)
    tol[:, 5] = 4 * _ulp32(xm) + ATOL
    yt = 4 * _ulp32(ref_full[:, 3])
    tol[:, 3] += 0.4 * tol[:, 5] + yt
    tol[:, 4] += 0.02 * tol[:, 5]
    tol[:, 6:] += (0.4 * tol[:, 5] + yt)[:, None]
    full = np.full(ref_full.shape, ATOL)
    full[:, 3] += yt
    full[:, 5] = tol[:, 5]
    for name, f in WIDENED['obs'].items():
        if name == 'ahead':
            tol[:, 6:] *= f
        else:
            tol[:, ENTRY.index(name)] *= f
    for name, f in WIDENED['full'].items():
        full[:, FULL_ENTRY.index(name)] *= f
    return tol, full


ENTRY = ('v_x', 'v_y', 'r', 'delta_y', 'delta_phi', 'x')
FULL_ENTRY = ('v_x', 'v_y', 'r', 'y', 'phi', 'x')


def ratios(got_obs, got_full, got_rew, ref_obs, ref_full, ref_rew, x_mag, skip=None):
    """|got - ref| / bar per (agent, entry): (observation [n][6 + K], state [n][6], reward [n]); skip [n] bool: the agents whose x,
    heading and delta_phi are not compared (near()) - their ratios there are 0"""
    tol, ftol = bars(ref_obs, ref_full, x_mag)
    ro = np.abs(np.asarray(got_obs, np.float64) - ref_obs) / tol
    rf = np.abs(np.asarray(got_full, np.float64) - ref_full) / ftol
    ref_rew = np.asarray(ref_rew, np.float64)
    rr = np.abs(np.asarray(got_rew, np.float64) - ref_rew) / (REW_BAR[1] + REW_BAR[0] * np.abs(ref_rew))
    if skip is not None:
        ro[np.ix_(skip, [4, 5])] = 0.
        rf[np.ix_(skip, [4, 5])] = 0.
    return ro, rf, rr


# ---- the oracle's closed loop ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trajectory(K, seed=SEED, steps=STEPS):
    """the float32 oracle's own closed loop on inputs(K, seed): per step the state it was taken from, the action and every output"""
    obs0, act = inputs(K, seed)
    ora = LoggingEnvOracle(N, K)
    ora.reset(init_obs=obs0.copy())
    rec = []
    for t in range(steps):
        a = actions_at(act, t, steps)
        before = (ora.veh_state.copy(), ora.veh_full_state.copy())
        obs, rew, done, _ = ora.step(a)
        rec.append(dict(before=before, act=a, obs=obs.copy(), rew=rew.copy(), done=done.copy(), state=ora.veh_state.copy(),
                        full=ora.veh_full_state.copy(), terms=ora.done_terms(), di=ora.done_intended(), cmp=ora.comparisons()))
    return dict(rec=rec, log=ora.log)


def one_step(K, before, act, dtype=np.float32, variant=None):
    """one step of a LoggingEnvOracle from the state pair `before` -> (dict of outputs, the step's log)"""
    ora = LoggingEnvOracle(len(act), K, dtype, variant).load(*before)
    obs, rew, done, _ = ora.step(act)
    return dict(obs=obs, rew=rew, done=done, state=ora.veh_state, full=ora.veh_full_state, terms=ora.done_terms(), di=ora.done_intended(),
                cmp=ora.comparisons()), ora.log[0]
