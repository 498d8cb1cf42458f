"""Start rows and actions that drive the cart-pole env (mpg_amd/csrc/env_cart_pole.hip, step_agent) to its control clamp, to both
sides of its two `done` bounds and to the angles, spin rates and cart positions a roll-out without a reset reaches, and the oracle
restatement that logs what a step passed through and says what a wrong term would cost.  Shared by tests/test_cart_pole_edges.py
(CPU: the conditions that make the device test worth running) and tests/test_cart_pole_edges_gpu.py (the kernels against the
oracle on these inputs).  A plain helper module, in the shape of tests/env_edge_inputs.py.

step_agent clips the action to +-3, runs two RK4 sub-steps of 0.02 s (sincosf of theta + theta0 in each of the eight derivative
evaluations) and tests done = not(|p| < 2 and |theta| <= 0.2) on the new state.  The reset law starts all four entries within
+-0.01 and every agent is re-drawn when it is done, so inputs drawn from that law see |theta| of a few radians at the most, no cart
beyond a few metres and nothing exactly at a bound.  mpg_env_rollout_pendulum ignores `done` for up to 1024 steps of 0.04 s: a
fallen pole that keeps turning hands sincosf angles of some hundreds of radians.

PARITY UNPINNED, as everywhere for this env: oracle.mpg_oracle.InvertedPendulumContiOracle alone says what the step computes."""
import functools

import numpy as np

from oracle import mpg_oracle as O

G = 16                                                    # agents per group
GROUPS = ('calm', 'circle', 'wound', 'spin', 'runaway', 'clamp', 'threshold theta', 'threshold p')
N_GROUPED = G * len(GROUPS)                               # 128
ROW_ZERO, ROW_CORNER = N_GROUPED, N_GROUPED + 1           # two single rows: everything 0; (1.999, 0.1999, 0, 0); action 0 in both
N = N_GROUPED + 2                                         # 130: no multiple of 16 or of 64
STEPS = 30
SEED = 0                                                  # chosen by tests/test_cart_pole_edges.py's conditions; see SEEDS_TRIED
SEEDS_TRIED = 1                                           # the first one met them all (with calm rows taken as they come, seeds 0 .. 11
                                                          # left `done` at 0 in 3.5 .. 5.3 % of the pairs: calm_rows says what was done)
TH0 = float(np.arctan2(0.001, 0.6))                       # the pole's rest axis against the hinge frame
P_BOUND, TH_BOUND = np.float32(2.), np.float32(.2)        # the float32 constants both the kernel and the float32 oracle compare with
CTRL = 3.
VARIANTS = ('no control clamp', 'no theta0', 'point mass', 'no centrifugal term', 'no cart damping', 'no hinge damping',
            'cos 1 in the determinant', 'one sub-step', 'euler', 'k4 at the half step', 'pre-step reward', 'done or',
            'done on theta + theta0')
# Stated by the oracle below, measured and printed by tests/test_cart_pole_edges.py and NOT in the list:
#   'done closed p' (|p| <= 2) and 'done open theta' (|theta| < 0.2) differ from the true test only for a post-step value EXACTLY on
#   its bound, which near() excludes;
#   'reduce theta' (theta + theta0 brought into [-pi, pi] by a float32 subtraction of a multiple of 2 pi before sin and cos) is what a
#   kernel with its own range reduction would do; what it costs at the wound rows is printed.
NO_BITE = ('done closed p', 'done open theta', 'reduce theta')


def rows_of(group):
    g = GROUPS.index(group)
    return slice(g * G, (g + 1) * G)


def group_of(row):
    return GROUPS[row // G] if row < N_GROUPED else ('zero', 'corner')[row - N_GROUPED]


# ---- start rows --------------------------------------------------------------------------------------------------------------
def calm_like(rng, n, p_max=1.9):
    """what the replay holds: |p| < p_max, |theta| <= 0.2, velocities within +-1, action U(-3, 3)"""
    obs = rng.uniform(-1, 1, (n, 4)) * np.array([p_max, 0.2, 1., 1.])
    return obs.astype(np.float32), rng.uniform(-3, 3, n).astype(np.float32)


def calm_rows(rng, pool=16384, steps=30):
    """(observations [16][4], actions [16]): the first four rows of a pool of calm-like rows, and the twelve that the float32 oracle
    keeps up longest under their constant action.  Why picked: a constant push of U(-3, 3) * 100 N turns the pole by about 10 |a| t^2
    rad, so a calm-like row is done after 3 steps on average (measured on the pool) and rows taken as they come leave `done` at 0 in
    3.5 .. 5.3 % of all pairs (seeds 0 .. 11; the conditions ask for 10 %); the replay of a policy that balances holds states with the action that keeps them up, which a constant
    action does only for the draws with |a| of a few tenths and thetadot against theta.  Every picked row is a draw of calm_like()."""
    cand, a = calm_like(rng, pool)
    ora = LoggingCartPoleOracle(pool)
    ora.reset(init_obs=cand)
    alive, life = np.ones(pool, bool), np.zeros(pool, int)
    for _ in range(steps):
        alive &= ~ora.step(a)[2]
        life += alive
    rest = np.arange(G // 4, pool)
    pick = np.concatenate([np.arange(G // 4), rest[np.argsort(-life[rest], kind='stable')[:G - G // 4]]])
    return cand[pick], a[pick]


CLAMP_ACTIONS = (3., -3., np.nextafter(np.float32(3), np.float32(np.inf)), -np.nextafter(np.float32(3), np.float32(np.inf)),
                 4.5, -3.75, 100., -1e6, np.inf, -np.inf)


def threshold_rows(rng, which, pool=16384):
    """(observations [16][4], actions [16]) picked from a pool of calm-like rows by the float32 oracle's first step, as
    tests/env_edge_inputs.calm_rows picks its rows: 8 whose post-step value lies just inside the bound and 8 just outside, none near().
      which = 'theta': |theta| in (0.2 - theta0, 0.2) and in (0.2, 0.2 + theta0), |p| < 1.9 (so that theta alone decides).  A test on
                       theta + theta0 is wrong only for theta > 0 inside and theta < 0 outside: six of each eight are of that sign,
                       two of the other (both signs are there on both sides);
      which = 'p':     |p| within 0.02 of 2 on either side, |theta| < 0.19 (p alone decides), four of each sign on each side; the
                       pool's carts start within +-2.1, a calm cart (|p| < 1.9, |pdot| <= 1) does not get there in one step."""
    cand, a = calm_like(rng, pool, 1.9 if which == 'theta' else 2.1)
    ora = LoggingCartPoleOracle(pool)
    ora.reset(init_obs=cand)
    o, _, _, _ = ora.step(a)
    o = o.astype(np.float64)
    ok = ~near_state(o)
    if which == 'theta':
        v, other_ok, lo, hi, want = o[:, 1], np.abs(o[:, 0]) < 1.9, 0.2 - TH0, 0.2 + TH0, (6, 2, 2, 6)
    else:
        v, other_ok, lo, hi, want = o[:, 0], np.abs(o[:, 1]) < 0.19, 1.98, 2.02, (4, 4, 4, 4)
    ok &= other_ok
    b = float(TH_BOUND if which == 'theta' else P_BOUND)
    inside, outside = ok & (np.abs(v) > lo) & (np.abs(v) < b), ok & (np.abs(v) > b) & (np.abs(v) < hi)
    pick = np.concatenate([np.flatnonzero(inside & (v > 0))[:want[0]], np.flatnonzero(inside & (v < 0))[:want[1]],
                           np.flatnonzero(outside & (v > 0))[:want[2]], np.flatnonzero(outside & (v < 0))[:want[3]]])
    assert len(pick) == G, (which, len(pick))
    return cand[pick], a[pick]


def edge_rows(rng):
    """(start observations [N][4], actions [N], held over the trajectory).  Eight groups of 16 agents, (p, theta, pdot, thetadot | action):
      calm             |p| < 1.9       |theta| <= 0.2      +-1          +-1        | U(-3, 3)    what the replay holds (calm_rows: 4 as
                                                                                                 they come, the 12 longest-lived of a pool)
      circle           calm            linspace(-pi, pi, 17)[1:]   calm            | U(-3, 3)    float32 pi itself a member
      wound            calm            +-U(50, 500)        calm         +-10       | U(-3, 3)    sincosf after a long roll-out
      spin             calm            calm                calm         +-U(15, 40)| U(-3, 3)    m l sin(theta) thetadot^2 dominates
      runaway          +-U(20, 60)     calm                +-U(5, 30)   calm       | U(-3, 3)
      clamp            calm                                                        | CLAMP_ACTIONS in turn: exactly +-3, one ulp beyond,
                                                                                     4.5, -3.75, 100, -1e6, +-inf
      threshold theta  post-step |theta| within theta0 of 0.2, either side (threshold_rows)
      threshold p      post-step |p| within 0.02 of 2, either side
    then a row of zeros and one at (1.999, 0.1999, 0, 0), both with action 0."""
    u = lambda lo, hi, n=G: rng.uniform(lo, hi, n)
    sign = lambda n=G: np.where(rng.random(n) < 0.5, -1., 1.)
    obs, act = calm_like(rng, N)
    obs = obs.astype(np.float64)
    obs[rows_of('circle'), 1] = np.linspace(-np.pi, np.pi, G + 1)[1:]
    s = rows_of('wound')
    obs[s, 1], obs[s, 3] = sign() * u(50, 500), u(-10, 10)
    obs[rows_of('spin'), 3] = sign() * u(15, 40)
    s = rows_of('runaway')
    obs[s, 0], obs[s, 2] = sign() * u(20, 60), sign() * u(5, 30)
    obs = obs.astype(np.float32)
    obs[rows_of('calm')], act[rows_of('calm')] = calm_rows(rng)
    act[rows_of('clamp')] = [CLAMP_ACTIONS[i % len(CLAMP_ACTIONS)] for i in range(G)]
    for which in ('theta', 'p'):
        s = rows_of('threshold ' + which)
        obs[s], act[s] = threshold_rows(rng, which)
    obs[ROW_ZERO], act[ROW_ZERO] = 0., 0.
    obs[ROW_CORNER], act[ROW_CORNER] = (1.999, 0.1999, 0., 0.), 0.
    assert np.float32(np.pi) in obs[rows_of('circle'), 1]
    return np.ascontiguousarray(obs, np.float32), np.ascontiguousarray(act, np.float32)


@functools.lru_cache(maxsize=None)
def inputs(seed=SEED):
    """edge_rows of the PCG64 stream `seed`; computed once and shared: nothing in it is written to later"""
    obs, act = edge_rows(np.random.Generator(np.random.PCG64(seed)))
    obs.setflags(write=False)
    act.setflags(write=False)
    return obs, act


# ---- the oracle with its terms switchable ------------------------------------------------------------------------------------
class LoggingCartPoleOracle(O.InvertedPendulumContiOracle):
    """InvertedPendulumContiOracle with _deriv and step restated, operation by operation, so that
      * every step's clipped action, the largest |theta + theta0| its eight derivative evaluations took sine and cosine of, and the
        |theta + theta0| and |thetadot| each of its two sub-steps started from go to self.log: one dict per step;
      * dtype = np.float32 computes what the parent computes, bit for bit (tests/test_cart_pole_edges.py); np.float64 is the yardstick;
      * variant (one of VARIANTS + NO_BITE) takes one term wrongly."""

    def __init__(self, num_agent, dtype=np.float32, variant=None):
        super().__init__(num_agent, dtype)
        assert variant is None or variant in VARIANTS + NO_BITE, variant
        self.variant, self.log, self._arg = variant, [], None

    def load(self, state):
        self.state = np.array(state, self.dt_)
        return self

    def _deriv(self, s, force):
        c, v = self.c, self.variant
        th, pd, thd = s[:, 1] + (0. if v == 'no theta0' else c['th0']), s[:, 2], s[:, 3]
        self._arg = np.maximum(self._arg, np.abs(th).astype(np.float64))
        if v == 'reduce theta':
            two_pi = self.dt_(2 * np.pi)
            th = th - two_pi * np.rint(th / two_pi)
        sn, cs = np.sin(th), np.cos(th)
        a11, a12, a22 = c['M'] + c['m'], c['m'] * c['l'] * cs, (0. if v == 'point mass' else c['I']) + c['m'] * c['l'] ** 2
        b1 = force - (0. if v == 'no cart damping' else self.DAMP_X) * pd
        if v != 'no centrifugal term':
            b1 = b1 + c['m'] * c['l'] * sn * thd * thd
        b2 = c['m'] * self.G * c['l'] * sn - (0. if v == 'no hinge damping' else self.DAMP_TH) * thd
        det = a11 * a22 - ((c['m'] * c['l']) ** 2 if v == 'cos 1 in the determinant' else a12 * a12)
        pdd = (a22 * b1 - a12 * b2) / det
        thdd = (a11 * b2 - a12 * b1) / det
        return np.stack([pd, thd, pdd, thdd], 1)

    def step(self, action):
        v = self.variant
        action = np.asarray(action, self.dt_).reshape(self.n)
        ctrl = action if v == 'no control clamp' else np.clip(action, -self.CTRL, self.CTRL)
        force = self.GEAR * ctrl
        s, h = self.state, self.dt_(self.DT)
        before = s
        self._arg = np.zeros(self.n)
        th_in, thd_in = [], []
        with np.errstate(invalid='ignore', over='ignore'):
            for _ in range(1 if v == 'one sub-step' else self.FRAME_SKIP):
                th_in.append(np.abs(s[:, 1] + self.c['th0']).astype(np.float64))
                thd_in.append(np.abs(s[:, 3]).astype(np.float64))
                k1 = self._deriv(s, force)
                if v == 'euler':
                    s = s + h * k1
                    continue
                k2 = self._deriv(s + 0.5 * h * k1, force)
                k3 = self._deriv(s + 0.5 * h * k2, force)
                k4 = self._deriv(s + (0.5 * h if v == 'k4 at the half step' else h) * k3, force)
                s = s + (h / 6) * (k1 + 2 * k2 + 2 * k3 + k4)
            self.state = s
            r = before if v == 'pre-step reward' else s
            p, th, pd, thd = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
            reward = -(0.01 * p * p + th * th) - (0.1 * pd * pd + 0.1 * thd * thd)
            p, th = s[:, 0], s[:, 1]
            if v == 'done on theta + theta0':
                th = th + self.c['th0']
            p_in = np.abs(p) <= 2. if v == 'done closed p' else np.abs(p) < 2.
            th_in_range = np.abs(th) < .2 if v == 'done open theta' else np.abs(th) <= .2
            done = ~(p_in | th_in_range) if v == 'done or' else ~(p_in & th_in_range)
        self.log.append(dict(action=action.astype(np.float64), ctrl=np.asarray(ctrl, np.float64), arg=self._arg, th_in=np.stack(th_in),
                             thd_in=np.stack(thd_in)))
        return s.copy(), reward, done, {}


# ---- what a trajectory holds -------------------------------------------------------------------------------------------------
def done_terms(obs):
    """(|p| >= 2, |theta| > 0.2) of post-step states [..., 4], against the float32 constants"""
    o = np.asarray(obs)
    return ~(np.abs(o[..., 0]) < P_BOUND), ~(np.abs(o[..., 1]) <= TH_BOUND)


def branch_counts(log, obs, done):
    """log of a LoggingCartPoleOracle ([steps] dicts), its post-step states [steps][n][4] and done flags [steps][n] -> counts of
    (agent, step) pairs: done 0 / 1; among done, |p| >= 2 alone and |theta| > 0.2 alone; the action clipped at either end and exactly
    at +-3 unclipped; |theta + theta0| > 50 or |thetadot| > 15 going into a sub-step"""
    act = np.stack([s['action'] for s in log])
    p_out, th_out = done_terms(obs)
    assert np.array_equal(np.asarray(done, bool), p_out | th_out)
    c = dict(done0=(~done).sum(), done1=done.sum(), p_alone=(p_out & ~th_out).sum(), theta_alone=(th_out & ~p_out).sum(),
             clip_hi=(act > CTRL).sum(), clip_lo=(act < -CTRL).sum(), at_hi=(act == CTRL).sum(), at_lo=(act == -CTRL).sum(),
             wound=np.stack([(s['th_in'] > 50.).any(0) for s in log]).sum(), fast=np.stack([(s['thd_in'] > 15.).any(0) for s in log]).sum())
    return {k: int(v) for k, v in c.items()}


PAIRS = N * STEPS                                          # 3900
CPU_MINIMUMS = dict(done0=PAIRS // 10, done1=PAIRS // 10, p_alone=10, theta_alone=10, clip_hi=30, clip_lo=30, at_hi=4, at_lo=4, wound=100,
                    fast=100)
EXACT_COUNTS = ('clip_hi', 'clip_lo', 'at_hi', 'at_lo')    # of the actions alone: the same on any trajectory


def near_state(obs):
    """[...] bool: post-step states [..., 4] whose |p| or |theta| lies within 1e-5 relative of 2 or 0.2 - where two correct float32
    evaluations may fall on different sides of a done bound"""
    o = np.asarray(obs, np.float64)
    return (np.abs(np.abs(o[..., 0]) - 2.) <= 2e-5) | (np.abs(np.abs(o[..., 1]) - float(TH_BOUND)) <= 1e-5 * float(TH_BOUND))


def near(obs):
    return near_state(obs)


def closest(obs):
    """the closest approaches behind near(), relative: (|p| to 2, |theta| to 0.2)"""
    o = np.asarray(obs, np.float64)
    return float(np.abs(np.abs(o[..., 0]) - 2.).min() / 2.), float(np.abs(np.abs(o[..., 1]) - float(TH_BOUND)).min() / float(TH_BOUND))


# ---- the bars ----------------------------------------------------------------------------------------------------------------
ENTRY = ('p', 'theta', 'pdot', 'thetadot')
OBS_BAR = 3e-6                                           # relative to scale: tests/test_env_gpu.py::test_cart_pole_env_vs_float64_restatement
REW_BAR = (2e-5, 1e-5)                                   # (rtol, atol) of the same test's reward comparison
# The added term: ARG_ULPS[entry] * ulp32(the largest |theta + theta0| the step took sine and cosine of).  sincosf sees the float32
# sum theta + theta0: at |theta| = 500 one rounding of it is 1.5e-5 rad, which the accelerations (up to m l thetadot^2 / (M + m) per
# unit of sine) carry into pdot and thetadot, and 0.04 s of those into p and theta.  Measured on the float32 ORACLE alone against its
# float64 restatement, one step from the same state (tests/test_cart_pole_edges.py): the worst error in units of that ulp over the
# pairs where the oracle takes more than half of the plain bar, doubled and rounded up; 0 where no pair does.  Never derived from a
# device's output.  DESIGN.md section 2 carries the measured figures.
# Measured (seed 0): worst error / plain bar p 0.035, theta 0.036, pdot 0.657, thetadot 6.401 - all of it in the wound group, 0.067 at the
# most where |theta + theta0| <= pi; in ulps of the argument pdot 0.322, thetadot 1.478; p and theta need nothing.
ARG_ULPS = dict(p=0., theta=0., pdot=0.65, thetadot=3.)


def _ulp32(a):
    return np.spacing(np.abs(np.asarray(a)).astype(np.float32)).astype(np.float64)


def bars(ref_obs, arg=None, arg_ulps=None):
    """tolerance of the observation / state [n][4] around a reference: OBS_BAR * (1 + |ref|), plus ARG_ULPS of the ulp of `arg`
    ([n], the step log's 'arg') where that is given"""
    ref_obs = np.asarray(ref_obs, np.float64)
    tol = OBS_BAR * (1. + np.abs(ref_obs))
    if arg is not None:
        k = ARG_ULPS if arg_ulps is None else arg_ulps
        tol = tol + _ulp32(arg)[:, None] * np.array([k[e] for e in ENTRY])
    return tol


def ratios(got_obs, got_rew, ref_obs, ref_rew, arg, arg_ulps=None):
    """|got - ref| / bar per (agent, entry): (observation [n][4], reward [n])"""
    ref_obs, ref_rew = np.asarray(ref_obs, np.float64), np.asarray(ref_rew, np.float64)
    ro = np.abs(np.asarray(got_obs, np.float64) - ref_obs) / bars(ref_obs, arg, arg_ulps)
    rr = np.abs(np.asarray(got_rew, np.float64) - ref_rew) / (REW_BAR[1] + REW_BAR[0] * np.abs(ref_rew))
    return ro, rr


# ---- the oracle's closed loop ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trajectory(seed=SEED, steps=STEPS, dtype=np.float32):
    """the oracle's own closed loop on inputs(seed): per step the state it was taken from, the action and every output"""
    obs0, act = inputs(seed)
    ora = LoggingCartPoleOracle(N, dtype)
    ora.reset(init_obs=obs0)
    rec = []
    for _ in range(steps):
        before = ora.state.copy()
        obs, rew, done, _ = ora.step(act)
        rec.append(dict(before=before, act=act, obs=obs.copy(), rew=rew.copy(), done=done.copy()))
    return dict(rec=rec, log=ora.log)


def one_step(before, act, dtype=np.float32, variant=None):
    """one step of a LoggingCartPoleOracle from the state `before` -> (dict of outputs, the step's log)"""
    ora = LoggingCartPoleOracle(len(act), dtype, variant).load(before)
    obs, rew, done, _ = ora.step(act)
    return dict(obs=obs, rew=rew, done=done), ora.log[0]
