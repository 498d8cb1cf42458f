"""Writes tests/golden/model_mpc_ref.npz: optimal-control solutions on the learners' own models, for tests/test_model_mpc.py and
tests/test_model_mpc_gpu.py.      python -m tests.golden.make_golden_model_mpc          (scipy is used HERE only)

Per (model, horizon) 16 candidate start rows, float32-rounded, from each model's start law (tests/test_model_rollout_gpu.start_rows'
laws; the double pendulum's narrowed, below), noise terms at their means, and for each row
    best       the float64 optimum of tests/model_mpc_oracle.horizon_cost over the box: the lowest of L-BFGS-B from zeros and from two
               random starts (gradients by autograd), and the point u_best
    spg64_*    the float64 emulation of the solver (model_mpc_oracle.spg_solve) from zeros at 200 iterations: its cost
    spg32_*    the float32 emulation likewise: its point, and the float64 cost at that point minus best (the yard-stick of the device's gap)
    kept       the row is kept iff the three L-BFGS-B runs agree to 1e-9 relative AND the float64 emulation ends within
               1e-6 * max(best, 1) of best: where the problem has one minimiser and the method finds it.
At least 12 of each 16 rows must be kept (asserted).  A set that falls short gets a shorter horizon, never a looser rule.

Horizons: PathTracking (K = 0) 20 and 5 - at 25 only 11 of its 16 rows are kept: on one the three L-BFGS-B runs agree on 12.41 and the
emulation ends 9.94 BELOW them, on four the runs disagree -; pendulum 25 and 5; double pendulum 10 and 5 with start angles and cart position within +-0.05
and velocities 0.05 sigma - at horizon 25 from +-0.1 the double pendulum's solve is not unique (L-BFGS-B ends at 16.07 from zeros and at
35.42 from a random start on one row, neither converged after 500 iterations), at 5 and 10 from +-0.05 three starts agree to 1e-12."""
import os

import numpy as np
import torch
from scipy.optimize import minimize

from tests import model_mpc_oracle as MO
from tests import model_rollout_oracle as R
from tests.golden_inputs import reset_law_obs
from tests import model_edge_inputs as E

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'model_mpc_ref.npz')
SETS = [('pt', R.PT, 20), ('pt', R.PT, 5), ('pd', R.PD, 25), ('pd', R.PD, 5), ('dp', R.DPEND, 10), ('dp', R.DPEND, 5)]
ROWS, ITERS, MIN_KEPT = 16, 200, 12


def key_of(tag, h):
    return '%s_h%d' % (tag, h)


def dp_narrow_obs(rng, n):
    """the double pendulum's start law narrowed: p, theta1, theta2 ~ U(-0.05, 0.05), velocities 0.05 N(0, 1), entries 8 .. 10 zero"""
    p, th = rng.uniform(-0.05, 0.05, n), rng.uniform(-0.05, 0.05, (n, 2))
    v = rng.standard_normal((n, 3)) * 0.05
    return np.concatenate([p[:, None], np.sin(th), np.cos(th), v, np.zeros((n, 3))], 1).astype(np.float32)


def start_rows(rng, env_id, n):
    if env_id == R.PT:
        return reset_law_obs(rng, n)
    return E.pendulum_wide_obs(rng, n) if env_id == R.PD else dp_narrow_obs(rng, n)


def lbfgsb(ocfg, obs_row, h, u0):
    def fun(x):
        c, g = MO.cost_and_grad(ocfg, obs_row[None], x.reshape(1, h, ocfg.act_dim))
        return float(c[0]), g.numpy().ravel().astype(np.float64)
    r = minimize(fun, u0.ravel(), jac=True, method='L-BFGS-B', bounds=[(-1., 1.)] * u0.size,
                 options=dict(maxiter=2000, maxfun=20000, ftol=1e-15, gtol=1e-12, maxcor=30))
    return r.fun, r.x.reshape(h, ocfg.act_dim)


def one_set(tag, env_id, h, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    ocfg = R.ocfg_of(env_id)
    obs0 = start_rows(rng, env_id, ROWS)
    ad = ocfg.act_dim
    best, u_best, agree = np.empty(ROWS), np.empty((ROWS, h, ad)), np.empty(ROWS, bool)
    for i in range(ROWS):
        runs = [lbfgsb(ocfg, obs0[i], h, u0) for u0 in (np.zeros((h, ad)), rng.uniform(-1, 1, (h, ad)), rng.uniform(-1, 1, (h, ad)))]
        costs = np.array([r[0] for r in runs])
        j = int(costs.argmin())
        best[i], u_best[i] = costs[j], runs[j][1]
        agree[i] = (costs.max() - costs.min()) <= 1e-9 * max(abs(costs.min()), 1e-300)
    u64, c64, _, info64 = MO.spg_solve(ocfg, obs0, horizon=h, iters=ITERS, dtype=torch.float64)
    u32, _, _, info32 = MO.spg_solve(ocfg, obs0, horizon=h, iters=ITERS, dtype=torch.float32)
    at32 = MO.horizon_cost(ocfg, obs0, u32.double()).numpy()
    c64 = c64.numpy()
    kept = agree & (np.abs(c64 - best) <= 1e-6 * np.maximum(best, 1.))
    print('%s: kept %d of %d (L-BFGS-B agree %d); float64 emulation gap max %.3g (kept rows), float32 emulation gap max %.3g; info64 %s'
          % (key_of(tag, h), kept.sum(), ROWS, agree.sum(), (c64 - best)[kept].max(), (at32 - best)[kept].max(), info64.tolist()))
    assert kept.sum() >= MIN_KEPT, (tag, h, int(kept.sum()))
    k = key_of(tag, h)
    return {'obs0_' + k: obs0, 'best_' + k: best, 'u_best_' + k: u_best, 'kept_' + k: kept, 'spg64_cost_' + k: c64,
            'spg32_u_' + k: u32.numpy(), 'spg32_gap_' + k: at32 - best}


if __name__ == '__main__':
    out = {}
    for n, (tag, env_id, h) in enumerate(SETS):
        out.update(one_set(tag, env_id, h, 8100 + n))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes')
