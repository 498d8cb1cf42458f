"""MPC on the learners' own models - what mpg_model_mpc_cost_grad and mpg_model_mpc_solve compute - restated on the oracles of the three
differentiable models (tests/model_rollout_oracle.model_of: PathTrackingModelOracle, InvertedPendulumModelOracle,
DoublePendulumModelOracle), in float32 or float64:

    horizon_cost(ocfg, obs0, u, eps)     model.reset(obs0) ONCE, then rollout_out per step on the carried state: cost = - sum of the raw
                                         rewards, t ascending (and the observations [B, H + 1, obs_dim], the rewards [B, H])
    cost_and_grad(ocfg, obs0, u, eps)    the cost and d cost / d u by autograd
    spg_minimize(fg, f, u0, ...)         the method include/mpg_hip.h fixes for mpg_mpc_solve and mpg_model_mpc_solve - spectral projected
                                         gradient, Birgin, Martinez and Raydan - statement by statement for a GENERIC cost
    spg_solve(ocfg, obs0, ...)           spg_minimize on horizon_cost; `dtype` float32 gives the float32 emulation the device's gap is
                                         measured against

A plain helper module shared by tests/test_model_mpc.py (CPU), tests/test_model_mpc_gpu.py and tests/golden/make_golden_model_mpc.py;
mpg_amd never imports it."""
import math

import numpy as np
import torch

from tests import model_rollout_oracle as R
from tests.mpc_oracle import SPG_ALPHA0, SPG_ALPHA_HI, SPG_ALPHA_LO, SPG_ALPHA_MAX_STEP, SPG_GAMMA, SPG_HALVINGS, SPG_M

PT, PD, DPEND = R.PT, R.PD, R.DPEND


def _t(x, dtype):
    return x.to(dtype) if torch.is_tensor(x) else torch.as_tensor(np.asarray(x)).to(dtype)


def horizon_cost(ocfg, obs0, u, eps=None, dtype=torch.float64, return_traj=False):
    """obs0 [B, obs_dim] start observations, u [B, H, act_dim] actions in the policy's range (taken as given), eps [H, B] standard normal
    or None (the noise terms at their means) -> cost [B]; with return_traj also obs_traj [B, H + 1, obs_dim] (row 0: obs0 as given) and
    rew_traj [B, H].  Tensors of `dtype`; differentiable in u."""
    obs0, u = _t(obs0, dtype), _t(u, dtype)
    m = R.model_of(ocfg)
    m.reset(obs0)
    cost = torch.zeros(obs0.shape[0], dtype=dtype)
    obs_l, rew_l = [obs0], []
    for t in range(u.shape[1]):
        e = torch.zeros(obs0.shape[0], dtype=dtype) if eps is None else _t(eps[t], dtype)
        o, r = m.rollout_out(u[:, t], e)
        cost = cost - r
        obs_l.append(o), rew_l.append(r)
    return (cost, torch.stack(obs_l, 1), torch.stack(rew_l, 1)) if return_traj else cost


def cost_and_grad(ocfg, obs0, u, eps=None, dtype=torch.float64):
    u = _t(u, dtype).detach().clone().requires_grad_(True)
    cost = horizon_cost(ocfg, obs0, u, eps, dtype)
    g, = torch.autograd.grad(cost.sum(), u)
    return cost.detach(), g


def _box(v):
    return torch.clamp(v, -1, 1)


def projected_gradient_norm(u, g):
    return (_box(u - g) - u).abs().flatten(1).amax(1)


def spg_minimize(fg, f_many, u0, iters=200, tol=0.):
    """The method of mpg_mpc_solve, statement by statement (include/mpg_hip.h), for any cost over the box [-1, 1]^n, in the dtype of u0
    [B, ...]:  fg(u) -> (cost [B], gradient like u);  f_many(t [k, B, ...]) -> cost [k, B] of k trial points per row (rows do not
    interact, so several lambdas are evaluated as one batch and each row takes its FIRST pass: the same arithmetic per row as one lambda
    at a time).  Returns (u, cost [B], pgnorm [B], info [B] int32)."""
    dtype, nb = u0.dtype, u0.shape[0]
    tail = (None,) * (u0.dim() - 1)
    u = _box(u0.clone())
    f, g = fg(u)
    pg = projected_gradient_norm(u, g)
    hist = torch.full((nb, SPG_M), -math.inf, dtype=dtype)
    hist[:, 0] = f
    alpha = torch.full((nb,), SPG_ALPHA0, dtype=dtype)
    accepted = torch.zeros(nb, dtype=torch.int32)
    failed = torch.zeros(nb, dtype=torch.bool)
    live = ~((pg <= tol) & (tol > 0))
    rows = torch.arange(nb)
    for _ in range(iters):
        if not live.any():
            break
        d = _box(u - alpha[(slice(None),) + tail] * g) - u
        gd = (g * d).flatten(1).sum(1)
        fmax = torch.where(torch.isnan(hist), torch.full_like(hist, -math.inf), hist).amax(1)
        searching = live.clone()
        trial, fnew = u.clone(), f.clone()
        for lo, hi in ((0, 3), (3, 9), (9, SPG_HALVINGS + 1)):
            if not searching.any():
                break
            lam = torch.tensor([0.5 ** h for h in range(lo, hi)], dtype=dtype)
            t = _box(u[None] + lam[(slice(None), None) + tail] * d[None])
            ft = f_many(t)
            ok = ft <= fmax[None] + SPG_GAMMA * lam[:, None] * gd[None]
            first = ok.to(torch.int8).argmax(0)
            take = searching & ok.any(0)
            trial[take], fnew[take] = t[first, rows][take], ft[first, rows][take]
            searching = searching & ~take
        failed |= live & searching
        live = live & ~searching
        if not live.any():
            break
        _, gt = fg(trial)
        s, y = trial - u, gt - g
        ss, sy = (s * s).flatten(1).sum(1), (s * y).flatten(1).sum(1)
        a = torch.where(sy > 0, ss / sy, torch.full_like(ss, SPG_ALPHA_MAX_STEP)).clamp(SPG_ALPHA_LO, SPG_ALPHA_HI)
        m = live
        u[m], g[m], f[m], alpha[m] = trial[m], gt[m], fnew[m], a[m]
        pg[m] = projected_gradient_norm(trial, gt)[m]
        hist[m] = torch.cat([fnew[m][:, None], hist[m][:, :-1]], 1)
        accepted[m] += 1
        live = live & ~((pg <= tol) & (tol > 0))
    info = torch.where(failed, -(accepted + 1), accepted)
    return u, f, pg, info


def spg_solve(ocfg, obs0, u_init=None, horizon=25, iters=200, tol=0., eps=None, dtype=torch.float64):
    """spg_minimize on horizon_cost from u_init (None: zeros).  Returns (u [B, H, act_dim], cost [B], pgnorm [B], info [B])."""
    obs0 = _t(obs0, dtype)
    nb = obs0.shape[0]
    u0 = torch.zeros(nb, horizon, ocfg.act_dim, dtype=dtype) if u_init is None else _t(u_init, dtype).reshape(nb, horizon, ocfg.act_dim)
    e = None if eps is None else _t(eps, dtype)

    def f_many(t):
        k = t.shape[0]
        with torch.no_grad():
            return horizon_cost(ocfg, obs0.repeat(k, 1), t.reshape(k * nb, horizon, ocfg.act_dim), None if e is None else e.repeat(1, k),
                                dtype).reshape(k, nb)

    return spg_minimize(lambda u: cost_and_grad(ocfg, obs0, u, e, dtype), f_many, u0, iters, tol)
