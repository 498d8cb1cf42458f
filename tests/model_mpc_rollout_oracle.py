"""MPC's closed loop on the learners' models, restated (mpg_model_mpc_rollout; include/mpg_hip.h writes the chain out): per step one
tests/model_mpc_oracle.spg_solve from the current row at the noise means, then the plant's step as the one-step horizon cost
(horizon_cost(H = 1, return_traj=True)) with the plan's first action under the plant's own noise; row 1 of that record is the next row.
float32 or float64 (`dtype`); rows in, rows out as numpy arrays of that precision."""
import numpy as np
import torch

from tests import model_mpc_oracle as MO

NP = {torch.float32: np.float32, torch.float64: np.float64}


def shifted(plan):
    """the plan one action later, its last action repeated"""
    return np.concatenate([plan[:, 1:], plan[:, -1:]], 1)


def plant_step(ocfg, obs, act, eps=None, dtype=torch.float64):
    """one model step in mpg_model_step's row format: obs [n, obs_dim], act [n, act_dim], eps [n] or None -> (next row, raw reward)"""
    e = None if eps is None else np.asarray(eps)[None, :]
    _, rec, rew = MO.horizon_cost(ocfg, obs, np.asarray(act)[:, None, :], e, dtype, return_traj=True)
    return rec[:, 1].detach().numpy(), rew[:, 0].detach().numpy()


def closed_loop(ocfg, obs, u, steps, iters=200, tol=0., warm_start=False, eps=None, dtype=torch.float64):
    """obs [n, obs_dim], u [n, H, act_dim] the first solve's start point, eps [steps, n] the PLANT's noise or None -> a dict of obs_traj
    [steps, n, obs_dim], plan_traj [steps, n, H, act_dim], rew_traj, cost_traj, pgnorm_traj [steps, n], info_traj [steps, n] int32,
    last_obs [n, obs_dim], u_next [n, H, act_dim]"""
    obs, u = np.asarray(obs).astype(NP[dtype]), np.asarray(u).astype(NP[dtype])
    keys = ('obs_traj', 'plan_traj', 'rew_traj', 'cost_traj', 'pgnorm_traj', 'info_traj')
    rec = {k: [] for k in keys}
    for t in range(steps):
        plan, cost, pg, info = (x.numpy() for x in MO.spg_solve(ocfg, obs, u, u.shape[1], iters, tol, None, dtype))
        if warm_start:
            u = shifted(plan)
        nxt, rew = plant_step(ocfg, obs, plan[:, 0], None if eps is None else eps[t], dtype)
        for k, v in zip(keys, (obs, plan, rew, cost, pg, info)):
            rec[k].append(v)
        obs = nxt
    out = {k: np.stack(v) for k, v in rec.items()}
    out.update(last_obs=obs, u_next=u)
    return out
