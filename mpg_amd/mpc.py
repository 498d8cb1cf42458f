"""The reference's MPC baseline, SLSQP form (mpc/main.py), on the device: the horizon cost, its gradient and a batched solver, and the
closed loop that measures a policy against it.  Names follow the reference.

Where mpc/main.py runs one scipy SLSQP solve with finite-difference gradients per env step (about 2 s each), ModelPredictiveControl
here holds B start states and solves all of them in ONE launch (mpg_mpc_solve: spectral projected gradient on the hand adjoint of the
25-step rollout; include/mpg_hip.h states the problem, the method and its constants).  The IPOPT form (mpc/mpc_ipopt.py) needs casadi
and is not provided."""
import torch

from . import _lib as L
from .envs import PathTrackingEnv

MAX_HORIZON, MAX_ITERS = 31, 1000        # MPG_MPC_MAX_HORIZON, MPG_MPC_MAX_ITERS


def _f32(t):
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.to(torch.float32).contiguous()


def mpc_cost_grad(x0, u, want_grad=True, want_traj=False):
    """mpg_mpc_cost_grad: x0 [B, 6], u [B, H, 2] -> (cost [B], grad [B, H, 2] or None, traj [B, H + 1, 6] or None), one launch"""
    rows, horizon = u.shape[0], u.shape[1]
    assert x0.shape == (rows, 6) and u.shape == (rows, horizon, 2), (x0.shape, u.shape)
    cost = torch.empty(rows, dtype=torch.float32, device=x0.device)
    grad = torch.empty(rows, horizon, 2, dtype=torch.float32, device=x0.device) if want_grad else None
    traj = torch.empty(rows, horizon + 1, 6, dtype=torch.float32, device=x0.device) if want_traj else None
    L.call('mpg_mpc_cost_grad', L.c_int(rows), L.c_int(horizon), L.ptr(_f32(x0)), L.ptr(_f32(u)), L.ptr(cost), L.ptr(grad), L.ptr(traj),
           L.stream())
    return cost, grad, traj


def mpc_solve(x0, u_init, iters=200, tol=0.):
    """mpg_mpc_solve: x0 [B, 6], u_init [B, H, 2] (left as it is) -> (u [B, H, 2], cost [B], pgnorm [B], info [B] int32), one launch"""
    rows, horizon = u_init.shape[0], u_init.shape[1]
    assert x0.shape == (rows, 6) and u_init.shape == (rows, horizon, 2), (x0.shape, u_init.shape)
    u = u_init.to(torch.float32).contiguous().clone()
    cost = torch.empty(rows, dtype=torch.float32, device=x0.device)
    pgnorm = torch.empty(rows, dtype=torch.float32, device=x0.device)
    info = torch.empty(rows, dtype=torch.int32, device=x0.device)
    L.call('mpg_mpc_solve', L.c_int(rows), L.c_int(horizon), L.c_int(int(iters)), L.c_float(float(tol)), L.ptr(_f32(x0)), L.ptr(u),
           L.ptr(cost), L.ptr(pgnorm), L.ptr(info), L.stream())
    return u, cost, pgnorm, info


class ModelPredictiveControl(object):
    """mpc/main.py:111-165.  init_x: [6] or [B, 6] on the device, [v_x, v_y, r, delta_y, delta_phi, x] with entry 0 the speed in m/s
    (compute_rew :133 reads it against expected_vs = 20).  Controls are normalised, [horizon, 2] (flat accepted) or [B, horizon, 2]."""

    def __init__(self, init_x, horizon):
        self.horizon = int(horizon)
        self.base_frequency = 10.
        self.num_future_data = 0
        self.expected_vs = 20.
        self.reset_init_x(init_x)

    def reset_init_x(self, init_x):
        self.single = init_x.dim() == 1
        self.init_x = _f32(init_x.reshape(-1, 6))

    def _u(self, u):
        return _f32(u.to(self.init_x.device).reshape(self.init_x.shape[0], self.horizon, 2))

    def cost_function(self, u):
        """:156-165.  A Python float for one row (as the reference returns; this reads the device), a tensor [B] for a batch."""
        cost = mpc_cost_grad(self.init_x, self._u(u), want_grad=False)[0]
        return float(cost[0]) if self.single else cost

    def cost_and_gradient(self, u):
        """(cost, d cost / d u) with respect to the normalised controls, in the shape of u; tensors in both forms"""
        cost, grad, _ = mpc_cost_grad(self.init_x, self._u(u))
        return (cost[0], grad[0].reshape(u.shape)) if self.single else (cost, grad.reshape(u.shape))

    def solve(self, u_init=None, iters=200, tol=0.0):
        """minimise over [-1, 1]^(2 horizon) from u_init (zeros, main.py:184) -> (u, cost, pgnorm, info); info: the accepted iterations,
        negative for a row whose line search failed.  Tensors [B, ...]; for one row u is [horizon, 2] and the rest are 0-d tensors."""
        rows = self.init_x.shape[0]
        u0 = torch.zeros(rows, self.horizon, 2, dtype=torch.float32, device=self.init_x.device) if u_init is None else self._u(u_init)
        u, cost, pgnorm, info = mpc_solve(self.init_x, u0, iters, tol)
        return (u[0], cost[0], pgnorm[0], info[0]) if self.single else (u, cost, pgnorm, info)


def run_mpc(policy, num_agent=1, steps=90, horizon=25, seed=0, iters=200, device='cuda'):
    """The closed loop of mpc/main.py:168-223 for `num_agent` start states at once: two PathTrackingEnv (num_future_data 0) from the same
    start, one driven by the first control pair of a fresh MPC solve per step (from zeros, :184), one by `policy` (PolicyWithQs), and the
    policy's action on the MPC env's observations beside them.

    The solve starts from the MPC env's observation with 20 ADDED to column 0.  main.py:185,221 hands the observation over as it is, and
    its cost reads column 0 as the speed against expected_vs = 20 (:133); that fits the env its recording mpc/mpc_rl.npy was made with,
    whose column 0 was the speed - today's PathTrackingEnv (and this project's) returns v_x - 20, which is why the fixture made from
    that recording subtracts 20 from it ("subtract 20 from obs[0]").  Unshifted, the baseline would drive to 40 m/s.

    Returns the reference's record keys as stacked device tensors over the steps: mpc_obs, rl_obs [steps, n, 6], mpc_action [steps, n,
    horizon, 2] (the whole plan), rl_action, rl_action_mpc [steps, n, 2], mpc_rew, rl_rew [steps, n] (the reward that led to the recorded
    observation: zeros first).  Nothing in the loop synchronises or copies to the host, so timing is the caller's: synchronise around the
    call."""
    env4mpc = PathTrackingEnv(num_future_data=0, num_agent=num_agent, device=device, seed=seed)
    env4rl = PathTrackingEnv(num_future_data=0, num_agent=num_agent, device=device, seed=seed)
    obs = env4mpc.reset()
    obs4rl = env4rl.reset(init_obs=obs.clone())
    shift = torch.zeros(6, dtype=torch.float32, device=obs.device)
    shift[0] = 20.
    mpc = ModelPredictiveControl(obs + shift, horizon)
    rew = torch.zeros(num_agent, dtype=torch.float32, device=obs.device)
    rew4rl = torch.zeros_like(rew)
    keys = ('mpc_obs', 'rl_obs', 'mpc_action', 'rl_action', 'rl_action_mpc', 'mpc_rew', 'rl_rew')
    rec = {k: [] for k in keys}
    for _ in range(steps):
        mpc_action = mpc.solve(iters=iters)[0]
        rl_action_mpc = policy.compute_action(obs)[0]
        rl_action = policy.compute_action(obs4rl)[0]
        for k, v in zip(keys, (obs, obs4rl, mpc_action, rl_action, rl_action_mpc, rew, rew4rl)):
            rec[k].append(v)
        obs, rew, _, _ = env4mpc.step(mpc_action[:, 0, :].contiguous())
        obs4rl, rew4rl, _, _ = env4rl.step(rl_action)
        mpc.reset_init_x(obs + shift)
    return {k: torch.stack(v) for k, v in rec.items()}
