"""The MPC baseline of the reference (mpc/main.py, SLSQP form) restated in torch, for the tests of mpg_mpc_cost_grad / mpg_mpc_solve:

    horizon_cost(x0, u)             ModelPredictiveControl.cost_function (:156-165) for a batch, operator by operator in the reference's
                                    order (float64 by default: tests/golden/mpc_ref.npz pins it to the reference's own values)
    cost_and_grad(x0, u)            the cost and d cost / d u (normalised controls) by autograd
    cost_and_grad_adjoint(x0, u)    the same by the hand adjoint of the step, without a graph (pinned to autograd by the tests)
    spg_solve(x0, ...)              the solver include/mpg_hip.h fixes for mpg_mpc_solve - spectral projected gradient, Birgin, Martinez
                                    and Raydan - as plain batched torch; `dtype` float32 gives the float32 emulation the device's gap is
                                    measured against

Nothing here is used by the product (mpg_amd/mpc.py calls the library)."""
import math

import torch

# mpc/main.py:60-67, :116-118, :161
C_f, C_r, A, B, MASS, I_z = -128915.5, -85943.6, 1.06, 1.85, 1412., 1536.7
TAU = 1 / 10.
EXPECTED_VS = 20.
STEER_SCALE, ACC_SCALE = 0.4, 3.
# include/mpg_hip.h, MPG_MPC_SPG_*
SPG_M, SPG_HALVINGS, SPG_GAMMA = 5, 20, 1e-4
SPG_ALPHA0, SPG_ALPHA_MAX_STEP, SPG_ALPHA_LO, SPG_ALPHA_HI = 0.05, 10., 1e-6, 1e3


def next_state(x, steer, a_x):
    """compute_next_obses (:145-154): f_xu (:75-104) at tau = 0.1, v_x clipped to [1, 35], delta_phi wrapped once.  x: six [B] tensors."""
    v_x, v_y, r, y, phi, xx = x
    tau = TAU
    n_vx = v_x + tau * (a_x + v_y * r)
    n_vy = (MASS * v_y * v_x + tau * (A * C_f - B * C_r) * r - tau * C_f * steer * v_x - tau * MASS * torch.square(v_x) * r) / \
        (MASS * v_x - tau * (C_f + C_r))
    n_r = (-I_z * r * v_x - tau * (A * C_f - B * C_r) * v_y + tau * A * C_f * steer * v_x) / (tau * (A ** 2 * C_f + B ** 2 * C_r) - I_z * v_x)
    n_y = y + tau * (v_x * torch.sin(phi) + v_y * torch.cos(phi))
    n_phi = phi + tau * r
    n_x = xx + tau * (v_x * torch.cos(phi) - v_y * torch.sin(phi))
    n_vx = torch.clamp(n_vx, 1, 35)
    n_phi = torch.where(n_phi > math.pi, n_phi - 2 * math.pi, n_phi)
    n_phi = torch.where(n_phi <= -math.pi, n_phi + 2 * math.pi, n_phi)
    return [n_vx, n_vy, n_r, n_y, n_phi, n_x]


def horizon_cost(x0, u, control_penalty=True, return_traj=False):
    """x0 [B, 6] (entry 0 the speed in m/s), u [B, H, 2] normalised -> cost [B] (and the states [B, H + 1, 6]).  control_penalty False
    leaves 5 steer^2 + 0.05 a_x^2 out: what is left of a control's gradient then reached the cost through the model alone."""
    x = [x0[:, k] for k in range(6)]
    loss = torch.zeros_like(x0[:, 0])
    traj = [torch.stack(x, 1)]
    for i in range(u.shape[1]):
        steer, a_x = u[:, i, 0] * STEER_SCALE, u[:, i, 1] * ACC_SCALE
        # compute_rew :133-141 (the reference subtracts the sum of the negated squares)
        rew = 0.01 * torch.square(x[0] - EXPECTED_VS) + 0.04 * torch.square(x[3]) + 0.1 * torch.square(x[4]) + 0.02 * torch.square(x[2])
        if control_penalty:
            rew = rew + 5 * torch.square(steer) + 0.05 * torch.square(a_x)
        loss = loss + rew
        x = next_state(x, steer, a_x)
        if return_traj:
            traj.append(torch.stack(x, 1))
    return (loss, torch.stack(traj, 1)) if return_traj else loss


def cost_and_grad(x0, u, control_penalty=True):
    u = u.detach().clone().requires_grad_(True)
    cost = horizon_cost(x0, u, control_penalty)
    g, = torch.autograd.grad(cost.sum(), u)
    return cost.detach(), g


def cost_and_grad_adjoint(x0, u):
    """cost_and_grad by the hand adjoint of the step - the formulas of the kernel (and of rollout::PathTracking::vjp), in the dtype of the
    inputs, without a graph: what spg_solve iterates on, a third of autograd's time.  tests/test_mpc_golden.py pins it to cost_and_grad."""
    with torch.no_grad():
        H = u.shape[1]
        K1, K2, K3, K4 = TAU * (A * C_f - B * C_r), TAU * C_f, TAU * MASS, TAU * (C_f + C_r)
        K5, K6 = TAU * A * C_f, TAU * (A ** 2 * C_f + B ** 2 * C_r)
        x = [x0[:, k] for k in range(6)]
        states, loss = [], torch.zeros_like(x0[:, 0])
        for i in range(H):
            steer, a_x = u[:, i, 0] * STEER_SCALE, u[:, i, 1] * ACC_SCALE
            states.append(x)
            loss = loss + (0.01 * torch.square(x[0] - EXPECTED_VS) + 0.04 * torch.square(x[3]) + 0.1 * torch.square(x[4]) +
                           0.02 * torch.square(x[2]) + 5 * torch.square(steer) + 0.05 * torch.square(a_x))
            x = next_state(x, steer, a_x)
        g = torch.empty_like(u)
        zero = torch.zeros_like(loss)
        l_vx_in, l_vy, l_r, l_dy, l_dphi = zero, zero, zero, zero, zero
        for i in range(H - 1, -1, -1):
            vx, vy, r, dy, dphi, _ = states[i]
            de, ax = u[:, i, 0] * STEER_SCALE, u[:, i, 1] * ACC_SCALE
            raw = vx + TAU * (ax + vy * r)
            l_vx = torch.where((raw >= 1) & (raw <= 35), l_vx_in, zero)
            iD1, iD2 = 1 / (MASS * vx - K4), 1 / (K6 - I_z * vx)
            nvy = (MASS * vy * vx + K1 * r - K2 * de * vx - K3 * vx * vx * r) * iD1
            nr = (-I_z * r * vx - K1 * vy + K5 * de * vx) * iD2
            sp, cp = torch.sin(dphi), torch.cos(dphi)
            dvy_vx = (MASS * vy - K2 * de - 2 * K3 * vx * r - nvy * MASS) * iD1
            dr_vx = (-I_z * r + K5 * de + nr * I_z) * iD2
            g[:, i, 1] = (l_vx * TAU + 0.1 * ax) * ACC_SCALE
            g[:, i, 0] = (l_vy * (-K2 * vx * iD1) + l_r * (K5 * vx * iD2) + 10 * de) * STEER_SCALE
            g_vx = l_vx + l_vy * dvy_vx + l_r * dr_vx + l_dy * TAU * sp + 0.02 * (vx - EXPECTED_VS)
            g_vy = l_vx * TAU * r + l_vy * (MASS * vx * iD1) + l_r * (-K1 * iD2) + l_dy * TAU * cp
            g_r = l_vx * TAU * vy + l_vy * ((K1 - K3 * vx * vx) * iD1) + l_r * (-I_z * vx * iD2) + l_dphi * TAU + 0.04 * r
            g_dphi = l_dphi + l_dy * TAU * (vx * cp - vy * sp) + 0.2 * dphi
            g_dy = l_dy + 0.08 * dy
            l_vx_in, l_vy, l_r, l_dy, l_dphi = g_vx, g_vy, g_r, g_dy, g_dphi
        return loss, g


def _box(v):
    return torch.clamp(v, -1, 1)


def projected_gradient_norm(u, g):
    return (_box(u - g) - u).abs().flatten(1).amax(1)


def spg_solve(x0, u_init=None, horizon=25, iters=200, tol=0., dtype=torch.float64):
    """The method of mpg_mpc_solve, statement by statement (include/mpg_hip.h).  Returns (u [B, H, 2], cost [B], pgnorm [B], info [B])."""
    x0 = torch.as_tensor(x0).to(dtype)
    nb = x0.shape[0]
    u = _box(torch.zeros(nb, horizon, 2, dtype=dtype) if u_init is None else torch.as_tensor(u_init).to(dtype).reshape(nb, horizon, 2).clone())
    f, g = cost_and_grad_adjoint(x0, u)
    pg = projected_gradient_norm(u, g)
    hist = torch.full((nb, SPG_M), -math.inf, dtype=dtype)
    hist[:, 0] = f
    alpha = torch.full((nb,), SPG_ALPHA0, dtype=dtype)
    accepted = torch.zeros(nb, dtype=torch.int32)
    failed = torch.zeros(nb, dtype=torch.bool)
    live = ~((pg <= tol) & (tol > 0))
    for _ in range(iters):
        if not live.any():
            break
        d = _box(u - alpha[:, None, None] * g) - u
        gd = (g * d).flatten(1).sum(1)
        fmax = torch.where(torch.isnan(hist), torch.full_like(hist, -math.inf), hist).amax(1)
        searching = live.clone()
        trial, fnew = u.clone(), f.clone()
        # lambda = 1, 1/2, ...: a row takes the FIRST one that passes.  Rows do not interact, so several lambdas are evaluated as one
        # batch (a chunk of them at a time) and each row picks its first pass: the same arithmetic per row as one lambda at a time
        for lo, hi in ((0, 3), (3, 9), (9, SPG_HALVINGS + 1)):
            if not searching.any():
                break
            lam = torch.tensor([0.5 ** h for h in range(lo, hi)], dtype=dtype)[:, None]          # [k, 1]
            t = _box(u[None] + lam[:, :, None, None] * d[None])                                  # [k, B, H, 2]
            with torch.no_grad():
                ft = horizon_cost(x0.repeat(hi - lo, 1), t.reshape(-1, horizon, 2)).reshape(hi - lo, nb)
            ok = ft <= fmax[None] + SPG_GAMMA * lam * gd[None]                                   # [k, B]
            first = ok.to(torch.int8).argmax(0)                                                  # the first pass of each row
            take = searching & ok.any(0)
            rows = torch.arange(nb)
            trial[take], fnew[take] = t[first, rows][take], ft[first, rows][take]
            searching = searching & ~take
        failed |= live & searching
        live = live & ~searching
        if not live.any():
            break
        _, gt = cost_and_grad_adjoint(x0, trial)
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
