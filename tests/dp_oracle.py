"""Restatement of the reference's InvertedDoublePendulum-v2 model, of the closed-form adjoint the HIP reverse sweep implements, and of
NADP on that model, in torch on the CPU (float32 / float64), op by op with the reference's line numbers
(envs_and_models/inverted_double_pendulum_model.py, learners/nadp.py).  Used by the tests only; mpg_amd never imports it.

The model has no noise: `eps` arguments exist for the shape of the oracle's interfaces and are ignored."""
import numpy as np
import torch

from oracle import mpg_oracle as O

ENV_ID = 'InvertedDoublePendulum-v2'
# Dynamics.__init__, :16-24
M_CART, M_ROD1, M_ROD2, L_ROD1, L_ROD2, GRAV = 9.42477796, 4.1033127, 4.1033127, 0.6, 0.6, 9.81
TAU, N_SUB, U_SCALE = 0.01, 5, 500.


def _consts(dt):
    """tf.constant(..., dtype=tf.float32) of :27-34: the run's dtype (the float64 run of the reference carries them as doubles)"""
    return [torch.tensor(v, dtype=dt) for v in (M_CART, M_ROD1, M_ROD2, L_ROD1, L_ROD2, GRAV)]


def f_xu_old(states, u, tau):
    """Dynamics.f_xu_old, :26-53 (damping 0: the three damping terms of :43-45 are exact zeros)."""
    dt = states.dtype
    m, m1, m2, l1, l2, g = _consts(dt)
    p, th1, th2, pd, th1d, th2d = [states[:, i] for i in range(6)]
    ones = torch.ones_like(p)
    M = torch.stack([(m + m1 + m2) * ones, l1 * (m1 + m2) * torch.cos(th1), m2 * l2 * torch.cos(th2),
                     l1 * (m1 + m2) * torch.cos(th1), torch.square(l1) * (m1 + m2) * ones, l1 * l2 * m2 * torch.cos(th1 - th2),
                     l2 * m2 * torch.cos(th2), l1 * l2 * m2 * torch.cos(th1 - th2), torch.square(l2) * m2 * ones], 1).reshape(-1, 3, 3)   # :39-42
    f = torch.stack([l1 * (m1 + m2) * torch.square(th1d) * torch.sin(th1) + m2 * l2 * torch.square(th2d) * torch.sin(th2) - 0. * pd + u,
                     -l1 * l2 * m2 * torch.square(th2d) * torch.sin(th1 - th2) + g * (m1 + m2) * l1 * torch.sin(th1) - 0. * th1d,
                     l1 * l2 * m2 * torch.square(th1d) * torch.sin(th1 - th2) + g * l2 * m2 * torch.sin(th2)], 1).reshape(-1, 3, 1)        # :43-46
    tmp = torch.matmul(torch.linalg.inv(M), f).squeeze(-1)                                                                            # :47-48
    deriv = torch.cat([states[:, 3:], tmp], -1)                                                                                       # :50
    return states + tau * deriv                                                                                                       # :51


def compute_rewards(states):
    """Dynamics.compute_rewards, :89-100"""
    p, th1, th2, pd, th1d, th2d = [states[:, i] for i in range(6)]
    tip_x = p + L_ROD1 * torch.sin(th1) + L_ROD2 * torch.sin(th2)
    tip_y = L_ROD1 * torch.cos(th1) + L_ROD2 * torch.cos(th2)
    dist_penalty = 0.01 * torch.square(tip_x) + torch.square(tip_y - 2)
    vel_penalty = 1e-3 * torch.square(th1d) + 5e-3 * torch.square(th2d)
    return -dist_penalty - vel_penalty


def get_obs(states):
    """_get_obs, :118-124"""
    p, th1, th2, pd, th1d, th2d = [states[:, i] for i in range(6)]
    z = torch.zeros_like(p)
    return torch.stack([p, torch.sin(th1), torch.sin(th2), torch.cos(th1), torch.cos(th2), pd, th1d, th2d, z, z, z], 1)


def get_state(obses):
    """_get_state, :126-132"""
    return torch.stack([obses[:, 0], torch.atan2(obses[:, 1], obses[:, 3]), torch.atan2(obses[:, 2], obses[:, 4]),
                        obses[:, 5], obses[:, 6], obses[:, 7]], 1)


class DoublePendulumModelOracle(object):
    """InvertedDoublePendulumModel, :103-144"""
    obs_dim, act_dim = 11, 1

    def reset(self, obses):                                                   # :114-116
        self.obses = obses
        self.states = get_state(obses)

    def rollout_out(self, actions, eps=None):                                 # :134-141
        u = (torch.tensor(U_SCALE, dtype=actions.dtype) * actions)[:, 0]      # :143-144
        for _ in range(N_SUB):
            self.states = f_xu_old(self.states, u, TAU)
            self.obses = get_obs(self.states)
        return self.obses, compute_rewards(self.states)


def make_cfg(n=25, **kw):
    """the oracle's Cfg with this project's defaults for the env (mpg_amd.ops.make_cfg; the reference ships no parser for it)"""
    c = O.Cfg('InvertedPendulumConti-v0')
    c.env = ENV_ID
    c.obs_dim, c.act_dim = 11, 1
    c.obs_scale = [1.] * 11
    c.rew_scale, c.rew_shift = 1., 0.
    c.policy_out_act, c.action_range = 'linear', 1.
    c.n, c.select, c.delay_update = n, [0, n], 1
    c.__dict__.update(kw)
    return c


# ---- the closed-form solve and adjoint of the kernel (csrc/rollout_common.h DoublePendulum), float64 numpy --------------------
_A = M_CART + M_ROD1 + M_ROD2
_B = L_ROD1 * (M_ROD1 + M_ROD2)
_C = M_ROD2 * L_ROD2
_D = L_ROD1 ** 2 * (M_ROD1 + M_ROD2)
_E = L_ROD1 * L_ROD2 * M_ROD2
_F = L_ROD2 ** 2 * M_ROD2
_G1 = GRAV * (M_ROD1 + M_ROD2) * L_ROD1
_G2 = GRAV * L_ROD2 * M_ROD2


def _setup(t1, t2):
    s1, c1, s2, c2 = np.sin(t1), np.cos(t1), np.sin(t2), np.cos(t2)
    c12, s12 = c1 * c2 + s1 * s2, s1 * c2 - c1 * s2
    x, y, z = _B * c1, _C * c2, _E * c12
    a00, a01, a02 = _D * _F - z * z, y * z - x * _F, x * z - _D * y
    a11, a12, a22 = _A * _F - y * y, x * y - _A * z, _A * _D - x * x
    idet = 1. / (_A * a00 + x * a01 + y * a02)
    inv = [a00 * idet, a01 * idet, a02 * idet, a11 * idet, a12 * idet, a22 * idet]       # i00 i01 i02 i11 i12 i22
    return (s1, c1, s2, c2, s12, c12), inv


def _accel(trig, inv, s, u):
    s1, c1, s2, c2, s12, c12 = trig
    i00, i01, i02, i11, i12, i22 = inv
    w1s, w2s = s[:, 4] ** 2, s[:, 5] ** 2
    f0 = _B * w1s * s1 + _C * w2s * s2 + u
    f1 = -_E * w2s * s12 + _G1 * s1
    f2 = _E * w1s * s12 + _G2 * s2
    return [i00 * f0 + i01 * f1 + i02 * f2, i01 * f0 + i11 * f1 + i12 * f2, i02 * f0 + i12 * f1 + i22 * f2]


def dp_substep(s, u):
    trig, inv = _setup(s[:, 1], s[:, 2])
    q = _accel(trig, inv, s, u)
    out = s.copy()
    out[:, :3] = s[:, :3] + TAU * s[:, 3:]
    for i in range(3):
        out[:, 3 + i] = s[:, 3 + i] + TAU * q[i]
    return out


def dp_model_step(s, a):
    """forward step of the kernel (closed-form solve): new state, reward"""
    u = U_SCALE * a[:, 0]
    for _ in range(N_SUB):
        s = dp_substep(s, u)
    tx = s[:, 0] + L_ROD1 * np.sin(s[:, 1]) + L_ROD2 * np.sin(s[:, 2])
    ty = L_ROD1 * np.cos(s[:, 1]) + L_ROD2 * np.cos(s[:, 2])
    return s, -(0.01 * tx ** 2 + (ty - 2.) ** 2) - (1e-3 * s[:, 4] ** 2 + 5e-3 * s[:, 5] ** 2)


def dp_model_step_vjp(s0, a, lam_new, rho):
    """DoublePendulum::vjp: lam_new = dL/d(new state) [N, 6], rho = dL/d(reward) [N] -> dL/d(state) [N, 6], dL/d(action) [N, 1]"""
    u = U_SCALE * a[:, 0]
    states = [s0]
    for _ in range(N_SUB):
        states.append(dp_substep(states[-1], u))
    on = states[-1]
    s1, c1, s2, c2 = np.sin(on[:, 1]), np.cos(on[:, 1]), np.sin(on[:, 2]), np.cos(on[:, 2])
    tx, ty = on[:, 0] + L_ROD1 * s1 + L_ROD2 * s2, L_ROD1 * c1 + L_ROD2 * c2
    dx, dy = -0.02 * tx, -2. * (ty - 2.)
    lam = lam_new.copy()
    lam[:, 0] += rho * dx
    lam[:, 1] += rho * (dx * L_ROD1 * c1 - dy * L_ROD1 * s1)
    lam[:, 2] += rho * (dx * L_ROD2 * c2 - dy * L_ROD2 * s2)
    lam[:, 4] += rho * (-2e-3 * on[:, 4])
    lam[:, 5] += rho * (-1e-2 * on[:, 5])
    gu = np.zeros_like(u)
    for k in range(N_SUB - 1, -1, -1):
        s = states[k]
        trig, inv = _setup(s[:, 1], s[:, 2])
        s1, c1, s2, c2, s12, c12 = trig
        i00, i01, i02, i11, i12, i22 = inv
        q = _accel(trig, inv, s, u)
        w1, w2 = s[:, 4], s[:, 5]
        m0, m1, m2 = TAU * lam[:, 3], TAU * lam[:, 4], TAU * lam[:, 5]
        z0 = i00 * m0 + i01 * m1 + i02 * m2
        z1 = i01 * m0 + i11 * m1 + i12 * m2
        z2 = i02 * m0 + i12 * m1 + i22 * m2
        k01, k02, k12 = z0 * q[1] + z1 * q[0], z0 * q[2] + z2 * q[0], z1 * q[2] + z2 * q[1]
        g_t1 = k01 * _B * s1 + k12 * _E * s12 + z0 * (_B * w1 * w1 * c1) + z1 * (-_E * w2 * w2 * c12 + _G1 * c1) + z2 * (_E * w1 * w1 * c12)
        g_t2 = k02 * _C * s2 - k12 * _E * s12 + z0 * (_C * w2 * w2 * c2) + z1 * (_E * w2 * w2 * c12) + z2 * (-_E * w1 * w1 * c12 + _G2 * c2)
        g_w1 = z0 * (2. * _B * w1 * s1) + z2 * (2. * _E * w1 * s12)
        g_w2 = z0 * (2. * _C * w2 * s2) - z1 * (2. * _E * w2 * s12)
        gu += z0
        new = lam.copy()
        new[:, 3] = lam[:, 3] + TAU * lam[:, 0]
        new[:, 4] = lam[:, 4] + TAU * lam[:, 1] + g_w1
        new[:, 5] = lam[:, 5] + TAU * lam[:, 2] + g_w2
        new[:, 1] = lam[:, 1] + g_t1
        new[:, 2] = lam[:, 2] + g_t2
        lam = new
    return lam, (U_SCALE * gu)[:, None]


def feature_vjp(s, v, scale):
    """DoublePendulum::fold: J^T (v * scale) of the 11 features of the state s; v [N, >= 8]"""
    s1, c1, s2, c2 = np.sin(s[:, 1]), np.cos(s[:, 1]), np.sin(s[:, 2]), np.cos(s[:, 2])
    v = v * np.asarray(scale)[None, :v.shape[1]]
    return np.stack([v[:, 0], v[:, 1] * c1 - v[:, 3] * s1, v[:, 2] * c2 - v[:, 4] * s2, v[:, 5], v[:, 6], v[:, 7]], 1)


# ---- NADP on the model (learners/nadp.py) -----------------------------------------------------------------------------------
def rollout_q_estimation(cfg, nets, start_obses, start_actions, select, M=1, target='Q1_target'):
    """NADPLearner.model_rollout_for_q_estimation, nadp.py:87-126 -> [len(select) * B], no gradient"""
    dt = nets.dtype
    with torch.no_grad():
        obses, a = start_obses.repeat(M, 1), start_actions.repeat(M, 1)
        po = O.process_obses(cfg, obses)
        po_list, a_list = [po], [a]
        rsum = torch.zeros(obses.shape[0], dtype=dt)
        rsum_list, gam_list = [rsum], [torch.ones(obses.shape[0], dtype=dt)]
        model = DoublePendulumModelOracle()
        model.reset(obses)                                                   # :98
        n = max(select)
        for ri in range(n):
            obses, rew = model.rollout_out(a)                               # :102
            po = O.process_obses(cfg, obses)
            rsum = rsum + O.tf_pow(cfg.gamma, ri, dt) * O.process_rewards(cfg, rew)      # :105
            rsum_list.append(rsum)
            a = nets.compute_action(po)                                      # :107
            po_list.append(po), a_list.append(a)
            gam_list.append(O.tf_pow(cfg.gamma, ri + 1, dt) * torch.ones(obses.shape[0], dtype=dt))
        all_q = nets.q(target, torch.cat(po_list, 0), torch.cat(a_list, 0))  # :113-114
        final = (torch.cat(rsum_list, 0) + torch.cat(gam_list, 0) * all_q).reshape(n + 1, M, -1)
        returns = final.mean(1)                                              # :119-120
        return torch.cat([returns[k] for k in select], 0), model.states


def rollout_policy_update(cfg, nets, start_obses, n, M=1, all_steps_param_grad=True):
    """NADPLearner.model_rollout_for_policy_update, nadp.py:128-171: every step through pi_theta -> reduced returns [n + 1].
    all_steps_param_grad=False: steps 1..n use a VALUE copy of the policy (mpg_learner.py:422, the MPG form the rollout entry point
    also serves): same numbers, the parameter gradient flows through the first evaluation only."""
    dt = nets.dtype
    obses = start_obses.repeat(M, 1)
    po = O.process_obses(cfg, obses)
    a = nets.compute_action(po)                                              # :133
    po_list, a_list = [po], [a]
    rsum = torch.zeros(obses.shape[0], dtype=dt)
    rsum_list, gam_list = [rsum], [torch.ones(obses.shape[0], dtype=dt)]
    model = DoublePendulumModelOracle()
    model.reset(obses)                                                       # :141
    w_roll = [w.detach() for w in nets.w['policy']]
    for ri in range(n):
        obses, rew = model.rollout_out(a)                                    # :144
        po = O.process_obses(cfg, obses)
        rsum = rsum + O.tf_pow(cfg.gamma, ri, dt) * O.process_rewards(cfg, rew)
        rsum_list.append(rsum)
        if all_steps_param_grad:
            a = nets.compute_action(po)                                      # :149
        else:
            logits = O.mlp(w_roll, po, cfg.policy_out_act)[:, :cfg.act_dim]
            a = cfg.action_range * torch.tanh(logits) if cfg.action_range is not None else logits
        po_list.append(po), a_list.append(a)
        gam_list.append(O.tf_pow(cfg.gamma, ri + 1, dt) * torch.ones(obses.shape[0], dtype=dt))
    all_q = nets.q('Q1', torch.cat(po_list, 0), torch.cat(a_list, 0))        # :155-156
    final = (torch.cat(rsum_list, 0) + torch.cat(gam_list, 0) * all_q).reshape(n + 1, M, -1)
    return final.mean(1).mean(1)                                             # :166-168


def nadp_compute_gradient(cfg, nets, batch, clip=True):
    """NADPLearner.compute_gradient, nadp.py:209-241 (M = 1).  Returns ([Q1's 6 arrays + the policy's 6], stats)."""
    dt = nets.dtype
    obs, act = [torch.as_tensor(np.asarray(b, dtype=np.float32)).to(dt) for b in batch[:2]]
    n = cfg.n
    targets, _ = rollout_q_estimation(cfg, nets, obs, act, [n])              # :176
    q_losses, q_grads = O.q_forward_and_backward(cfg, nets, obs, act, targets, ['Q1'])     # :173-184
    qg, qn = O.clip_by_global_norm(q_grads[0], cfg.clip)
    reduced = rollout_policy_update(cfg, nets, obs, n)
    policy_loss = -reduced[n]                                                # :170
    pg_raw = list(torch.autograd.grad(policy_loss, nets.w['policy']))
    pg, pn = O.clip_by_global_norm(pg_raw, cfg.clip)
    stats = dict(q_loss=q_losses[0].numpy(), policy_loss=policy_loss.detach().numpy(), value_mean=reduced[0].detach().numpy(),
                 q_gradient_norm=qn.numpy(), policy_gradient_norm=pn.numpy(), targets=targets.numpy())
    out = (qg + pg) if clip else (list(q_grads[0]) + pg_raw)
    return [g.detach().numpy() for g in out], stats


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
def start_obs(rng, B):
    """the generator's start law (tests/golden/make_golden_dp.py:start_obs)"""
    p = rng.uniform(-0.1, 0.1, B)
    th = rng.uniform(-0.1, 0.1, (B, 2))
    v = rng.standard_normal((B, 3)) * 0.1
    frc = rng.standard_normal((B, 3)) * 0.1
    return np.concatenate([p[:, None], np.sin(th), np.cos(th), v, frc], 1).astype(np.float32)


def load_case(golden_dir, H, n):
    """(inputs, results) of a NADP fixture"""
    import os
    inp = np.load(os.path.join(golden_dir, 'nadp_dp_H%d_B64_inputs.npz' % H))
    res = np.load(os.path.join(golden_dir, 'nadp_dp_H%d_B64%s.npz' % (H, '' if n == 25 else '_n%d' % n)))
    assert int(res['n']) == n
    return inp, res


def nets_of(cfg, inp, dtype):
    return O.Nets(cfg, {'policy': inp['w_policy'], 'Q1': inp['w_Q1']}, target_scale=inp['target_scale'], dtype=dtype)


def check_arrays(got, r32, r64, nets, H, where=''):
    """the rule of tests/yardstick.py, per array, where the float64 values are known completely (restatements, H = 32 fixtures).
    nets: [(name, din, dout), ...] in the order of the flat vectors.  Prints every figure, then asserts; returns the worst
    error / allowance ratio."""
    from tests import yardstick as Y
    got, r32, r64 = [np.asarray(v).ravel() for v in (got, r32, r64)]
    o, rows = 0, []
    for nm, din, dout in nets:
        for shp in O.mlp_shapes(din, H, dout):
            n = int(np.prod(shp))
            a, b, c = got[o:o + n], r32[o:o + n], r64[o:o + n]
            o += n
            if np.linalg.norm(b) == 0:
                assert np.linalg.norm(a) == 0, (where, nm, shp, 'reference gradient is exactly zero')
                continue
            rows.append((nm, shp, Y.rel_l2(a, c), Y.rel_l2(b, c), Y.rel_l2(a, b)))
            print('   %s %-6s %-10s vs float64 %.3e  reference float32 %.3e  error / allowance %.3f  vs float32 %.3e'
                  % (where, nm, shp, rows[-1][2], rows[-1][3], rows[-1][2] / (4 * rows[-1][3] + Y.FLOOR), rows[-1][4]))
    assert o == got.size == r32.size == r64.size, (o, got.size, r32.size, r64.size)
    for nm, shp, e_got, e_ref, e32 in rows:
        assert e_got <= 4 * e_ref + Y.FLOOR, (where, nm, shp, 'vs float64: got %.3e, reference float32 %.3e' % (e_got, e_ref))
        assert e_got <= 1e-4 and e32 <= 1e-4, (where, nm, shp, e_got, e32)
    return max(r[2] / (4 * r[3] + Y.FLOOR) for r in rows)


# ---- a short learner loop: compute_gradient + apply_gradients on seeded batches ------------------------------------------------
class _Adam(object):
    """Keras Adam as oracle.AdamState states it (beta 0.9 / 0.999, eps 1e-7, the float32-formed step size), in the run's dtype"""

    def __init__(self, n, dt):
        self.m, self.v, self.step, self.dt = np.zeros(n, dt), np.zeros(n, dt), 0, dt

    def apply(self, w, g, sched):
        f = self.dt
        lr_t = f(O.adam_step_size(sched, self.step))
        self.m = self.m + (g - self.m) * (f(1) - f(np.float32(0.9)))
        self.v = self.v + (g * g - self.v) * (f(1) - f(np.float32(0.999)))
        self.step += 1
        return (w - (self.m * lr_t) / (np.sqrt(self.v) + f(np.float32(1e-7)))).astype(f)


def loop_batches(seed, iters, B):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [(start_obs(rng, B), rng.uniform(-1, 1, (B, 1)).astype(np.float32)) for _ in range(iters)]


def loop_weights(seed):
    from tests.golden_inputs import mlp_weights_flat
    rng = np.random.Generator(np.random.PCG64(seed))
    return {'Q1': mlp_weights_flat(rng, 12, 1), 'policy': mlp_weights_flat(rng, 11, 2)}


def nadp_loop(cfg, w0, batches, dtype):
    """`len(batches)` iterations of NADPLearner.compute_gradient + PolicyWithQs.apply_gradients (policy.py:123-171, delay_update 1:
    every network and the Polyak update every iteration) in `dtype`; returns the final online weights {name: flat}"""
    npdt = np.float64 if dtype == torch.float64 else np.float32
    w = {k: v.astype(npdt) for k, v in w0.items()}
    tgt = {k: v.copy() for k, v in w.items()}
    opt = {k: _Adam(v.size, npdt) for k, v in w.items()}
    tau = npdt(np.float32(cfg.tau))
    for it, (obs, act) in enumerate(batches):
        nets = O.Nets(cfg, w, flat_targets=tgt, dtype=dtype)
        grads, _ = nadp_compute_gradient(cfg, nets, [obs, act])
        g = {'Q1': np.concatenate([x.ravel() for x in grads[:6]]), 'policy': np.concatenate([x.ravel() for x in grads[6:]])}
        w['Q1'] = opt['Q1'].apply(w['Q1'], g['Q1'].astype(npdt), cfg.value_lr)
        w['policy'] = opt['policy'].apply(w['policy'], g['policy'].astype(npdt), cfg.policy_lr)
        for nm in w:
            tgt[nm] = (tau * w[nm] + (npdt(1) - tau) * tgt[nm]).astype(npdt)
    return w
