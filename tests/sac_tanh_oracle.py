"""Restatement of the reference's SAC learner with an action range (policy.py:183-190: the diagonal Gaussian of tests/sac_oracle.py
wrapped in TransformedDistribution(Chain([Affine(scale_identity_multiplier=R), Tanh()]))) in torch on the CPU (float32 / float64),
composed from tests/sac_oracle.py, tests/sac_auto_oracle.py and oracle/mpg_oracle.py.  Published formulas:
    sample      a = R tanh(u),  u = mean + scale * eps
    log_prob    base.log_prob(u) - [Tanh.forward_log_det_jacobian(u) + Affine.forward_log_det_jacobian(tanh u)]
                Tanh:   sum_k 2 (log 2 - u_k - softplus(-2 u_k));    Affine: act_dim * log |R|
The density is evaluated at u itself: TFP's bijector cache returns the x that produced y when log_prob is called on the tensor that
sample() returned (policy.py:200-204), so no atanh is taken.  InvertedPendulumConti-v0 (train_script4mujoco.py built_SAC_parser:
R = 3, obs_dim 4, act_dim 1) and PathTracking-v0 with a range.  The fixed temperature, or (log_alpha given) the learned one with its
third draw.  Used by the tests only; mpg_amd never imports it."""
import math

import numpy as np
import torch

from oracle import mpg_oracle as O
from tests import sac_auto_oracle as A
from tests import sac_oracle as S
from tests.golden_inputs import mlp_weights_flat

PEND = 'InvertedPendulumConti-v0'
PT = 'PathTracking-v0'
STATS, CLIP, ALPHA = S.STATS, S.CLIP, S.ALPHA


def dims(env, K=0):
    """(obs_dim, act_dim)"""
    return (4, 1) if env == PEND else (6 + K, 2)


def net_list(env, K=0):
    """[(name, in, out)] in the order of the flat gradient (tests/yardstick.py layout)"""
    od, ad = dims(env, K)
    return [('Q1', od + ad, 1), ('Q2', od + ad, 1), ('policy', od, 2 * ad)]


def fixture_weights(seed, env, K=0, H=256):
    """the online networks of tests/golden/make_golden_sac_tanh.py for `seed`: its first draws, `policy`, `Q1`, `Q2`, flat Keras order"""
    od, ad = dims(env, K)
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    return {'policy': mlp_weights_flat(rng, od, 2 * ad, H), 'Q1': mlp_weights_flat(rng, od + ad, 1, H),
            'Q2': mlp_weights_flat(rng, od + ad, 1, H)}


def make_cfg(env, action_range, K=0, H=256, alpha=ALPHA):
    if env == PEND:
        return O.Cfg(env, H=H, delay_update=1, policy_out_act='linear', clip=CLIP, alpha=alpha, action_range=float(action_range))
    return O.Cfg(env, obs_dim=6 + K, obs_scale=list(O.OBS_SCALE_PT) + [1.] * K, H=H, delay_update=1, policy_out_act='linear', clip=CLIP,
                 alpha=alpha, action_range=float(action_range))


def fixture_nets(g, env, K=0, H=256, dtype=torch.float32):
    """(cfg, nets) of a fixture: its stored weights, or the ones its `weights_seed` regenerates; targets = online * target_scale"""
    cfg = make_cfg(env, float(g['action_range']), K, H)
    w = {k: g['w_' + k] for k in ('policy', 'Q1', 'Q2')} if 'w_policy' in g else fixture_weights(int(g['weights_seed']), env, K, H)
    return cfg, O.Nets(cfg, w, target_scale=np.float32(g['target_scale']), dtype=dtype)


def tanh_fldj(u):
    """Tanh.forward_log_det_jacobian, elementwise"""
    return 2. * (math.log(2.) - u - torch.nn.functional.softplus(-2. * u))


def head(cfg, logits, eps):
    """(actions, logps, u) of the squashed head on the 2 act_dim logits"""
    ad, R = cfg.act_dim, cfg.action_range
    mean, log_std = logits[:, :ad], torch.clamp(logits[:, ad:], -5., 1.)
    scale = torch.exp(log_std)
    u = mean + scale * eps
    z = (u - mean) / scale
    base = (-0.5 * z * z - torch.log(scale) - 0.5 * math.log(2. * math.pi)).sum(-1)
    return R * torch.tanh(u), base - tanh_fldj(u).sum(-1) - ad * math.log(abs(R)), u


def sample(cfg, nets, name, po, eps):
    """S.sample under the bijectors: (actions, logps) of network `name` on processed observations"""
    a, logp, _ = head(cfg, O.mlp(nets.w[name], po, cfg.policy_out_act), eps)
    return a, logp


def soft_target(cfg, nets, rew, obs_tp1, eps):
    """sac.py:67-80"""
    with torch.no_grad():
        pr, po = O.process_rewards(cfg, rew), O.process_obses(cfg, obs_tp1)
        a, logp = sample(cfg, nets, 'policy', po, eps)
        return pr + cfg.gamma * (torch.minimum(nets.q('Q1_target', po, a), nets.q('Q2_target', po, a)) - cfg.alpha * logp), logp


def policy_forward_and_backward(cfg, nets, obs, eps):
    """sac.py:119-136"""
    po = O.process_obses(cfg, obs)
    a, logp = sample(cfg, nets, 'policy', po, eps)
    qmin = torch.minimum(nets.q('Q1', po, a), nets.q('Q2', po, a))
    loss = (cfg.alpha * logp - qmin).mean()
    grads = list(torch.autograd.grad(loss, nets.w['policy']))
    return loss.detach(), grads, -logp.mean().detach(), qmin.mean().detach(), qmin.var(unbiased=False).detach(), logp.detach()


def compute_gradient(cfg, nets, batch, eps_target, eps_policy, eps_alpha=None, log_alpha=None, target_entropy=None):
    """SACLearner.compute_gradient (sac.py:169-219) with an action range: S.compute_gradient's outputs; with log_alpha (alpha = 'auto')
    A.compute_gradient's - the temperature's clipped 0-d gradient appended and `alpha`, `alpha_loss`, `alpha_gradient_norm`,
    `logp_alpha` among the stats."""
    dt = nets.dtype
    if log_alpha is not None:
        cfg = A.with_alpha(cfg, log_alpha, dt)
    obs, act, rew, obs_tp1 = [torch.as_tensor(np.asarray(b, dtype=np.float32)).to(dt) for b in batch[:4]]
    et, ep = [torch.as_tensor(np.asarray(e, dtype=np.float32)).to(dt) for e in (eps_target, eps_policy)]
    targets, logp_t = soft_target(cfg, nets, rew, obs_tp1, et)
    q_losses, q_grads = O.q_forward_and_backward(cfg, nets, obs, act, targets, ['Q1', 'Q2'])
    g1, n1 = O.clip_by_global_norm(q_grads[0], cfg.clip)
    g2, n2 = O.clip_by_global_norm(q_grads[1], cfg.clip)
    loss, pg, entropy, value_mean, value_var, logp_p = policy_forward_and_backward(cfg, nets, obs, ep)
    pg, pn = O.clip_by_global_norm(pg, cfg.clip)
    st = dict(q_loss1=q_losses[0].numpy(), q_loss2=q_losses[1].numpy(), policy_loss=loss.numpy(), policy_entropy=entropy.numpy(),
              mb_targets_mean=targets.numpy().mean(), value_mean=value_mean.numpy(), value_var=value_var.numpy(),
              q_gradient_norm1=n1.numpy(), q_gradient_norm2=n2.numpy(), policy_gradient_norm=pn.numpy(), targets=targets.numpy(),
              logp_target=logp_t.numpy(), logp_policy=logp_p.numpy())
    grads = [g.detach().numpy() for g in g1 + g2 + pg]
    if log_alpha is None:
        return grads, st
    ea = torch.as_tensor(np.asarray(eps_alpha, dtype=np.float32)).to(dt)                    # sac.py:138-148
    with torch.no_grad():
        _, logp_a = sample(cfg, nets, 'policy', O.process_obses(cfg, obs), ea)
    la = torch.tensor(float(log_alpha), dtype=dt, requires_grad=True)
    a_loss = (-la * (logp_a + target_entropy)).mean()
    g, = torch.autograd.grad(a_loss, [la])
    (gc,), norm = O.clip_by_global_norm([g], cfg.clip)
    st.update(alpha=torch.exp(la.detach()).numpy(), alpha_loss=a_loss.detach().numpy(), alpha_gradient_norm=norm.numpy(),
              logp_alpha=logp_a.numpy())
    return grads + [gc.numpy()], st
