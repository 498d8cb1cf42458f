"""Restatement of the reference's SAC learner with a fixed temperature (learners/sac.py) in torch on the CPU (float32 / float64),
composed from the pieces of oracle/mpg_oracle.py: the Gaussian head of policy.py:179-204 with action_range None (no bijector), the
soft clipped double-Q target (sac.py:67-80; the action at s' is sampled from the ONLINE policy, :71), the critic losses and
gradients (:102-117) and the policy loss mean(alpha * logp - min Q) by autograd (:119-136).  The draws are the caller's: `eps_target`
for the target action, `eps_policy` for the policy loss, in the order the reference makes them.  The density's arithmetic is the
published formula of MultivariateNormalDiag, log_prob = sum(-0.5 z^2 - log(scale) - 0.5 log(2 pi)), z = (x - loc) / scale.
Used by the tests only; mpg_amd never imports it."""
import math

import numpy as np
import torch

from oracle import mpg_oracle as O
from tests.golden_inputs import mlp_weights_flat

STATS = ('q_loss1', 'q_loss2', 'policy_loss', 'policy_entropy', 'mb_targets_mean', 'value_mean', 'value_var', 'q_gradient_norm1',
         'q_gradient_norm2', 'policy_gradient_norm')
ALPHA = 0.03              # train_script.py:672-792 (built_SAC_parser)
CLIP = 1.0                # the fixtures' gradient_clip_norm (tests/golden/make_golden_sac.py: critics above it, policy below)


def fixture_weights(seed, K=0, H=256):
    """the online networks of tests/golden/make_golden_sac.py for `seed`: its first draws, `policy`, `Q1`, `Q2`, flat Keras order"""
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    return {'policy': mlp_weights_flat(rng, 6 + K, 4, H), 'Q1': mlp_weights_flat(rng, 8 + K, 1, H), 'Q2': mlp_weights_flat(rng, 8 + K, 1, H)}


def make_cfg(K=0, H=256):
    return O.Cfg(obs_dim=6 + K, obs_scale=list(O.OBS_SCALE_PT) + [1.] * K, H=H, delay_update=1, policy_out_act='linear', clip=CLIP,
                 alpha=ALPHA)


def fixture_nets(g, K=0, H=256, dtype=torch.float32):
    """(cfg, nets) of a fixture: its stored weights, or the ones its `weights_seed` regenerates; targets = online * target_scale"""
    cfg = make_cfg(K, H)
    w = {k: g['w_' + k] for k in ('policy', 'Q1', 'Q2')} if 'w_policy' in g else fixture_weights(int(g['weights_seed']), K, H)
    return cfg, O.Nets(cfg, w, target_scale=np.float32(g['target_scale']), dtype=dtype)


def fixture_batch(g):
    return [g['batch_obs'], g['batch_actions'], g['batch_rewards'], g['batch_obs_tp1'], g['batch_dones']]


def sample(cfg, nets, name, po, eps):
    """policy.py:179-204, _logits2dist + sample + log_prob: (actions, logps) of network `name` on processed observations"""
    logits = O.mlp(nets.w[name], po, cfg.policy_out_act)
    mean, log_std = logits[:, :cfg.act_dim], torch.clamp(logits[:, cfg.act_dim:], -5., 1.)
    scale = torch.exp(log_std)
    a = mean + scale * eps
    z = (a - mean) / scale
    return a, (-0.5 * z * z - torch.log(scale) - 0.5 * math.log(2. * math.pi)).sum(-1)


def soft_target(cfg, nets, rew, obs_tp1, eps):
    """sac.py:67-80"""
    with torch.no_grad():
        pr, po = O.process_rewards(cfg, rew), O.process_obses(cfg, obs_tp1)
        a, logp = sample(cfg, nets, 'policy', po, eps)
        return pr + cfg.gamma * (torch.minimum(nets.q('Q1_target', po, a), nets.q('Q2_target', po, a)) - cfg.alpha * logp), logp


def policy_forward_and_backward(cfg, nets, obs, eps):
    """sac.py:119-136; value_var = tf.math.reduce_variance (population)"""
    po = O.process_obses(cfg, obs)
    a, logp = sample(cfg, nets, 'policy', po, eps)
    qmin = torch.minimum(nets.q('Q1', po, a), nets.q('Q2', po, a))
    loss = (cfg.alpha * logp - qmin).mean()
    grads = list(torch.autograd.grad(loss, nets.w['policy']))
    return loss.detach(), grads, -logp.mean().detach(), qmin.mean().detach(), qmin.var(unbiased=False).detach(), logp.detach()


def compute_gradient(cfg, nets, batch, eps_target, eps_policy):
    """SACLearner.compute_gradient, sac.py:169-219 (first call: the batch is fetched).  batch = [obs, act, rew, obs', done] numpy f32.
    Returns (list of numpy grads in reference order q1, q2, policy; stats dict with `targets`, `logp_target`, `logp_policy`)."""
    dt = nets.dtype
    obs, act, rew, obs_tp1 = [torch.as_tensor(np.asarray(b, dtype=np.float32)).to(dt) for b in batch[:4]]
    et, ep = [torch.as_tensor(np.asarray(e, dtype=np.float32)).to(dt) for e in (eps_target, eps_policy)]
    targets, logp_t = soft_target(cfg, nets, rew, obs_tp1, et)
    q_losses, q_grads = O.q_forward_and_backward(cfg, nets, obs, act, targets, ['Q1', 'Q2'])
    g1, n1 = O.clip_by_global_norm(q_grads[0], cfg.clip)
    g2, n2 = O.clip_by_global_norm(q_grads[1], cfg.clip)
    loss, pg, entropy, value_mean, value_var, logp_p = policy_forward_and_backward(cfg, nets, obs, ep)
    pg, pn = O.clip_by_global_norm(pg, cfg.clip)
    stats = dict(q_loss1=q_losses[0].numpy(), q_loss2=q_losses[1].numpy(), policy_loss=loss.numpy(), policy_entropy=entropy.numpy(),
                 mb_targets_mean=targets.numpy().mean(), value_mean=value_mean.numpy(), value_var=value_var.numpy(),
                 q_gradient_norm1=n1.numpy(), q_gradient_norm2=n2.numpy(), policy_gradient_norm=pn.numpy(), targets=targets.numpy(),
                 logp_target=logp_t.numpy(), logp_policy=logp_p.numpy())
    return [g.detach().numpy() for g in g1 + g2 + pg], stats
