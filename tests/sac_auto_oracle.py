"""Restatement of the reference's SAC learner with the LEARNED temperature (alpha = 'auto'; learners/sac.py:138-148,206-216,
policy.py:136-143) in torch on the CPU, on top of tests/sac_oracle.py and oracle/mpg_oracle.py: alpha = exp(log_alpha) in the soft
target and the policy loss (no gradient into log_alpha), the temperature's loss mean(-log_alpha (logp + target_entropy)) on a THIRD
draw `eps_alpha` from the same policy on the same observations, its gradient -(mean logp + target_entropy) clipped alone in its list
and appended last, and the temperature's own Keras Adam, stepped with the policy's when iteration % delay_update == 0.
Used by the tests only; mpg_amd never imports it."""
import copy

import numpy as np
import torch

from oracle import mpg_oracle as O
from tests import sac_oracle as S

LOG_ALPHA0 = np.float32(np.log(0.2))           # the fixtures' start: alpha neither 1 nor the fixed default 0.03
ALPHA_LR = [8e-5, 100000, 8e-6]                # built_SAC_parser's alpha_lr_schedule
STATS = S.STATS + ('alpha', 'alpha_loss', 'alpha_gradient_norm')


def with_alpha(cfg, log_alpha, dtype):
    c = copy.copy(cfg)
    c.alpha = torch.exp(torch.tensor(float(log_alpha), dtype=dtype))          # sac.py:76,127 (a float32 tensor in the reference)
    return c


def alpha_forward_and_backward(cfg, nets, obs, eps_alpha, log_alpha, target_entropy):
    """sac.py:138-148 and the clip of :209: (alpha_loss, alpha, clipped gradient, norm before the clip)"""
    dt = nets.dtype
    with torch.no_grad():
        _, logp = S.sample(cfg, nets, 'policy', O.process_obses(cfg, obs), eps_alpha)
    la = torch.tensor(float(log_alpha), dtype=dt, requires_grad=True)
    loss = (-la * (logp + target_entropy)).mean()
    g, = torch.autograd.grad(loss, [la])
    (gc,), norm = O.clip_by_global_norm([g], cfg.clip)
    return loss.detach(), torch.exp(la.detach()), gc, norm, logp


def compute_gradient(cfg, nets, batch, eps_target, eps_policy, eps_alpha, log_alpha, target_entropy):
    """SACLearner.compute_gradient with alpha = 'auto': 19 numpy arrays (q1, q2, policy, the temperature's 0-d gradient) and the stats"""
    dt = nets.dtype
    c = with_alpha(cfg, log_alpha, dt)
    grads, st = S.compute_gradient(c, nets, batch, eps_target, eps_policy)
    obs = torch.as_tensor(np.asarray(batch[0], dtype=np.float32)).to(dt)
    ea = torch.as_tensor(np.asarray(eps_alpha, dtype=np.float32)).to(dt)
    loss, alpha, g, norm, logp = alpha_forward_and_backward(c, nets, obs, ea, log_alpha, target_entropy)
    st.update(alpha=alpha.numpy(), alpha_loss=loss.numpy(), alpha_gradient_norm=norm.numpy(), logp_alpha=logp.numpy())
    return grads + [g.numpy()], st


class Loop(object):
    """compute_gradient + PolicyWithQs.apply_gradients, iteration after iteration, on flat float32 weights: the networks through
    oracle/mpg_oracle.py apply_gradients, the temperature's Adam (its own object and counter) beside the policy's"""
    NAMES = ['Q1', 'Q2', 'policy']

    def __init__(self, cfg, weights, targets, log_alpha, target_entropy, dtype=torch.float32):
        self.cfg, self.dtype, self.target_entropy = cfg, dtype, target_entropy
        self.w = {k: np.array(v, np.float32) for k, v in weights.items()}
        self.t = {k: np.array(v, np.float32) for k, v in targets.items()}
        self.opt = {k: O.AdamState(self.w[k].size) for k in self.NAMES}
        self.log_alpha, self.alpha_opt = np.array([log_alpha], np.float32), O.AdamState(1)

    def step(self, iteration, batch, eps_target, eps_policy, eps_alpha):
        nets = O.Nets(self.cfg, self.w, flat_targets=self.t, dtype=self.dtype)
        grads, st = compute_gradient(self.cfg, nets, batch, eps_target, eps_policy, eps_alpha, self.log_alpha[0], self.target_entropy)
        flat = {k: np.concatenate([g.ravel() for g in grads[6 * i:6 * i + 6]]).astype(np.float32) for i, k in enumerate(self.NAMES)}
        O.apply_gradients(self.cfg, self.w, self.t, self.opt, flat, iteration, self.NAMES)
        if iteration % self.cfg.delay_update == 0:                      # policy.py:136-143
            self.log_alpha = self.alpha_opt.apply(self.log_alpha, np.array([grads[18]], np.float32), ALPHA_LR)
        return grads, st
