"""Restatement of the reference's n-step DPG learner (learners/ndpg.py) in torch on the CPU (float32 / float64), composed from the
pieces of oracle/mpg_oracle.py: MPG-v1's n-step real-env target (ndpg.py:127-151 = mpg_learner.py:146-169), the critic loss and
gradient (:162-172), and the one-step DPG policy loss through Q1 by autograd (:174-186).  Used by the tests only; mpg_amd never
imports it."""
import numpy as np
import torch

from oracle import mpg_oracle as O
from tests.golden_inputs import mlp_weights_flat

STATS = ('q_loss', 'policy_loss', 'mb_targets_mean', 'value_mean', 'value_var', 'q_gradient_norm', 'policy_gradient_norm')


def fixture_weights(seed, K=0, H=256):
    """the online networks of tests/golden/make_golden_ndpg.py for `seed`: its first draws, `policy` then `Q1`, flat Keras order"""
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    return {'policy': mlp_weights_flat(rng, 6 + K, 4, H), 'Q1': mlp_weights_flat(rng, 8 + K, 1, H)}


def make_cfg(K=0, H=256, n=25):
    return O.Cfg(obs_dim=6 + K, obs_scale=list(O.OBS_SCALE_PT) + [1.] * K, H=H, n=n, delay_update=1)


def fixture_nets(g, K=0, H=256, dtype=torch.float32):
    """(cfg, nets) of a fixture: its stored weights, or the ones its `weights_seed` regenerates; targets = online * target_scale"""
    cfg = make_cfg(K, H)
    if 'w_policy' in g:
        w = {'policy': g['w_policy'], 'Q1': g['w_Q1']}
    else:
        w = fixture_weights(int(g['weights_seed']), K, H)
    return cfg, O.Nets(cfg, w, target_scale=np.float32(g['target_scale']), dtype=dtype)


def fixture_batch(g):
    return [g['batch_obs'], g['batch_actions'], g['batch_rewards'], g['batch_obs_tp1'], g['batch_dones']]


def policy_forward_and_backward(cfg, nets, obs):
    """ndpg.py:174-186: loss = -mean Q1(s~, pi(s~)); value_var = tf.math.reduce_variance (population)"""
    po = O.process_obses(cfg, obs)
    q = nets.q('Q1', po, nets.compute_action(po))
    loss = -q.mean()
    grads = list(torch.autograd.grad(loss, nets.w['policy']))
    return loss.detach(), grads, -loss.detach(), q.var(unbiased=False).detach()


def compute_gradient(cfg, nets, batch):
    """NDPGLearner.compute_gradient, ndpg.py:202-237 (first call: the batch is fetched).  batch = [obs, act, rew, obs', done] numpy f32.
    Returns (list of numpy grads in reference order q1, policy; stats dict with `targets`)."""
    dt = nets.dtype
    obs, act = [torch.as_tensor(np.asarray(b, dtype=np.float32)).to(dt) for b in batch[:2]]
    targets = torch.as_tensor(O.n_step_target(cfg, nets, np.asarray(batch[0], np.float32), np.asarray(batch[1], np.float32))).to(dt)
    q_losses, q_grads = O.q_forward_and_backward(cfg, nets, obs, act, targets, ['Q1'])
    qg, qn = O.clip_by_global_norm(q_grads[0], cfg.clip)
    loss, pg, value_mean, value_var = policy_forward_and_backward(cfg, nets, obs)
    pg, pn = O.clip_by_global_norm(pg, cfg.clip)
    stats = dict(q_loss=q_losses[0].numpy(), policy_loss=loss.numpy(), mb_targets_mean=targets.numpy().mean(), value_mean=value_mean.numpy(),
                 value_var=value_var.numpy(), q_gradient_norm=qn.numpy(), policy_gradient_norm=pn.numpy(), targets=targets.numpy())
    return [g.detach().numpy() for g in qg + pg], stats
