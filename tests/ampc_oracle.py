"""Restatement of the reference's AMPC learner (learners/ampc.py) in torch on the CPU (float32 / float64), composed from the pieces of
oracle/mpg_oracle.py and, for InvertedDoublePendulum-v2, tests/dp_oracle.py: the n-step model rollout with every step through the
policy, NO critic and NO discount (ampc.py:73-87), the policy gradient by autograd and tf.clip_by_global_norm (:105-112).
Used by the tests only; mpg_amd never imports it."""
import numpy as np
import torch

from oracle import mpg_oracle as O
from tests import dp_oracle as DP
from tests.golden_inputs import mlp_weights_flat

STATS = ('policy_loss', 'policy_gradient_norm')
# fixture -> (env, num_future_data): the three cases of tests/golden/make_golden_ampc.py
FIXTURES = {'ampc_H256_B64.npz': ('PathTracking-v0', 0), 'ampc_H256_B64_K3_M2.npz': ('PathTracking-v0', 3),
            'ampc_dp_H256_B64_n10.npz': (DP.ENV_ID, 0)}


def make_cfg(env='PathTracking-v0', K=0, n=25, M=1, clip=3., H=256, **kw):
    """the oracle's Cfg of built_AMPC_parser (gamma = 1 reaches the Preprocessor only: the rollout never reads it)"""
    if env == DP.ENV_ID:
        c = DP.make_cfg(n, H=H)
    elif env == 'PathTracking-v0':
        c = O.Cfg(obs_dim=6 + K, obs_scale=list(O.OBS_SCALE_PT) + [1.] * K, H=H)
    else:
        c = O.Cfg(env, H=H)
    c.n, c.M, c.clip, c.gamma = int(n), int(M), float(clip), 1.
    c.__dict__.update(kw)
    return c


def policy_dims(cfg):
    return cfg.obs_dim, 2 * cfg.act_dim


def fixture_weights(seed, cfg):
    """the policy of tests/golden/make_golden_ampc.py for `seed`: its first draws, flat Keras order"""
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    din, dout = policy_dims(cfg)
    return {'policy': mlp_weights_flat(rng, din, dout, cfg.H)}


def fixture_case(g, name, dtype=torch.float32):
    """(cfg, nets, batch_obs, eps or None) of a fixture: the weights its `weights_seed` regenerates"""
    env, K = FIXTURES[name]
    cfg = make_cfg(env, K, n=int(g['n']), M=int(g['M']), clip=float(g['clip']))
    nets = O.Nets(cfg, fixture_weights(int(g['weights_seed']), cfg), dtype=dtype)
    return cfg, nets, g['batch_obs'], g.get('eps')


def make_model(cfg):
    return DP.DoublePendulumModelOracle() if cfg.env == DP.ENV_ID else O.make_model(cfg)


def model_rollout_for_policy_update(cfg, nets, start_obses, eps, model=None):
    """AMPCLearner.model_rollout_for_policy_update, ampc.py:73-87.  eps [n, M*B] standard normal (None: a model without noise).
    model: a model object to roll instead of make_model(cfg) (tests/model_edge_inputs.py).  Returns (policy_loss, rewards_sum [M*B])."""
    dt = nets.dtype
    obses = start_obses.repeat(cfg.M, 1)                                     # :74
    model = make_model(cfg) if model is None else model
    model.reset(obses)                                                       # :75
    rsum = torch.zeros(obses.shape[0], dtype=dt)                             # :76
    for t in range(cfg.n):                                                   # :79
        actions = nets.compute_action(O.process_obses(cfg, obses))           # :80-81
        obses, rew = model.rollout_out(actions, None if eps is None else eps[t])     # :82
        rsum = rsum + O.process_rewards(cfg, rew)                            # :83 (no gamma)
    return -rsum.mean(), rsum                                                # :85


def compute_gradient(cfg, nets, batch_obs, eps, clip=True, model=None):
    """AMPCLearner.compute_gradient, ampc.py:105-122.  Returns (the policy's 6 gradient arrays as numpy, stats with the un-clipped
    flat gradient and the per-trajectory reward sums)."""
    dt = nets.dtype
    obs = torch.as_tensor(np.asarray(batch_obs, dtype=np.float32)).to(dt)
    e = None if eps is None else torch.as_tensor(np.asarray(eps, dtype=np.float32)).to(dt)
    loss, rsum = model_rollout_for_policy_update(cfg, nets, obs, e, model=model)
    raw = list(torch.autograd.grad(loss, nets.w['policy']))
    pg, pn = O.clip_by_global_norm(raw, cfg.clip)
    stats = dict(policy_loss=loss.detach().numpy(), policy_gradient_norm=pn.numpy(), rewards_sum=rsum.detach().numpy(),
                 grad_unclipped=np.concatenate([g.numpy().ravel() for g in raw]))
    return [g.detach().numpy() for g in (pg if clip else raw)], stats
