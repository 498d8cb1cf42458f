"""Writes the fixtures of SAC with an ACTION RANGE - the tanh-squashed Gaussian head - from the UNMODIFIED reference, beside
make_golden_sac.py and make_golden_sac_auto.py, whose helpers it uses:

    sac_tanh_pend_H256_B64.npz        learners.sac.SACLearner.compute_gradient, InvertedPendulumConti-v0, action_range 3, alpha 0.03
    sac_tanh_pend_auto_H256_B64.npz   the same with alpha 'auto', target_entropy -2
    sac_tanh_pt_H256_B64.npz          PathTracking-v0 with action_range 2 (not 1: act_dim * log R is then not zero)
    sac_tanh_pend_H32_B64.npz         the pendulum with 32-unit nets (CPU tests only; keeps its weights, it is tiny)
    sac_mujoco_parser_defaults.json   what train_scripts/train_script4mujoco.py:built_SAC_parser() returns (settings only)

    MPG_REFERENCE=/path/to/reference python tests/golden/make_golden_sac_tanh.py

The reference's learners/sac.py and policy.py run as they are.  policy.py:183-190 wraps the Gaussian in
tfp.distributions.TransformedDistribution(bijector=tfb.Chain([tfb.Affine(scale_identity_multiplier=R), tfb.Tanh()])).  The stand-in
packages under oracle/refshim lack those four symbols; they are put into the stand-in's `distributions` and `bijectors` objects
here, at run time, beside MultivariateNormalDiag (make_golden_sac.py) - policy.py binds `tfb = tfp.bijectors` in its class body,
and it is that very object that receives the attributes.  Published formulas, not TFP's code:
    Tanh     forward tanh(x);  forward_log_det_jacobian 2 (log 2 - x - softplus(-2 x)), summed over the event
    Affine   forward s x;      forward_log_det_jacobian (event size) * log |s|
    Chain    [b1, b2]: forward b1(b2(x)); the log-dets add, b1's taken at b2(x)
    TransformedDistribution    sample() = bijector.forward(distribution.sample());  log_prob(y) = distribution.log_prob(x) -
                               forward_log_det_jacobian(x), x the cached input where y IS the tensor sample() returned (TFP's
                               bijector cache; policy.py:200-204 calls log_prob on exactly that tensor), else bijector.inverse(y)
An inherent pin, like the others.  The draws are RECORDED standard normals: `eps_target`, `eps_policy` (and `eps_alpha`), [B, act_dim].

InvertedPendulumConti-v0 is a MuJoCo environment and MuJoCo is absent: the pendulum's replay batch is seeded data of the env's
shapes (a learner treats a batch as data) - observations in the range an episode visits, actions in [-3, 3], rewards in (0.5, 1.5).

Self-checks, on the reference alone: a case is written for the first seed of a fixed list whose float32 run is within a QUARTER of
the 1e-4 bar of tests/yardstick.py from its float64 run on every gradient array, the targets and every logp array, and for which
gradient_clip_norm = 1.0 is exercised on both sides (a critic norm above it, the policy norm below it).  The figures of every seed
tried are printed."""
import json
import os
import sys

import numpy as np

import make_golden as G                                 # noqa: E402
from make_golden import NoiseStream, add_targets, flat, make_replay_batch_pt, set_policy_weights, sub64     # noqa: E402
from make_golden_sac import QUARTER_BAR, inject, sac_args              # noqa: E402
from make_golden_sac_auto import inject_alpha             # noqa: E402
from golden_inputs import mlp_weights_list              # noqa: E402
from tests.sac_auto_oracle import ALPHA_LR, LOG_ALPHA0             # noqa: E402
from tests.sac_auto_oracle import STATS as AUTO_STATS              # noqa: E402
from tests.sac_tanh_oracle import CLIP, PEND, PT, STATS, dims, fixture_weights      # noqa: E402

torch, tf = G.torch, G.tf
HERE = G.HERE
SEEDS = (2, 3, 4, 5, 6, 7, 8, 9, 10, 11)
TARGET_ENTROPY = -2.0
LOG_2 = float(np.log(2.))


class Tanh(object):
    def forward(self, x):
        return torch.tanh(x)

    def inverse(self, y):
        return torch.atanh(y)

    def forward_log_det_jacobian(self, x):
        return (2. * (LOG_2 - x - torch.nn.functional.softplus(-2. * x))).sum(-1)


class Affine(object):
    def __init__(self, scale_identity_multiplier=None, **kw):
        assert scale_identity_multiplier is not None and not kw, 'policy.py:187 passes scale_identity_multiplier only'
        self.s = float(scale_identity_multiplier)

    def forward(self, x):
        return self.s * x

    def inverse(self, y):
        return y / self.s

    def forward_log_det_jacobian(self, x):
        return x.shape[-1] * float(np.log(abs(self.s))) + torch.zeros(x.shape[:-1], dtype=x.dtype)


class Chain(object):
    def __init__(self, bijectors):
        self.bijectors = list(bijectors)          # applied right to left

    def forward(self, x):
        for b in reversed(self.bijectors):
            x = b.forward(x)
        return x

    def inverse(self, y):
        for b in self.bijectors:
            y = b.inverse(y)
        return y

    def forward_log_det_jacobian(self, x):
        total = 0.
        for b in reversed(self.bijectors):
            total = total + b.forward_log_det_jacobian(x)
            x = b.forward(x)
        return total


class TransformedDistribution(object):
    def __init__(self, distribution, bijector, **kw):
        self.distribution, self.bijector, self._cache = distribution, bijector, (None, None)

    def sample(self, *a, **k):
        x = self.distribution.sample()
        y = self.bijector.forward(x)
        self._cache = (y, x)
        return y

    def log_prob(self, y):
        x = self._cache[1] if y is self._cache[0] else self.bijector.inverse(y)
        return self.distribution.log_prob(x) - self.bijector.forward_log_det_jacobian(x)


def inject_bijectors():
    inject_alpha()                 # MultivariateNormalDiag and the AlphaModel's weight list
    import tensorflow_probability as tfp
    tfp.distributions.TransformedDistribution = TransformedDistribution
    for cls in (Chain, Affine, Tanh):
        setattr(tfp.bijectors, cls.__name__, cls)


def tanh_args(env, B, H, action_range, auto):
    args = sac_args(B, H, 0)                         # built_SAC_parser's settings on PathTracking, gradient_clip_norm 1.0
    if env == PEND:                                  # train_script4mujoco.py built_SAC_parser
        args.env_id, args.num_agent, args.obs_dim, args.act_dim = PEND, 1, 4, 1
        args.obs_scale, args.rew_scale = list(G.OBS_SCALE_PD), 1.
    args.action_range = float(action_range)
    if auto:
        args.alpha, args.target_entropy, args.alpha_lr_schedule = 'auto', TARGET_ENTROPY, list(ALPHA_LR)
    return args


def pendulum_batch(rng, B):
    obs = (rng.standard_normal((B, 4)) * np.array([0.5, 0.1, 0.5, 0.5])).astype(np.float32)
    obs2 = (obs + rng.standard_normal((B, 4)) * np.array([0.02, 0.01, 0.1, 0.1])).astype(np.float32)
    act = rng.uniform(-3, 3, (B, 1)).astype(np.float32)
    rew = rng.uniform(0.5, 1.5, B).astype(np.float32)
    return [obs, act, rew, obs2, np.zeros(B, np.float32)]


def fx(env, H, B, action_range, auto, seed, lean, name):
    inject_bijectors()
    from learners.sac import SACLearner
    from policy import PolicyWithQs
    od, ad = dims(env)
    rng = np.random.Generator(np.random.PCG64(seed))
    args = tanh_args(env, B, H, action_range, auto)
    nets = {'policy': mlp_weights_list(rng, od, H, 2 * ad), 'Q1': mlp_weights_list(rng, od + ad, H, 1),
            'Q2': mlp_weights_list(rng, od + ad, H, 1)}
    add_targets(nets)
    if auto:
        nets['alpha'] = [np.array(LOG_ALPHA0, np.float32)]
    batch = pendulum_batch(rng, B) if env == PEND else make_replay_batch_pt(rng, B, 0)
    names = ('eps_target', 'eps_policy') + (('eps_alpha',) if auto else ())
    eps = [rng.standard_normal((B, ad)).astype(np.float32) for _ in names]
    out = dict(batch_obs=batch[0], batch_actions=batch[1], batch_rewards=batch[2], batch_obs_tp1=batch[3], batch_dones=batch[4],
               target_scale=G.TARGET_SCALE, weights_seed=np.array(seed), action_range=np.array(action_range, np.float32))
    out.update(zip(names, eps))
    if auto:
        out.update(log_alpha=np.array(LOG_ALPHA0), target_entropy=np.array(TARGET_ENTROPY, np.float32))
    logps = tuple('logp_' + n[4:] for n in names)
    n_net = 18
    full = {}
    for tag, dt in (('', torch.float32), ('_f64', torch.float64)):
        tf.set_ref_dtype(dt)
        learner = SACLearner(PolicyWithQs, args)
        pw = learner.policy_with_value
        set_policy_weights(pw, nets)
        tf.set_noise_source(NoiseStream(list(eps)))
        grads = learner.compute_gradient(batch, None, None, 0)
        assert len(grads) == n_net + int(auto)
        st = learner.get_stats()
        full[tag] = [np.asarray(g, np.float64) for g in grads]
        out['grads' + tag] = flat(grads[:n_net]) if tag == '' else sub64(flat(grads[:n_net]), H)
        if auto:
            out['alpha_grad' + tag] = np.asarray(grads[n_net])
        out['targets' + tag] = np.asarray(learner.batch_data['batch_targets'])
        for key in (AUTO_STATS if auto else STATS):
            out[key + tag] = np.asarray(st[key])
        # logp (and the actions) of every draw, from the reference's own compute_action on the same noise
        po = [learner.preprocessor.tf_process_obses(batch[i]).numpy() for i in (3, 0, 0)[:len(names)]]
        tf.set_noise_source(NoiseStream(list(eps)))
        for k, p in zip(logps, po):
            a, lp = pw.compute_action(p)
            out[k + tag] = np.asarray(lp)
            out['act_' + k[5:] + tag] = np.asarray(a)
            assert np.abs(np.asarray(a)).max() <= action_range
        for k in ('targets',) + logps:
            full[k + tag] = np.asarray(out[k + tag], np.float64)
    out['small64'] = np.concatenate([g.ravel() for g in full['_f64'][:n_net] if g.size < 8])
    tf.set_ref_dtype(torch.float32)
    tf.set_noise_source(None)
    rel = [np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30) for a, b in zip(full[''], full['_f64'])]
    rel_v = [np.linalg.norm(full[k] - full[k + '_f64']) / np.linalg.norm(full[k + '_f64']) for k in ('targets',) + logps]
    qn1, qn2, pn = [float(out[k]) for k in ('q_gradient_norm1', 'q_gradient_norm2', 'policy_gradient_norm')]       # norms BEFORE the clip
    print('%s seed %d: reference float32 vs float64, rel L2 per array: %s   (max %.1e); targets / logp %s; norms Q1 %.2f Q2 %.2f '
          'policy %.2f%s' % (name, seed, ' '.join('%.1e' % r for r in rel), max(rel), ' '.join('%.1e' % r for r in rel_v), qn1, qn2, pn,
                             '; temperature |g| %.3f' % float(out['alpha_gradient_norm']) if auto else ''))
    ok = max(max(rel), max(rel_v)) <= QUARTER_BAR and max(qn1, qn2) > CLIP and pn < CLIP
    if ok:
        if lean:
            for k, v in fixture_weights(seed, env, 0, H).items():
                assert np.array_equal(flat(nets[k]), v), k
        else:
            for k in ('policy', 'Q1', 'Q2'):
                out['w_' + k] = flat(nets[k])
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) <= 1 << 20, (path, os.path.getsize(path))
    return ok


def fx_parser_defaults():
    """built_SAC_parser() of train_script4mujoco.py as it lies: argparse defaults, nothing on the command line"""
    sys.path.insert(0, os.path.join(G.REF, 'train_scripts'))
    argv, sys.argv = sys.argv, sys.argv[:1]
    cwd = os.getcwd()
    try:
        os.chdir(os.path.join(G.REF, 'train_scripts'))
        import train_script4mujoco
        d = vars(train_script4mujoco.built_SAC_parser())
    finally:
        sys.argv = argv
        os.chdir(cwd)
    for k in ('result_dir', 'log_dir', 'model_dir'):        # time-stamped paths
        d.pop(k)
    with open(os.path.join(HERE, 'sac_mujoco_parser_defaults.json'), 'w') as fh:
        json.dump(d, fh, indent=1, sort_keys=True)
        fh.write('\n')


CASES = ((PEND, 256, 3., False, True, 'sac_tanh_pend_H256_B64.npz'), (PEND, 256, 3., True, True, 'sac_tanh_pend_auto_H256_B64.npz'),
         (PT, 256, 2., False, True, 'sac_tanh_pt_H256_B64.npz'), (PEND, 32, 3., False, False, 'sac_tanh_pend_H32_B64.npz'))


def main():
    torch.manual_seed(0)
    for env, H, R, auto, lean, name in CASES:
        assert any(fx(env, H, 64, R, auto, seed, lean, name) for seed in SEEDS), 'no seed of the list meets the conditions (%s)' % name
    fx_parser_defaults()


if __name__ == '__main__':
    main()
