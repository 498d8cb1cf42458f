"""Writes the SAC fixtures from the UNMODIFIED reference (beside make_golden.py, whose helpers it uses):

    sac_H256_B64.npz         learners.sac.SACLearner.compute_gradient, PathTracking-v0, alpha 0.03, num_future_data 0
    sac_H256_B64_K3.npz      the same with num_future_data = 3 (obs_dim 9)
    sac_H32_B64.npz          32-unit nets (CPU tests only; keeps its weights, it is tiny)
    sac_parser_defaults.json     what train_scripts/train_script.py:built_SAC_parser() returns (settings only; the time-stamped
                                 result / log / model directories left out)

    MPG_REFERENCE=/path/to/reference python tests/golden/make_golden_sac.py

The reference's learners/sac.py and policy.py run as they are.  The one symbol the stand-in packages under oracle/refshim lack,
tfp.distributions.MultivariateNormalDiag, is put into the stand-in's `distributions` namespace here, at run time: sample() = loc +
scale * eps with eps taken from the stand-in's noise source, log_prob(x) = sum(-0.5 z^2 - log(scale) - 0.5 log(2 pi)), z = (x - loc) /
scale.  That is TFP's published formula, not TFP's code: the fixtures pin the reference's GRAPH on that arithmetic - an inherent pin,
like the Keras Adam restatement of the loop fixtures.  The draws are RECORDED standard normals (float32 values, cast to the run's
dtype), so the float32 run, the float64 run and the device see the same noise: `eps_target` [B, 2] for the action at s'
(sac.py:71), then `eps_policy` [B, 2] for the policy loss (:123) - the two draws of one compute_gradient call, in that order.

The H = 256 files are lean (at most 1 MiB each): `weights_seed` instead of the weights - tests/sac_oracle.py fixture_weights(seed, K)
regenerates them in the same draw order (asserted equal here) - the float32 gradients completely, every 8th element of the float64
ones (make_golden.sub64) and `small64`.

The generator checks its own draw, on the reference alone: a case is written for the first seed of a fixed list whose float32 run is
within a QUARTER of the 1e-4 bar of tests/yardstick.py from its float64 run on every gradient array, the targets and both logp
arrays.  The fixtures' args use gradient_clip_norm = 1.0 so that the clip is exercised on both sides: the seed must also have at
least one un-clipped critic norm above it and the policy norm below it.  The figures of every seed tried are printed."""
import json
import os
import sys
import types

import numpy as np

import make_golden as G                                 # noqa: E402
from make_golden import NoiseStream, add_targets, flat, make_replay_batch_pt, mpg_args, set_policy_weights, sub64     # noqa: E402
from golden_inputs import mlp_weights_list              # noqa: E402  (make_golden put tests/ on the path)
from tests.sac_oracle import ALPHA, CLIP, STATS, fixture_weights    # noqa: E402  (make_golden put the repository root on the path too)

torch, tf = G.torch, G.tf
HERE = G.HERE
QUARTER_BAR = 0.25e-4
SEEDS = (2, 3, 4, 5, 6, 7)


class MultivariateNormalDiag(object):
    """the stand-in put into oracle/refshim's tensorflow_probability.distributions (see the module docstring)"""

    def __init__(self, loc, scale_diag, **kw):
        self.loc, self.scale = tf.convert_to_tensor(loc), tf.convert_to_tensor(scale_diag)

    def sample(self, *a, **k):
        return self.loc + self.scale * tf._std_normal(self.loc.shape)

    def log_prob(self, x):
        z = (x - self.loc) / self.scale
        return (-0.5 * z * z - torch.log(self.scale) - 0.5 * float(np.log(2. * np.pi))).sum(-1)


def inject():
    import tensorflow_probability as tfp
    if isinstance(tfp.distributions, types.SimpleNamespace):
        tfp.distributions.MultivariateNormalDiag = MultivariateNormalDiag


def sac_args(B, H, K):
    args = mpg_args('TD3', B, H)                       # the two-critic namespace; what built_SAC_parser sets differently:
    args.alg_name, args.learner_version = 'SAC', 'SAC'
    args.delay_update, args.deterministic_policy, args.policy_out_activation = 1, False, 'linear'
    args.alpha, args.alpha_lr_schedule, args.explore_sigma = ALPHA, [8e-5, 100000, 8e-6], None
    args.gradient_clip_norm = CLIP
    if K:
        args.num_future_data, args.obs_dim, args.obs_scale = K, 6 + K, G.OBS_SCALE_PT + [1.] * K
    return args


def unclipped(norm):
    return float(norm)          # tf.clip_by_global_norm returns the norm BEFORE the clip


def fx_sac(H, B, K, seed, lean):
    inject()
    from learners.sac import SACLearner
    from policy import PolicyWithQs
    rng = np.random.Generator(np.random.PCG64(seed))
    args = sac_args(B, H, K)
    nets = {'policy': mlp_weights_list(rng, 6 + K, H, 4), 'Q1': mlp_weights_list(rng, 8 + K, H, 1), 'Q2': mlp_weights_list(rng, 8 + K, H, 1)}
    add_targets(nets)
    batch = make_replay_batch_pt(rng, B, K)
    eps_t, eps_p = rng.standard_normal((B, 2)).astype(np.float32), rng.standard_normal((B, 2)).astype(np.float32)
    out = dict(batch_obs=batch[0], batch_actions=batch[1], batch_rewards=batch[2], batch_obs_tp1=batch[3], batch_dones=batch[4],
               target_scale=G.TARGET_SCALE, weights_seed=np.array(seed), eps_target=eps_t, eps_policy=eps_p)
    full = {}
    for tag, dt in (('', torch.float32), ('_f64', torch.float64)):
        tf.set_ref_dtype(dt)
        learner = SACLearner(PolicyWithQs, args)
        pw = learner.policy_with_value
        set_policy_weights(pw, nets)
        tf.set_noise_source(NoiseStream([eps_t, eps_p]))
        grads = learner.compute_gradient(batch, None, None, 0)
        st = learner.get_stats()
        full[tag] = [np.asarray(g, np.float64) for g in grads]
        out['grads' + tag] = flat(grads) if tag == '' else sub64(flat(grads), H)
        out['targets' + tag] = np.asarray(learner.batch_data['batch_targets'])
        for key in STATS:
            out[key + tag] = np.asarray(st[key])
        # logp of both draws, from the reference's own compute_action on the same noise
        po = [learner.preprocessor.tf_process_obses(batch[i]).numpy() for i in (3, 0)]
        tf.set_noise_source(NoiseStream([eps_t, eps_p]))
        out['logp_target' + tag] = np.asarray(pw.compute_action(po[0])[1])
        out['logp_policy' + tag] = np.asarray(pw.compute_action(po[1])[1])
        for k in ('targets', 'logp_target', 'logp_policy'):
            full[k + tag] = np.asarray(out[k + tag], np.float64)
    # the float64 values of the arrays shorter than 8 entries (yardstick.check_gradients small64): the three output biases
    out['small64'] = np.concatenate([g.ravel() for g in full['_f64'] if g.size < 8])
    tf.set_ref_dtype(torch.float32)
    tf.set_noise_source(None)
    rel = [np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30) for a, b in zip(full[''], full['_f64'])]
    rel_v = [np.linalg.norm(full[k] - full[k + '_f64']) / np.linalg.norm(full[k + '_f64']) for k in ('targets', 'logp_target', 'logp_policy')]
    qn1, qn2, pn = [unclipped(out[k]) for k in ('q_gradient_norm1', 'q_gradient_norm2', 'policy_gradient_norm')]
    print('sac H %d K %d seed %d: reference float32 vs float64, rel L2 per array: %s   (max %.1e); targets %.1e logp %.1e %.1e; '
          'norms Q1 %.2f Q2 %.2f policy %.2f' % (H, K, seed, ' '.join('%.1e' % r for r in rel), max(rel), rel_v[0], rel_v[1], rel_v[2],
                                                 qn1, qn2, pn))
    ok = max(max(rel), max(rel_v)) <= QUARTER_BAR and max(qn1, qn2) > CLIP and pn < CLIP
    if ok:
        if lean:
            for k, v in fixture_weights(seed, K, H).items():
                assert np.array_equal(flat(nets[k]), v), k
        else:
            for k in ('policy', 'Q1', 'Q2'):
                out['w_' + k] = flat(nets[k])
        path = os.path.join(HERE, 'sac_H%d_B%d%s.npz' % (H, B, '_K%d' % K if K else ''))
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) <= 1 << 20, (path, os.path.getsize(path))
    return ok


def fx_parser_defaults():
    """built_SAC_parser() as it lies (train_script.py:672-792): argparse defaults, nothing on the command line"""
    sys.path.insert(0, os.path.join(G.REF, 'train_scripts'))
    argv, sys.argv = sys.argv, sys.argv[:1]
    cwd = os.getcwd()
    try:
        os.chdir(os.path.join(G.REF, 'train_scripts'))
        import train_script
        d = vars(train_script.built_SAC_parser())
    finally:
        sys.argv = argv
        os.chdir(cwd)
    for k in ('result_dir', 'log_dir', 'model_dir'):        # time-stamped paths
        d.pop(k)
    with open(os.path.join(HERE, 'sac_parser_defaults.json'), 'w') as fh:
        json.dump(d, fh, indent=1, sort_keys=True)
        fh.write('\n')


def main():
    torch.manual_seed(0)
    for H, K, lean in ((256, 0, True), (256, 3, True), (32, 0, False)):
        assert any(fx_sac(H, 64, K, seed, lean) for seed in SEEDS), 'no seed of the list meets the conditions (H %d, K %d)' % (H, K)
    fx_parser_defaults()


if __name__ == '__main__':
    main()
