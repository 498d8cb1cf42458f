"""Writes the AMPC fixtures from the UNMODIFIED reference (beside make_golden.py and make_golden_dp.py, whose helpers it uses):

    ampc_H256_B64.npz          learners.ampc.AMPCLearner.compute_gradient, PathTracking-v0, n = 25, M = 1, num_future_data 0
    ampc_H256_B64_K3_M2.npz    num_future_data = 3 (obs_dim 9), M = 2 copies of 32 start observations, n = 10
    ampc_dp_H256_B64_n10.npz   InvertedDoublePendulum-v2 (this project's settings for the env, make_golden_dp.dp_args), n = 10
    ampc_parser_defaults.json  what train_scripts/train_script.py:built_AMPC_parser() returns (settings only; the time-stamped
                               result / log / model directories left out)

    MPG_REFERENCE=/path/to/reference python tests/golden/make_golden_ampc.py

learners/ampc.py and policy.py (policy_only=True) run as they are over the stand-in `tensorflow` (oracle/refshim), in float32 and in
float64; the model's noise draws (path_tracking_env.py:119) are recorded as `eps` [n, M * B] and fed back in call order.

The files are lean: `weights_seed` instead of the weights (tests/ampc_oracle.py fixture_weights regenerates them; asserted equal
here), the float32 gradient completely and every 8th element of the float64 one (make_golden.sub64).

The generator checks its own draw, like make_golden_dp.py and make_golden_ndpg.py: a case is written for the first seed of a fixed
list for which the reference's float32 run is within HALF of the 1e-4 bar of tests/yardstick.py from its float64 run on every
gradient array and both statistics - a condition on the reference alone; the figures of every seed tried are printed.

The clip: built_AMPC_parser's gradient_clip_norm is 3.  CLIP below is the norm each case was made with; main() asserts that at least
one case's un-clipped gradient norm lies above its clip, so that the clip is exercised."""
import json
import os
import sys

import numpy as np

import make_golden as G                                 # noqa: E402
import make_golden_dp as GDP                            # noqa: E402  (tf.atan2 for the stand-in, the Agg backend, start_obs, dp_args)
from make_golden import flat, make_replay_batch_pt, mpg_args, set_policy_weights, sub64     # noqa: E402
from golden_inputs import mlp_weights_list              # noqa: E402  (make_golden put tests/ on the path)
from tests import ampc_oracle as A                      # noqa: E402  (make_golden put the repository root on the path too)

torch, tf = G.torch, G.tf
HERE = G.HERE
HALF_BAR = 0.5e-4
STATS = A.STATS
# name -> (env, K, rows, M, n, clip, the seeds tried in order)
CASES = {
    'ampc_H256_B64.npz': ('PathTracking-v0', 0, 64, 1, 25, 3., (110, 111, 112, 113, 114, 115)),
    'ampc_H256_B64_K3_M2.npz': ('PathTracking-v0', 3, 32, 2, 10, 3., (120, 121, 122, 123, 124, 125)),
    'ampc_dp_H256_B64_n10.npz': (GDP.ENV_ID, 0, 64, 1, 10, 3., (130, 131, 132, 133, 134, 135)),
}


def ampc_args(env, B, H, K, M, n, clip):
    """built_AMPC_parser's settings (policy_only, no critic, no target: double_Q / target False, tau / delay_update None; gamma 1)"""
    args = GDP.dp_args(B, H, n) if env == GDP.ENV_ID else mpg_args('MPG-v2', B, H)
    args.alg_name, args.learner_version = 'AMPC', None
    args.policy_only, args.double_Q, args.target, args.tau, args.delay_update = True, False, False, None, None
    args.gamma, args.M, args.gradient_clip_norm = 1., M, clip
    args.num_rollout_list_for_policy_update, args.num_rollout_list_for_q_estimation = [n], []
    if K:
        args.num_future_data, args.obs_dim, args.obs_scale = K, 6 + K, G.OBS_SCALE_PT + [1.] * K
    return args


def fx_ampc(name, seed, H=256):
    from learners.ampc import AMPCLearner
    from policy import PolicyWithQs
    env, K, B, M, n, clip, _ = CASES[name]
    rng = np.random.Generator(np.random.PCG64(seed))
    args = ampc_args(env, B, H, K, M, n, clip)
    cfg = A.make_cfg(env, K, n=n, M=M, clip=clip, H=H)
    nets = {'policy': mlp_weights_list(rng, cfg.obs_dim, H, 2 * cfg.act_dim)}
    if env == GDP.ENV_ID:
        obs = GDP.start_obs(rng, B)
        act = np.zeros((B, 1), np.float32)
        eps = None                                      # the model draws no noise
    else:
        obs, act = make_replay_batch_pt(rng, B, K)[:2]
        eps = rng.standard_normal((n, M * B)).astype(np.float32)
    batch = [obs, act, np.zeros(B, np.float32), obs.copy(), np.zeros(B, np.float32)]
    out = dict(batch_obs=obs, weights_seed=np.array(seed), n=np.int32(n), M=np.int32(M), clip=np.float32(clip))
    if eps is not None:
        out['eps'] = eps
    full = {}
    for tag, dt in (('', torch.float32), ('_f64', torch.float64)):
        tf.set_ref_dtype(dt)
        learner = AMPCLearner(PolicyWithQs, args)
        assert [m.name for m in learner.policy_with_value.models] == ['policy'] and not learner.policy_with_value.target_models
        set_policy_weights(learner.policy_with_value, nets)
        if eps is not None:
            stream = G.NoiseStream(list(eps))
            tf.set_noise_source(stream)
        grads = learner.compute_gradient(batch, None, None, 0)
        if eps is not None:
            assert stream.k == n, (stream.k, n)         # one draw per model step, nothing else draws
        st = learner.get_stats()
        full[tag] = [np.asarray(g, np.float64) for g in grads]
        out['grads' + tag] = flat(grads) if tag == '' else sub64(flat(grads), H)
        for key in STATS:
            out[key + tag] = np.asarray(st[key])
    tf.set_ref_dtype(torch.float32)
    tf.set_noise_source(None)
    # the float64 values of the arrays shorter than 8 entries (yardstick.check_gradients small64): the policy's b3
    out['small64'] = np.concatenate([g.ravel() for g in full['_f64'] if g.size < 8])
    rel = [np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30) for a, b in zip(full[''], full['_f64'])]
    srel = {k: abs(float(out[k]) - float(out[k + '_f64'])) / abs(float(out[k + '_f64'])) for k in STATS}
    norm = float(out['policy_gradient_norm_f64'])
    print('%s seed %d: reference float32 vs float64, rel L2 per array: %s   (max %.1e); %s; un-clipped norm %.3f (clip %.1f)'
          % (name, seed, ' '.join('%.1e' % r for r in rel), max(rel), ' '.join('%s %.1e' % kv for kv in srel.items()), norm, clip))
    ok = max(max(rel), max(srel.values())) <= HALF_BAR
    if ok:
        assert np.array_equal(flat(nets['policy']), A.fixture_weights(seed, cfg)['policy'])
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) <= 1 << 20, (path, os.path.getsize(path))
    return ok, norm > clip


def fx_parser_defaults():
    """built_AMPC_parser() as it lies (train_script.py:57-175): argparse defaults, nothing on the command line"""
    sys.path.insert(0, os.path.join(G.REF, 'train_scripts'))
    argv, sys.argv = sys.argv, sys.argv[:1]
    cwd = os.getcwd()
    try:
        os.chdir(os.path.join(G.REF, 'train_scripts'))
        import train_script
        d = vars(train_script.built_AMPC_parser())
    finally:
        sys.argv = argv
        os.chdir(cwd)
    for k in ('result_dir', 'log_dir', 'model_dir'):        # time-stamped paths
        d.pop(k)
    with open(os.path.join(HERE, 'ampc_parser_defaults.json'), 'w') as fh:
        json.dump(d, fh, indent=1, sort_keys=True)
        fh.write('\n')


def main():
    torch.manual_seed(0)
    clipped = []
    for name, case in CASES.items():
        for seed in case[-1]:
            ok, above = fx_ampc(name, seed)
            if ok:
                clipped.append(above)
                break
        else:
            raise AssertionError('no seed of the list meets the conditions (%s)' % name)
    assert any(clipped), 'no case exercises the clip: choose a smaller CLIP for one of them'
    fx_parser_defaults()


if __name__ == '__main__':
    main()
