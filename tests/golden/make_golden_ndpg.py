"""Writes the n-step DPG fixtures from the UNMODIFIED reference (beside make_golden.py, whose helpers it uses):

    ndpg_H256_B64.npz        learners.ndpg.NDPGLearner.compute_gradient, PathTracking-v0, num_future_data 0
    ndpg_H256_B64_K3.npz     the same with num_future_data = 3 (obs_dim 9)
    ndpg_H32_B64.npz         32-unit nets (CPU tests only; keeps its weights, it is tiny)
    ndpg_parser_defaults.json    what train_scripts/train_script.py:built_NDPG_parser() returns (settings only; the time-stamped
                                 result / log / model directories left out)

    MPG_REFERENCE=/path/to/reference python tests/golden/make_golden_ndpg.py

The H = 256 files are lean (at most 1 MiB each): they store `weights_seed` instead of the weights - tests/ndpg_oracle.py
fixture_weights(seed, K) regenerates them in the same draw order (`policy`, then `Q1`; asserted equal here) - the float32 gradients
completely and every 8th element of the float64 ones (make_golden.sub64).

The generator checks its own draw, like make_golden_dp.py: a case is written for the first seed of a fixed list for which the
reference's float32 run is within a QUARTER of the 1e-4 bar of tests/yardstick.py from its float64 run on the targets and on every
gradient array, and whose un-clipped critic gradient norm exceeds the clip norm 3 (so that the clip is exercised).  Both are
conditions on the reference alone; the figures of every seed tried are printed."""
import json
import os
import sys

import numpy as np

import make_golden as G                                 # noqa: E402
from make_golden import add_targets, flat, make_replay_batch_pt, mpg_args, set_policy_weights, sub64     # noqa: E402
from golden_inputs import mlp_weights_list              # noqa: E402  (make_golden put tests/ on the path)
from tests.ndpg_oracle import STATS, fixture_weights    # noqa: E402  (make_golden put the repository root on the path too)

torch, tf = G.torch, G.tf
HERE = G.HERE
QUARTER_BAR = 0.25e-4
SEEDS = {0: (92, 93, 94, 95, 96, 97), 3: (91, 92, 93, 94, 95, 96)}       # K -> the seeds tried, in order


def ndpg_args(B, H, K):
    args = mpg_args('MPG-v1', B, H)
    args.alg_name, args.double_Q, args.delay_update = 'NDPG', False, 1
    if K:
        args.num_future_data, args.obs_dim, args.obs_scale = K, 6 + K, G.OBS_SCALE_PT + [1.] * K
    return args


def fx_ndpg(H, B, K, seed, lean):
    from learners.ndpg import NDPGLearner
    from policy import PolicyWithQs
    rng = np.random.Generator(np.random.PCG64(seed))
    args = ndpg_args(B, H, K)
    nets = {'policy': mlp_weights_list(rng, 6 + K, H, 4), 'Q1': mlp_weights_list(rng, 8 + K, H, 1)}
    add_targets(nets)
    batch = make_replay_batch_pt(rng, B, K)
    out = dict(batch_obs=batch[0], batch_actions=batch[1], batch_rewards=batch[2], batch_obs_tp1=batch[3], batch_dones=batch[4],
               target_scale=G.TARGET_SCALE, weights_seed=np.array(seed))
    full = {}
    for tag, dt in (('', torch.float32), ('_f64', torch.float64)):
        tf.set_ref_dtype(dt)
        learner = NDPGLearner(PolicyWithQs, args)
        set_policy_weights(learner.policy_with_value, nets)
        grads = learner.compute_gradient(batch, None, None, 0)
        st = learner.get_stats()
        full[tag] = [np.asarray(g, np.float64) for g in grads]
        out['grads' + tag] = flat(grads) if tag == '' else sub64(flat(grads), H)
        out['targets' + tag] = np.asarray(learner.batch_data['batch_targets'])
        full['targets' + tag] = np.asarray(out['targets' + tag], np.float64)
        for key in STATS:
            out[key + tag] = np.asarray(st[key])
        if tag == '':
            out['td_error'] = np.asarray(learner.compute_td_error())
            ro = learner.sample(batch[0].astype(np.float32), batch[1].astype(np.float32))
            out['nstep_all_rewards'] = ro['all_rewards']
            out['nstep_last_obs'] = ro['all_obs_tp1'][-1]
    # the float64 values of the arrays shorter than 8 entries (yardstick.check_gradients small64): Q1's b3, the policy's b3
    out['small64'] = np.concatenate([g.ravel() for g in full['_f64'] if g.size < 8])
    tf.set_ref_dtype(torch.float32)
    rel = [np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30) for a, b in zip(full[''], full['_f64'])]
    rel_t = np.linalg.norm(full['targets'] - full['targets_f64']) / np.linalg.norm(full['targets_f64'])
    qn = float(out['q_gradient_norm'])
    print('ndpg H %d K %d seed %d: reference float32 vs float64, rel L2 per array: %s   (max %.1e); targets %.1e; Q norm %.2f'
          % (H, K, seed, ' '.join('%.1e' % r for r in rel), max(rel), rel_t, qn))
    ok = max(max(rel), rel_t) <= QUARTER_BAR and qn > 3.
    if ok:
        if lean:
            for k, v in fixture_weights(seed, K, H).items():
                assert np.array_equal(flat(nets[k]), v), k
        else:
            for k in ('policy', 'Q1'):
                out['w_' + k] = flat(nets[k])
        path = os.path.join(HERE, 'ndpg_H%d_B%d%s.npz' % (H, B, '_K%d' % K if K else ''))
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) <= 1 << 20, (path, os.path.getsize(path))
    return ok


def fx_parser_defaults():
    """built_NDPG_parser() as it lies (train_script.py:431-549): argparse defaults, nothing on the command line"""
    sys.path.insert(0, os.path.join(G.REF, 'train_scripts'))
    argv, sys.argv = sys.argv, sys.argv[:1]
    cwd = os.getcwd()
    try:
        os.chdir(os.path.join(G.REF, 'train_scripts'))
        import train_script
        d = vars(train_script.built_NDPG_parser())
    finally:
        sys.argv = argv
        os.chdir(cwd)
    for k in ('result_dir', 'log_dir', 'model_dir'):        # time-stamped paths
        d.pop(k)
    with open(os.path.join(HERE, 'ndpg_parser_defaults.json'), 'w') as fh:
        json.dump(d, fh, indent=1, sort_keys=True)
        fh.write('\n')


def main():
    torch.manual_seed(0)
    for H, K, lean in ((256, 0, True), (256, 3, True), (32, 0, False)):
        assert any(fx_ndpg(H, 64, K, seed, lean) for seed in SEEDS[K]), 'no seed of the list meets the conditions (H %d, K %d)' % (H, K)
    fx_parser_defaults()


if __name__ == '__main__':
    main()
