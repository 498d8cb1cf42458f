"""Writes the fixtures of MPG on InvertedPendulumConti-v0 from the UNMODIFIED reference (beside make_golden.py, whose helpers it uses):

    mpg_v1_pendulum_H256_B64.npz     learners.mpg_learner.MPGLearner.compute_gradient, MPG-v1 at built_MPG_parser's defaults
                                     (train_script4mujoco.py:169-293), B = 64, n = 25, at iterations 100 and 3000 (the rule-based weights
                                     differ under rule_based_bias_total_ite 4000); and from sample() / compute_n_step_target():
                                     `all_rewards`, `last_obs` (the last all_obs_tp1), `q_boot` (the UNclipped bootstrap values: the
                                     argument the reference hands to tf.clip_by_value, mpg_learner.py:163-164) and the targets
    mpg_v2_pendulum_H256_B64.npz     the same for MPG-v2: the clipped double-Q target, two critics, no env rollout
    (+ ..._it3000.npz)               the second iteration's policy gradient of a case whose one file would pass the 1 MiB limit of a
                                     committed file (`split` says so)
    mpg_mujoco_parser_defaults.json  what built_MPG_parser('MPG-v1') and ('MPG-v2') return (settings only; the time-stamped result /
                                     log / model directories left out)

    MPG_REFERENCE=/path/to/reference python tests/golden/make_golden_mpg_pendulum.py

Each case runs twice: float32 nets with a float32 env, float64 nets with a float64 env (`_f64`; gradients: every 8th element,
make_golden.sub64; value arrays complete).

THE ENV IS A STAND-IN.  InvertedPendulumConti-v0 is a MuJoCo environment and MuJoCo is absent, so the reference's
gym.make('InvertedPendulumConti-v0') is served by gym.register(...) with a small adapter around oracle.InvertedPendulumContiOracle(1,
dtype) - the closed-form cart-pole of the same model file, whose parity with MuJoCo is unpinned - that provides
the reset(), set_state(qpos, qvel) and step(a) the reference's utils/dummy_vec_env.py calls.  The reference's learner, its
DummyVecEnv, policy and model run as they are; what the fixture pins is the LEARNER on that env, on both sides of every comparison.

The files are lean: `weights_seed` instead of the weights (tests/mpg_pendulum_oracle.py fixture_weights regenerates them in the same
draw order; asserted equal here); the critics' float32 gradients are stored once (`q_grads`: they do not depend on the iteration,
asserted here), the policy's per iteration.  Fresh target critics give bootstrap values of one sign, so the TARGET critic Q1's output
layer is scaled and shifted (W3 * q_scale, b3 * q_scale + q_shift; both recorded) until the values straddle the clip interval.

Two CONDITIONS on the inputs, asserted here and again by tests/test_mpg_pendulum_golden.py - on the reference alone, the first seed of
a fixed list that meets them is written, the figures of every seed tried are printed:
  clip coverage    of the 64 unclipped bootstrap values at least 8 lie below -0.5, at least 8 inside [-0.5, 0], at least 8 above 0;
  amplification    the reference's float32 run is within a QUARTER of the 1e-4 bar of tests/yardstick.py from its float64 run on
                   `targets`, on `all_rewards` (and on every gradient array) - the pole is unstable over 25 steps, so the start states
                   are drawn from a narrow part of what the replay holds (|p| < 2, |theta| <= 0.2)."""
import json
import os
import sys

import numpy as np

import make_golden as G                                 # noqa: E402
from make_golden import NoiseStream, add_targets, flat, mpg_args, set_policy_weights, sub64     # noqa: E402
from golden_inputs import mlp_weights_list              # noqa: E402  (make_golden put tests/ on the path)
from tests import mpg_pendulum_oracle as P              # noqa: E402  (make_golden put the repository root on the path too)

torch, tf, O = G.torch, G.tf, G.O
HERE = G.HERE
QUARTER_BAR = 0.25e-4
SEEDS = (131, 132, 133, 134, 135, 136, 137, 138)
B, H = 64, 256
Q_SCALE, Q_SHIFT = np.float32(12.0), np.float32(-0.25)   # the target critic's output layer (module docstring)
SPREAD = np.array([0.5, 0.02, 0.1, 0.1])                 # start states: p, theta, pdot, thetadot (standard deviations)


def register_stand_in(dtype):
    import gym

    class StandIn(gym.Env):
        def __init__(self):
            self.sim = O.InvertedPendulumContiOracle(1, dtype=dtype)

        def reset(self):
            return self.sim.reset(init_obs=np.zeros((1, 4), dtype))[0]

        def set_state(self, qpos, qvel):
            self.sim.reset(init_obs=np.concatenate([np.asarray(qpos), np.asarray(qvel)])[np.newaxis, :])

        def step(self, a):
            obs, rew, done, info = self.sim.step(np.asarray(a, dtype).reshape(1, 1))
            return obs[0], rew[0], bool(done[0]), info
    gym.register('InvertedPendulumConti-v0', StandIn)


def pendulum_args(version):
    """built_MPG_parser(version)'s settings (fx_parser_defaults writes them out) with B = 64"""
    args = mpg_args(version, B, H, env=P.PEND)
    args.num_agent, args.rule_based_bias_total_ite = 1, P.TOTAL_ITE
    args.num_batch_reuse = 10 if version == 'MPG-v1' else 1
    return args


def replay_batch(rng):
    """transitions of the stand-in env itself: start states from the narrow middle of what the replay holds, actions 3 tanh(.) plus the
    worker's 0.1 exploration noise (some beyond the control clamp +-3)"""
    obs = (rng.standard_normal((B, 4)) * SPREAD).astype(np.float32)
    act = (3. * np.tanh(1.5 * rng.standard_normal((B, 1))) + 0.1 * rng.standard_normal((B, 1))).astype(np.float32)
    env = O.InvertedPendulumContiOracle(B, dtype=np.float32)
    env.reset(init_obs=obs)
    obs2, rew, done, _ = env.step(act)
    return [obs, act, rew.astype(np.float32), obs2.astype(np.float32), done.astype(np.float32)]


def rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def coverage(q):
    q = np.asarray(q)
    return int((q < P.Q_LO).sum()), int(((q >= P.Q_LO) & (q <= P.Q_HI)).sum()), int((q > P.Q_HI).sum())


def fx(version, seed):
    from learners.mpg_learner import MPGLearner
    from policy import PolicyWithQs
    v1 = version == 'MPG-v1'
    rng = np.random.Generator(np.random.PCG64(seed))
    args = pendulum_args(version)
    nets = {'policy': mlp_weights_list(rng, 4, H, 2), 'Q1': mlp_weights_list(rng, 5, H, 1)}
    if not v1:
        nets['Q2'] = mlp_weights_list(rng, 5, H, 1)
    add_targets(nets)
    q_scale, q_shift = (Q_SCALE, Q_SHIFT) if v1 else (np.float32(1.), np.float32(0.))
    t = nets['Q1_target']
    t[4] = (t[4] * q_scale).astype(np.float32)
    t[5] = (t[5] * q_scale + q_shift).astype(np.float32)
    batch = replay_batch(rng)
    eps = rng.standard_normal((25, B)).astype(np.float32)
    out = dict(batch_obs=batch[0], batch_actions=batch[1], batch_rewards=batch[2], batch_obs_tp1=batch[3], batch_dones=batch[4], eps=eps,
               iterations=np.array(P.ITERATIONS), target_scale=G.TARGET_SCALE, weights_seed=np.array(seed), q_scale=q_scale, q_shift=q_shift)
    n_q = len(P.names_of(version)) * 6
    full = {}
    for tag, dt in (('', torch.float32), ('_f64', torch.float64)):
        tf.set_ref_dtype(dt)
        register_stand_in(np.float32 if tag == '' else np.float64)
        learner = MPGLearner(PolicyWithQs, args)
        set_policy_weights(learner.policy_with_value, nets)
        for it in P.ITERATIONS:
            learner.counter = 0
            tf.set_noise_source(NoiseStream(list(eps)))
            grads = learner.compute_gradient(batch, None, None, it)
            st = learner.get_stats()
            p = 'it%d_' % it
            full[p + 'grads' + tag] = [np.asarray(g, np.float64) for g in grads]
            if tag == '':
                if it == P.ITERATIONS[0]:
                    out['q_grads'] = flat(grads[:n_q])
                else:
                    assert np.array_equal(out['q_grads'], flat(grads[:n_q])), 'the critic gradients depend on the iteration'
                out[p + 'policy_grads'] = flat(grads[n_q:])
            else:
                out[p + 'grads_f64'] = sub64(flat(grads), H)
            out[p + 'targets' + tag] = np.asarray(learner.batch_data['batch_targets'])
            for key in P.STATS:
                if key in st:
                    out[p + key + tag] = np.asarray(st[key])
            out[p + 'w_list' + tag] = np.asarray(st['w_list'])
            out[p + 'all_losses' + tag] = np.asarray(st['all_losses'])
            # the float64 values of the arrays shorter than 8 entries (yardstick.check_gradients small64): the output biases
            if tag == '_f64':
                out[p + 'small64'] = np.concatenate([g.ravel() for g in full[p + 'grads_f64'] if g.size < 8])
        assert np.array_equal(out['it%d_targets%s' % (P.ITERATIONS[0], tag)], out['it%d_targets%s' % (P.ITERATIONS[1], tag)])
        out['targets' + tag] = out.pop('it%d_targets%s' % (P.ITERATIONS[0], tag))
        del out['it%d_targets%s' % (P.ITERATIONS[1], tag)]
        if v1:
            ro = learner.sample(batch[0].astype(np.float32), batch[1].astype(np.float32))
            out['all_rewards' + tag] = ro['all_rewards']
            out['last_obs' + tag] = ro['all_obs_tp1'][-1]
            seen, clip = [], tf.clip_by_value
            tf.clip_by_value = lambda x, lo, hi, name=None: (seen.append((np.array(x), lo, hi)), clip(x, lo, hi))[1]
            try:
                again = learner.compute_n_step_target()
            finally:
                tf.clip_by_value = clip
            assert len(seen) == 1 and seen[0][1:] == (P.Q_LO, P.Q_HI) and np.array_equal(np.asarray(again), out['targets' + tag])
            out['q_boot' + tag] = np.asarray(seen[0][0][-1], np.float32)
        if tag == '':
            out['td_error'] = np.asarray(learner.compute_td_error())
    tf.set_ref_dtype(torch.float32)
    tf.set_noise_source(None)
    worst_g = max(rel(a, b) for it in P.ITERATIONS for a, b in zip(full['it%d_grads' % it], full['it%d_grads_f64' % it]))
    figures = dict(targets=rel(out['targets'], out['targets_f64']), grads=worst_g)
    ok = True
    if v1:
        figures['all_rewards'] = rel(out['all_rewards'], out['all_rewards_f64'])
        cov = coverage(out['q_boot'])
        ok = min(cov) >= 8 and min(coverage(out['q_boot_f64'])) >= 8
        print('%s seed %d: unclipped bootstrap values below / inside / above [-0.5, 0]: %s' % (version, seed, cov))
    print('%s seed %d: reference float32 vs float64, rel L2: %s' % (version, seed, '  '.join('%s %.1e' % kv for kv in figures.items())))
    ok = ok and max(figures.values()) <= QUARTER_BAR
    if ok:
        for k, v in P.fixture_weights(seed, version, H).items():
            assert np.array_equal(flat(nets[k]), v), k
        for k, v in P.fixture_targets(P.fixture_weights(seed, version, H), G.TARGET_SCALE, q_scale, q_shift, H).items():
            assert np.array_equal(flat(nets[k + '_target']), v), k
        path = os.path.join(HERE, 'mpg_%s_pendulum_H%d_B%d.npz' % (version[-2:], H, B))
        late_key = 'it%d_policy_grads' % P.ITERATIONS[1]
        out['split'] = np.array(0)
        np.savez_compressed(path, **out)
        late_path = path[:-4] + '_it%d.npz' % P.ITERATIONS[1]
        if os.path.getsize(path) > 1 << 20:
            out['split'] = np.array(1)
            np.savez_compressed(late_path, **{late_key: out.pop(late_key)})
            np.savez_compressed(path, **out)
            assert os.path.getsize(late_path) <= 1 << 20
        elif os.path.exists(late_path):
            os.remove(late_path)
        assert os.path.getsize(path) <= 1 << 20, (path, os.path.getsize(path))
    return ok


def fx_parser_defaults():
    """built_MPG_parser(version) as it lies (train_script4mujoco.py:169-293): argparse defaults, nothing on the command line"""
    sys.path.insert(0, os.path.join(G.REF, 'train_scripts'))
    argv, sys.argv = sys.argv, sys.argv[:1]
    cwd = os.getcwd()
    out = {}
    try:
        os.chdir(os.path.join(G.REF, 'train_scripts'))
        import train_script4mujoco
        for version in ('MPG-v1', 'MPG-v2'):
            d = vars(train_script4mujoco.built_MPG_parser(version))
            for k in ('result_dir', 'log_dir', 'model_dir'):        # time-stamped paths
                d.pop(k)
            out[version] = d
    finally:
        sys.argv = argv
        os.chdir(cwd)
    with open(os.path.join(HERE, 'mpg_mujoco_parser_defaults.json'), 'w') as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write('\n')


def main():
    torch.manual_seed(0)
    for version in ('MPG-v1', 'MPG-v2'):
        assert any(fx(version, seed) for seed in SEEDS), 'no seed of the list meets the conditions (%s)' % version
    fx_parser_defaults()


if __name__ == '__main__':
    main()
