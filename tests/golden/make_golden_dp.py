"""Writes the InvertedDoublePendulum-v2 fixtures from the UNMODIFIED reference (beside make_golden.py, whose helpers it uses):

    double_pendulum_model_ref.npz        InvertedDoublePendulumModel.reset + 25 x rollout_out on 64 start observations
    nadp_dp_H{32,256}_B64_inputs.npz     weights and batch of the NADP cases (shared by both horizons)
    nadp_dp_H{32,256}_B64.npz            NADPLearner.compute_gradient, model horizon 25
    nadp_dp_H{32,256}_B64_n10.npz        the same at horizon 10 (|theta| < 3.6 throughout: tells a wrong formula from the
                                         error growth of the falling pendulum at 25)

    MPG_REFERENCE=/path/to/reference python tests/golden/make_golden_dp.py

The stand-in `tensorflow` (oracle/refshim) has no atan2, which the model's reset needs: it is added to the imported module in
this process.  The model's constructor calls plt.ion(): the Agg backend is selected first.  The reference ships no parser for this
env; obs_scale = ones, rew_scale 1, linear policy output with action_range 1 ("actions are in range [-1, 1]",
inverted_double_pendulum_model.py:134) are this project's choice (mpg_amd.ops.make_cfg)."""
import os

import matplotlib
matplotlib.use('Agg')
import numpy as np                                      # noqa: E402

import make_golden as G                                 # noqa: E402
from make_golden import add_targets, flat, mlp_weights, mpg_args, set_policy_weights, sub64     # noqa: E402

torch, tf = G.torch, G.tf
tf.atan2 = lambda y, x: torch.atan2(tf._wrap(y), tf._wrap(x))
HERE = G.HERE
ENV_ID = 'InvertedDoublePendulum-v2'
STATS = ('q_loss', 'policy_loss', 'value_mean', 'q_gradient_norm', 'policy_gradient_norm')
# The tolerance rule of tests/yardstick.py judges an implementation by the reference's own float32 error and presupposes that the
# reference alone stays inside the 1e-4 bar.  On this model that is a property of the DRAW: the pendulum falls within 25 steps and
# rounding differences grow along the trajectory, so for about one seed in six the reference's float32 policy-gradient NORM is
# 2e-4 .. 3e-4 from its float64 run (the clipped arrays, being directions, stay within 3e-5).  A case is therefore written for the
# first seed, counting up from its base, for which the reference's float32 run is within HALF the bar of its float64 run on every
# array and every statistic - a condition on the reference alone; the figures of every seed tried are printed.
HALF_BAR = 0.5e-4


def start_obs(rng, B):
    """gym's InvertedDoublePendulumEnv.reset_model law from a seeded Generator: qpos ~ U(-0.1, 0.1), qvel ~ 0.1 N(0, 1); the three
    constraint-force entries ~ 0.1 N(0, 1) (non-zero on purpose: only so can a test see that the START observation's entries
    reach the networks while the model observations carry zeros)."""
    p = rng.uniform(-0.1, 0.1, B)
    th = rng.uniform(-0.1, 0.1, (B, 2))
    v = rng.standard_normal((B, 3)) * 0.1
    frc = rng.standard_normal((B, 3)) * 0.1
    return np.concatenate([p[:, None], np.sin(th), np.cos(th), v, frc], 1).astype(np.float32)


def dp_args(B, H, n):
    args = mpg_args('NADP', B, H, env='InvertedPendulumConti-v0')
    args.env_id = ENV_ID
    args.obs_dim, args.act_dim = 11, 1
    args.obs_scale = [1.] * 11
    args.rew_scale, args.rew_shift = 1., 0.
    args.policy_out_activation, args.action_range = 'linear', 1.
    args.num_rollout_list_for_policy_update = [n]
    args.num_rollout_list_for_q_estimation = [n]
    args.delay_update = 1
    return args


def fx_dp_model(N=64, T=25, seed=90):
    from envs_and_models.inverted_double_pendulum_model import InvertedDoublePendulumModel
    rng = np.random.Generator(np.random.PCG64(seed))
    obs0 = start_obs(rng, N)
    actions = rng.uniform(-1, 1, (T, N, 1)).astype(np.float32)
    out = dict(obs0=obs0, actions=actions)
    for tag, dt in (('', torch.float32), ('_f64', torch.float64)):
        tf.set_ref_dtype(dt)
        m = InvertedDoublePendulumModel()
        m.reset(tf.constant(obs0))
        out['state0' + tag] = m.states.numpy()
        obs_l, rew_l = [], []
        for t in range(T):
            o, r = m.rollout_out(tf.constant(actions[t]))
            obs_l.append(o.numpy()), rew_l.append(r.numpy())
        out['obs' + tag] = np.stack(obs_l)
        out['reward' + tag] = np.stack(rew_l)
        out['state' + tag] = m.states.numpy()
    tf.set_ref_dtype(torch.float32)
    np.savez_compressed(os.path.join(HERE, 'double_pendulum_model_ref.npz'), **out)


def fx_nadp_dp(H, B, n, seed):
    from learners.nadp import NADPLearner
    from policy import PolicyWithQs
    rng = np.random.Generator(np.random.PCG64(seed))
    args = dp_args(B, H, n)
    nets = {'policy': mlp_weights(rng, 11, H, 2), 'Q1': mlp_weights(rng, 12, H, 1)}
    add_targets(nets)
    obs = start_obs(rng, B)
    act = rng.uniform(-1, 1, (B, 1)).astype(np.float32)
    batch = [obs, act, np.zeros(B, np.float32), obs.copy(), np.zeros(B, np.float32)]
    # the seed fixes weights and batch whatever the horizon: they are written once per H (and keep every file below 1 MiB)
    inputs = dict(batch_obs=obs, batch_actions=act, target_scale=G.TARGET_SCALE)
    for k, v in nets.items():
        if not k.endswith('_target'):
            inputs['w_' + k] = flat(v)
    np.savez_compressed(os.path.join(HERE, 'nadp_dp_H%d_B%d_inputs.npz' % (H, B)), **inputs)
    out = dict(n=np.int32(n))
    full = {}
    for tag, dt in (('', torch.float32), ('_f64', torch.float64)):
        tf.set_ref_dtype(dt)
        learner = NADPLearner(PolicyWithQs, args)
        set_policy_weights(learner.policy_with_value, nets)
        grads = learner.compute_gradient(batch, None, None, 0)
        st = learner.get_stats()
        full[tag] = [np.asarray(g, np.float64) for g in grads]
        out['grads' + tag] = flat(grads) if tag == '' else sub64(flat(grads), H)
        for key in STATS:
            out[key + tag] = np.asarray(st[key])
        out['final_state' + tag] = learner.model.states.numpy()
        out['targets' + tag] = learner.model_rollout_for_q_estimation(tf.constant(obs), tf.constant(act)).numpy()
    # the float64 values of the arrays shorter than 8 entries (yardstick.check_gradients small64): Q1's b3, the policy's b3
    out['small64'] = np.concatenate([g.ravel() for g in full['_f64'] if g.size < 8])
    tf.set_ref_dtype(torch.float32)
    rel = [np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30) for a, b in zip(full[''], full['_f64'])]
    srel = {k: abs(float(out[k]) - float(out[k + '_f64'])) / abs(float(out[k + '_f64'])) for k in STATS}
    th = np.abs(out['final_state_f64'][:, 1:3]).max()
    print('nadp_dp H %d n %d seed %d: reference float32 vs float64, rel L2 per array: %s   (max %.1e; final |theta| max %.2f)'
          % (H, n, seed, ' '.join('%.1e' % r for r in rel), max(rel), th))
    print('    statistics: %s' % ' '.join('%s %.1e' % kv for kv in srel.items()))
    worst = max(max(rel), max(srel.values()))
    if worst <= HALF_BAR:
        np.savez_compressed(os.path.join(HERE, 'nadp_dp_H%d_B%d%s.npz' % (H, B, '' if n == 25 else '_n%d' % n)), **out)
    return worst


def main():
    torch.manual_seed(0)
    fx_dp_model()
    for H, base in ((32, 91), (256, 92)):
        seed = base
        while fx_nadp_dp(H, 64, 25, seed) > HALF_BAR:         # (measured: 91 holds it; 92 does not - norm 2.9e-4 - 93 does)
            seed += 1
        assert fx_nadp_dp(H, 64, 10, seed) <= HALF_BAR       # same weights and batch at the short horizon


if __name__ == '__main__':
    main()
