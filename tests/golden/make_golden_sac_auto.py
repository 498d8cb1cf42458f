"""Writes the fixtures of SAC with the LEARNED temperature (alpha = 'auto') from the UNMODIFIED reference, beside make_golden_sac.py,
whose helpers it uses:

    sac_auto_H256_B64.npz         learners.sac.SACLearner.compute_gradient, alpha 'auto', target_entropy -2, num_future_data 0
    sac_auto_H256_B64_K3.npz      the same with num_future_data = 3 (obs_dim 9)
    sac_auto_H32_B64.npz          32-unit nets (CPU tests only; keeps its weights, it is tiny)
    sac_auto_loop_H32_B64.npz     six iterations of the reference's own compute_gradient + PolicyWithQs.apply_gradients on one batch,
                                  delay_update 2, fresh recorded noise per call: per iteration log_alpha, the temperature's gradient
                                  and its norm; at the end the parameters and targets

    MPG_REFERENCE=/path/to/reference python tests/golden/make_golden_sac_auto.py

The reference's learners/sac.py and policy.py run as they are.  Two things are put into the stand-in packages under oracle/refshim at
run time, here:
  - tfp.distributions.MultivariateNormalDiag, as make_golden_sac.py does (its docstring);
  - keras.Model.trainable_weights is wrapped so that a model with a `log_alpha` attribute (model.py:46-49 AlphaModel, which has no
    layer) lists that variable.  Keras tracks a tf.Variable assigned to a Model attribute as a trainable weight; the stand-in's Model
    tracks layers only, so without the wrapper tape.gradient(alpha_loss, alpha_model.trainable_weights) (sac.py:147) has nothing to
    differentiate.  That is Keras' documented behaviour, not Keras' code: an inherent pin, like the Adam restatement of the loop
    fixtures.
log_alpha starts at float32(log 0.2), so that alpha is neither 1 nor the fixed 0.03.  THREE recorded draws per compute_gradient
call, in the order the reference makes them: `eps_target` (sac.py:71), `eps_policy` (:123), `eps_alpha` (:142).

Self-checks, on the reference alone; a case is written for the first seed of a fixed list for which
  - the float32 run is within a QUARTER of the 1e-4 bar of tests/yardstick.py from its float64 run on every gradient array, the
    targets, the three logp arrays and the temperature's gradient;
  - at gradient_clip_norm 1.0 the temperature's |g| is above the clip (target_entropy -2);
and one further small case with target_entropy 3.0 must put |g| below the clip (kept in the H = 32 file as `small_*`)."""
import os

import numpy as np

import make_golden as G                                 # noqa: E402
from make_golden import NoiseStream, add_targets, flat, make_replay_batch_pt, set_policy_weights, sub64     # noqa: E402
from make_golden_sac import QUARTER_BAR, SEEDS, inject, sac_args              # noqa: E402
from golden_inputs import mlp_weights_list              # noqa: E402
from tests.sac_auto_oracle import ALPHA_LR, LOG_ALPHA0, STATS             # noqa: E402
from tests.sac_oracle import CLIP, fixture_weights      # noqa: E402

torch, tf = G.torch, G.tf
HERE = G.HERE
TARGET_ENTROPY = -2.0


def inject_alpha():
    inject()
    from tensorflow import keras
    prop = keras.Model.trainable_weights
    if getattr(prop.fget, '_lists_log_alpha', False):
        return

    def trainable_weights(self):
        ws = prop.fget(self)
        return ws + [self.log_alpha] if hasattr(self, 'log_alpha') else ws
    trainable_weights._lists_log_alpha = True
    keras.Model.trainable_weights = property(trainable_weights)


def auto_args(B, H, K, target_entropy=TARGET_ENTROPY, **kw):
    args = sac_args(B, H, K)
    args.alpha, args.target_entropy, args.alpha_lr_schedule = 'auto', target_entropy, list(ALPHA_LR)
    for k, v in kw.items():
        setattr(args, k, v)
    return args


def draw_nets(rng, H, K):
    nets = {'policy': mlp_weights_list(rng, 6 + K, H, 4), 'Q1': mlp_weights_list(rng, 8 + K, H, 1), 'Q2': mlp_weights_list(rng, 8 + K, H, 1)}
    add_targets(nets)
    nets['alpha'] = [np.array(LOG_ALPHA0, np.float32)]
    return nets


def run_once(args, nets, batch, eps3, dt):
    """one compute_gradient of a fresh reference learner at dtype dt: (learner, 19 arrays, stats)"""
    from learners.sac import SACLearner
    from policy import PolicyWithQs
    tf.set_ref_dtype(dt)
    learner = SACLearner(PolicyWithQs, args)
    set_policy_weights(learner.policy_with_value, nets)
    tf.set_noise_source(NoiseStream(list(eps3)))
    grads = learner.compute_gradient(batch, None, None, 0)
    assert len(grads) == 19
    w = learner.policy_with_value.get_weights()
    assert [len(x) for x in w] == [6, 6, 6, 1, 6, 6, 6], [len(x) for x in w]          # [Q1, Q2, policy, [log_alpha], targets...]
    return learner, grads, learner.get_stats()


def fx_auto(H, B, K, seed, lean):
    inject_alpha()
    rng = np.random.Generator(np.random.PCG64(seed))
    args = auto_args(B, H, K)
    nets = draw_nets(rng, H, K)
    batch = make_replay_batch_pt(rng, B, K)
    eps3 = [rng.standard_normal((B, 2)).astype(np.float32) for _ in range(3)]
    out = dict(batch_obs=batch[0], batch_actions=batch[1], batch_rewards=batch[2], batch_obs_tp1=batch[3], batch_dones=batch[4],
               target_scale=G.TARGET_SCALE, weights_seed=np.array(seed), eps_target=eps3[0], eps_policy=eps3[1], eps_alpha=eps3[2],
               log_alpha=np.array(LOG_ALPHA0), target_entropy=np.array(TARGET_ENTROPY, np.float32))
    full = {}
    for tag, dt in (('', torch.float32), ('_f64', torch.float64)):
        learner, grads, st = run_once(args, nets, batch, eps3, dt)
        pw = learner.policy_with_value
        full[tag] = [np.asarray(g, np.float64) for g in grads]
        out['grads' + tag] = flat(grads[:18]) if tag == '' else sub64(flat(grads[:18]), H)
        out['alpha_grad' + tag] = np.asarray(grads[18])
        out['targets' + tag] = np.asarray(learner.batch_data['batch_targets'])
        for key in STATS:
            out[key + tag] = np.asarray(st[key])
        po = [learner.preprocessor.tf_process_obses(batch[i]).numpy() for i in (3, 0, 0)]
        tf.set_noise_source(NoiseStream(list(eps3)))
        for k, p in zip(('logp_target', 'logp_policy', 'logp_alpha'), po):
            out[k + tag] = np.asarray(pw.compute_action(p)[1])
        for k in ('targets', 'logp_target', 'logp_policy', 'logp_alpha', 'alpha_grad'):
            full[k + tag] = np.asarray(out[k + tag], np.float64)
    out['small64'] = np.concatenate([g.ravel() for g in full['_f64'][:18] if g.size < 8])
    tf.set_ref_dtype(torch.float32)
    tf.set_noise_source(None)
    rel = [np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30) for a, b in zip(full[''], full['_f64'])]
    rel_v = [np.linalg.norm(full[k] - full[k + '_f64']) / np.linalg.norm(full[k + '_f64'])
             for k in ('targets', 'logp_target', 'logp_policy', 'logp_alpha')]
    gn = float(out['alpha_gradient_norm'])
    print('sac auto H %d K %d seed %d: reference float32 vs float64, rel L2 per array: %s   (max %.1e); targets / logp %s; '
          'temperature |g| %.3f alpha %.6f alpha_loss %.4f entropy %.3f' % (H, K, seed, ' '.join('%.1e' % r for r in rel), max(rel),
                                                                          ' '.join('%.1e' % r for r in rel_v), gn, float(out['alpha']),
                                                                          float(out['alpha_loss']), float(out['policy_entropy'])))
    ok = max(max(rel), max(rel_v)) <= QUARTER_BAR and gn > CLIP
    if ok and not lean:
        # the further small case: target_entropy 3.0 puts |g| below the clip, so the gradient passes as it is
        for tag, dt in (('', torch.float32), ('_f64', torch.float64)):
            _, grads, st = run_once(auto_args(B, H, K, target_entropy=3.0), nets, batch, eps3, dt)
            out['small_alpha_grad' + tag], out['small_alpha_gradient_norm' + tag] = np.asarray(grads[18]), np.asarray(st['alpha_gradient_norm'])
            out['small_alpha_loss' + tag] = np.asarray(st['alpha_loss'])
        tf.set_ref_dtype(torch.float32)
        tf.set_noise_source(None)
        out['small_target_entropy'] = np.array(3.0, np.float32)
        sn = float(out['small_alpha_gradient_norm'])
        print('   target_entropy 3.0: |g| %.4f' % sn)
        ok = 0 < sn < CLIP and abs(float(out['small_alpha_grad'])) == sn
    if ok:
        if lean:
            for k, v in fixture_weights(seed, K, H).items():
                assert np.array_equal(flat(nets[k]), v), k
        else:
            for k in ('policy', 'Q1', 'Q2'):
                out['w_' + k] = flat(nets[k])
        path = os.path.join(HERE, 'sac_auto_H%d_B%d%s.npz' % (H, B, '_K%d' % K if K else ''))
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) <= 1 << 20, (path, os.path.getsize(path))
    return ok


def fx_loop(H=32, B=64, seed=2, n_iter=6):
    """the reference's own loop on one batch: compute_gradient (num_batch_reuse 1: the batch and its target are taken again on every
    call, three draws each) then PolicyWithQs.apply_gradients(iteration, grads)"""
    inject_alpha()
    from learners.sac import SACLearner
    from policy import PolicyWithQs
    rng = np.random.Generator(np.random.PCG64(seed))
    args = auto_args(B, H, 0, delay_update=2)
    nets = draw_nets(rng, H, 0)
    batch = make_replay_batch_pt(rng, B, 0)
    eps = rng.standard_normal((n_iter, 3, B, 2)).astype(np.float32)
    out = dict(batch_obs=batch[0], batch_actions=batch[1], batch_rewards=batch[2], batch_obs_tp1=batch[3], batch_dones=batch[4],
               target_scale=G.TARGET_SCALE, eps=eps, log_alpha0=np.array(LOG_ALPHA0), target_entropy=np.array(TARGET_ENTROPY, np.float32),
               n_iter=np.array(n_iter), delay_update=np.array(2))
    for k in ('policy', 'Q1', 'Q2'):
        out['w_' + k] = flat(nets[k])
    for tag, dt in (('', torch.float32), ('_f64', torch.float64)):
        tf.set_ref_dtype(dt)
        learner = SACLearner(PolicyWithQs, args)
        pw = learner.policy_with_value
        set_policy_weights(pw, nets)
        la, ag, an, alpha, its = [], [], [], [], []
        for it in range(n_iter):
            tf.set_noise_source(NoiseStream(list(eps[it])))
            grads = learner.compute_gradient(batch, None, None, it)
            st = learner.get_stats()
            pw.apply_gradients(tf.constant(it, dtype=tf.int32), grads)
            la.append(np.asarray(pw.get_weights()[3][0], np.float64))
            ag.append(np.asarray(grads[18], np.float64)), an.append(float(st['alpha_gradient_norm'])), alpha.append(float(st['alpha']))
            its.append([int(o.iterations) for o in pw.optimizers])
        out['log_alpha' + tag], out['alpha_grad' + tag] = np.array(la), np.array(ag)
        out['alpha_gradient_norm' + tag], out['alpha' + tag] = np.array(an), np.array(alpha)
        p, t = G.flat_models(pw)                        # models [Q1, Q2, policy, alpha]: the last entry of p is log_alpha
        out['params' + tag], out['targets_end' + tag] = p[:-1], t
        if tag == '':
            out['opt_iterations'] = np.array(its)
    tf.set_ref_dtype(torch.float32)
    tf.set_noise_source(None)
    la32, la64 = out['log_alpha'], out['log_alpha_f64']
    print('sac auto loop: log_alpha %s\n   float64 %s\n   |g| %s   optimizer iterations at the end %s' % (
        ' '.join('%.7f' % v for v in la32), ' '.join('%.7f' % v for v in la64), ' '.join('%.3f' % v for v in out['alpha_gradient_norm']),
        out['opt_iterations'][-1]))
    # delay_update 2: the temperature's Adam (the fourth optimizer) steps on even iterations only
    assert list(out['opt_iterations'][:, 3]) == [it // 2 + 1 for it in range(n_iter)], out['opt_iterations']
    assert all(la32[it] == la32[it - 1] for it in range(1, n_iter, 2)) and all(la32[it] != la32[it - 1] for it in range(2, n_iter, 2))
    assert np.abs(la32 - la64).max() <= QUARTER_BAR * np.abs(la64).max()
    path = os.path.join(HERE, 'sac_auto_loop_H%d_B%d.npz' % (H, B))
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= 1 << 20, (path, os.path.getsize(path))


def main():
    torch.manual_seed(0)
    for H, K, lean in ((256, 0, True), (256, 3, True), (32, 0, False)):
        assert any(fx_auto(H, 64, K, seed, lean) for seed in SEEDS), 'no seed of the list meets the conditions (H %d, K %d)' % (H, K)
    fx_loop()


if __name__ == '__main__':
    main()
