"""Restatement of the reference's MPG learner on InvertedPendulumConti-v0 (train_script4mujoco.py:169-293 built_MPG_parser;
learners/mpg_learner.py) in torch / numpy on the CPU (float32 / float64), composed from the pieces of oracle/mpg_oracle.py:

    sample()                 mpg_learner.py:87-108, the num_agent == 1 branch: ROW BY ROW, n real-env steps from (s, a_replay), later
                             actions from the online policy without noise, `done` ignored, nothing reset;
    compute_n_step_target()  :146-169 with the pendulum's clip of the bootstrap value to [-0.5, 0] (:163-164);
    compute_gradient()       :401-455 for MPG-v1 (that target, one critic) and MPG-v2 (the clipped double-Q target, two critics).

The real env is MuJoCo's and MuJoCo is absent: on BOTH sides - here and in tests/golden/make_golden_mpg_pendulum.py - the env is the
documented closed-form stand-in oracle.InvertedPendulumContiOracle (its parity with MuJoCo is unpinned).
Used by the tests only; mpg_amd never imports it."""
import numpy as np
import torch

from oracle import mpg_oracle as O
from tests.golden_inputs import mlp_weights_flat

PEND = 'InvertedPendulumConti-v0'
Q_LO, Q_HI = -0.5, 0.0                      # mpg_learner.py:163-164
TOTAL_ITE = 4000                           # built_MPG_parser's rule_based_bias_total_ite
ITERATIONS = (100, 3000)
STATS = ('value_mean', 'policy_total_loss', 'policy_gradient_norm', 'q_loss1', 'q_gradient_norm1', 'q_loss2', 'q_gradient_norm2')


def names_of(version):
    return ['Q1', 'Q2'] if version == 'MPG-v2' else ['Q1']


def net_list(version):
    """[(name, in, out)] in the order of the flat gradient (tests/yardstick.py layout)"""
    return [(n, 5, 1) for n in names_of(version)] + [('policy', 4, 2)]


def fixture_weights(seed, version, H=256):
    """the online networks of tests/golden/make_golden_mpg_pendulum.py for `seed`: its first draws, `policy`, `Q1` (, `Q2`)"""
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    w = {'policy': mlp_weights_flat(rng, 4, 2, H), 'Q1': mlp_weights_flat(rng, 5, 1, H)}
    if version == 'MPG-v2':
        w['Q2'] = mlp_weights_flat(rng, 5, 1, H)
    return w


def fixture_targets(w, target_scale, q_scale, q_shift, H=256):
    """the target networks of a fixture: online * target_scale (float32 product), then the TARGET critic Q1's output layer scaled and
    shifted - W3 * q_scale, b3 * q_scale + q_shift, float32 - so that its values straddle the clip interval (the generator's factors)"""
    t = {k: (np.asarray(v) * np.float32(target_scale)).astype(np.float32) for k, v in w.items()}
    q = t['Q1'].copy()
    q[-(H + 1):] = (q[-(H + 1):] * np.float32(q_scale)).astype(np.float32)
    q[-1] = np.float32(q[-1] + np.float32(q_shift))
    t['Q1'] = q
    return t


def make_cfg(H=256):
    return O.Cfg(PEND, H=H, total_ite=TOTAL_ITE)


def fixture_nets(g, version, dtype=torch.float32, H=256):
    cfg = make_cfg(H)
    w = fixture_weights(int(g['weights_seed']), version, H)
    t = fixture_targets(w, g['target_scale'], g['q_scale'], g['q_shift'], H)
    return cfg, O.Nets(cfg, w, flat_targets=t, dtype=dtype)


def fixture_batch(g):
    return [g['batch_obs'], g['batch_actions'], g['batch_rewards'], g['batch_obs_tp1'], g['batch_dones']]


def np_dtype(dt):
    return np.float64 if dt == torch.float64 else np.float32


def sample(cfg, nets, obs, act):
    """(all_rewards [n, B], all_obs_tp1 [n, B, 4]) as float32, like the reference's np.array(..., dtype=np.float32); the env runs in the
    nets' precision"""
    B, dt = obs.shape[0], np_dtype(nets.dtype)
    all_r, all_o = np.zeros((cfg.n, B), np.float32), np.zeros((cfg.n, B, 4), np.float32)
    for i in range(B):
        env = O.InvertedPendulumContiOracle(1, dtype=dt)
        o = env.reset(init_obs=obs[i:i + 1])
        for t in range(cfg.n):
            if t == 0:
                a = np.asarray(act[i:i + 1], dt)
            else:
                with torch.no_grad():
                    a = nets.compute_action(O.process_obses(cfg, torch.as_tensor(o).to(nets.dtype))).numpy()
            o, r, _, _ = env.step(a)
            all_r[t, i], all_o[t, i] = r[0], o[0]
    return all_r, all_o


def n_step_target(cfg, nets, obs, act):
    """(targets float32 [B], unclipped bootstrap values [B], all_rewards, last observations)"""
    all_r, all_o = sample(cfg, nets, obs, act)
    with torch.no_grad():
        po = O.process_obses(cfg, torch.as_tensor(all_o[-1]).to(nets.dtype))
        pr = O.process_rewards(cfg, torch.as_tensor(all_r).to(nets.dtype)).numpy()
        q_last = nets.q('Q1_target', po, nets.compute_target_action(po))
        q_clip = torch.clamp(q_last, Q_LO, Q_HI)
    tgt = np.zeros((obs.shape[0],), dtype=np.float32)           # (the reference's own float32 accumulator, in both precisions: :165-168)
    for t in range(cfg.n):
        tgt += np.power(cfg.gamma, t) * pr[t]
    tgt += (float(np.power(cfg.gamma, cfg.n)) * q_clip).numpy()          # (a tensor product in the nets' precision, as in the reference)
    return tgt, q_last.numpy(), all_r, all_o[-1]


def compute_gradient(cfg, nets, batch, eps, iteration, version):
    """MPGLearner.compute_gradient on the pendulum.  Returns (list of numpy grads q1 (, q2), policy; stats with `targets`, and for
    MPG-v1 `q_boot`, `all_rewards`, `last_obs`)."""
    dt = nets.dtype
    obs, act, rew, obs1 = [torch.as_tensor(np.asarray(b, dtype=np.float32)).to(dt) for b in batch[:4]]
    stats = {}
    if version == 'MPG-v1':
        tgt, q_boot, all_r, last = n_step_target(cfg, nets, np.asarray(batch[0], np.float32), np.asarray(batch[1], np.float32))
        targets = torch.as_tensor(tgt).to(dt)
        stats.update(q_boot=q_boot, all_rewards=all_r, last_obs=last)
    else:
        targets = O.clipped_double_q_target(cfg, nets, rew, obs1)
    names = names_of(version)
    q_losses, q_grads = O.q_forward_and_backward(cfg, nets, obs, act, targets, names)
    stats['targets'] = targets.numpy()
    out = []
    for i, (l, g) in enumerate(zip(q_losses, q_grads)):
        g, nrm = O.clip_by_global_norm(g, cfg.clip)
        out += g
        stats['q_loss%d' % (i + 1)] = l.numpy()
        stats['q_gradient_norm%d' % (i + 1)] = nrm.numpy()
    reduced, _, _ = O.model_rollout_for_policy_update(cfg, nets, obs, torch.as_tensor(np.asarray(eps)).to(dt))
    ws = O.rule_based_weights(iteration, cfg.total_ite, cfg.eta, cfg.select, dt)
    minus = torch.stack([-reduced[k] for k in cfg.select])
    total_loss = torch.sum(ws.detach() * minus)
    pg, pnorm = O.clip_by_global_norm(list(torch.autograd.grad(total_loss, nets.w['policy'])), cfg.clip)
    out += pg
    stats.update(value_mean=reduced[0].detach().numpy(), policy_total_loss=total_loss.detach().numpy(), policy_gradient_norm=pnorm.numpy(),
                 w_list=ws.numpy(), all_losses=minus.detach().numpy())
    return [g.detach().numpy() for g in out], stats


def load(golden, version):
    """a fixture as one dict: mpg_v{1,2}_pendulum_H256_B64.npz and, where the generator split the second iteration off to fit the size
    limit of a committed file, ..._it3000.npz beside it"""
    name = 'mpg_%s_pendulum_H256_B64.npz' % version[-2:]
    g = dict(golden(name))
    if 'split' in g and int(g['split']):
        g.update(golden(name[:-4] + '_it%d.npz' % ITERATIONS[1]))
    return g


def flat_grads(g, it):
    """the flat float32 gradient of iteration `it` in reference order: the critics' arrays are stored once (they do not depend on the
    iteration: the generator asserts it), the policy's per iteration.  (The float64 yard-stick is `it{it}_grads_f64`: every 8th element
    of the whole flat vector.)"""
    return np.concatenate([g['q_grads'], g['it%d_policy_grads' % it]])
