"""MPG on the inverted pendulum on the GPU: MPGLearner (MPG-v1: one-launch real-env rollout + clipped n-step target; MPG-v2: clipped
double-Q target) against the fixtures of the unmodified reference (tests/golden/make_golden_mpg_pendulum.py - the env there is the
documented closed-form stand-in, MuJoCo being absent: DESIGN.md section 2); the v1 learner's sample() against the per-step chain
through mpg_amd.envs, bit for bit; the native step driver (learner_version 1 on the pendulum's env kind) against the method-by-method
path, with a checkpoint resume, and against itself with the chain forced (sample_iters < 0)."""
import numpy as np
import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops
from tests import mpg_pendulum_oracle as P
from tests import yardstick as Y

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BATCH_KEYS = ('batch_obs', 'batch_actions', 'batch_rewards', 'batch_obs_tp1', 'batch_dones')


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


@pytest.fixture(params=['split', 'f32'])
def engine(request):
    """both builds of the library (mpg_amd/_lib.py ENGINES): the split-fp16 product and the exact-fp32 engine"""
    with L.engine(request.param):
        yield request.param


# ---- the learner against the reference's fixtures ---------------------------------------------------------------------------------
def _learner(g, version):
    from mpg_amd.config import default_args
    from mpg_amd.learners import MPGLearner
    from mpg_amd.policy import PolicyWithQs
    args = default_args(version, env_id=P.PEND, replay_batch_size=64, num_batch_reuse=1)
    assert args.rule_based_bias_total_ite == P.TOTAL_ITE
    learner = MPGLearner(PolicyWithQs, args)
    pw = learner.policy_with_value
    assert pw.names == P.names_of(version) + ['policy']
    w = P.fixture_weights(int(g['weights_seed']), version)
    t = P.fixture_targets(w, g['target_scale'], g['q_scale'], g['q_shift'])
    pw.set_flat(np.concatenate([w[n] for n in pw.names]), np.concatenate([t[n] for n in pw.names]))
    return learner


@pytest.mark.parametrize('version', ['MPG-v1', 'MPG-v2'])
def test_compute_gradient_vs_reference_golden(golden, engine, version):
    """the list the reference's MPGLearner.compute_gradient returns on the pendulum (clipped critic and policy gradients) at both
    iterations, its targets, statistics and clipped norms, on the same minibatch, weights and model noise"""
    g = P.load(golden, version)
    learner = _learner(g, version)
    pw = learner.policy_with_value
    assert learner.pendulum and learner.env is None               # no PathTrackingEnv is built
    batch, eps = [dev(g[k]) for k in BATCH_KEYS], dev(g['eps'])
    nets = [(n,) + tuple(pw.dims[n]) for n in pw.names]
    assert nets == P.net_list(version)
    off = np.cumsum([0] + list(pw.sizes))
    for it in P.ITERATIONS:
        grads = learner.compute_gradient(batch, None, None, it, eps=eps)
        assert len(grads) == 6 * len(pw.names)
        got = torch.cat([x.reshape(-1) for x in grads]).cpu().numpy()
        where = '%s pendulum it %d (%s)' % (version, it, engine)
        worst = Y.check_gradients(got, P.flat_grads(g, it), g['it%d_grads_f64' % it], nets, where=where, small64=g['it%d_small64' % it])
        print(where, 'worst error / allowance %.3f' % worst)
        Y.check_values(learner.batch_data['batch_targets'].cpu().numpy(), g['targets'], g['targets_f64'], what='targets ' + where)
        st = learner.get_stats()
        # stats: means of float32 results inside the 1e-4 bar of the yardstick; the un-clipped norms likewise
        for k in P.STATS:
            if 'it%d_%s' % (it, k) in g:
                np.testing.assert_allclose(st[k], g['it%d_%s' % (it, k)], rtol=1e-4, atol=1e-7, err_msg=k)
        np.testing.assert_allclose(st['w_list'], g['it%d_w_list' % it], rtol=1e-5)
        np.testing.assert_allclose(np.asarray(st['all_losses']), g['it%d_all_losses' % it], rtol=1e-4, atol=1e-7)
        # the clipped norms of the returned arrays: min(3, the un-clipped norm) per network
        for i, n in enumerate(pw.names):
            key = 'policy_gradient_norm' if n == 'policy' else 'q_gradient_norm%s' % n[1]
            unclipped = float(g['it%d_%s' % (it, key)])
            np.testing.assert_allclose(np.linalg.norm(got[off[i]:off[i + 1]].astype(np.float64)), min(3.0, unclipped), rtol=1e-4, err_msg=n)
    np.testing.assert_allclose(learner.compute_td_error().cpu().numpy(), g['td_error'], rtol=1e-4, atol=2e-5)


def test_v1_sampler_and_target_vs_reference_golden(golden, engine):
    """MPGLearner.sample() and compute_n_step_target() on the fixture's batch: the reference's all_rewards, last observations and
    (clipped) targets"""
    g = P.load(golden, 'MPG-v1')
    learner = _learner(g, 'MPG-v1')
    learner._get_batch([dev(g[k]) for k in BATCH_KEYS])
    ro = learner.sample(learner.batch_data['batch_obs'], learner.batch_data['batch_actions'])
    Y.check_values(ro['all_rewards'].cpu().numpy(), g['all_rewards'], g['all_rewards_f64'], what='all_rewards')
    Y.check_values(ro['last_obs'].cpu().numpy(), g['last_obs'], g['last_obs_f64'], what='last_obs')
    Y.check_values(learner.compute_n_step_target().cpu().numpy(), g['targets'], g['targets_f64'], what='targets')


def test_v1_sample_equals_the_chain_through_the_env_class(golden, engine):
    """the learner's one launch against InvertedPendulumContiEnv.reset(init_obs) / ops.policy_action / env.step, bit for bit"""
    from mpg_amd.envs import InvertedPendulumContiEnv
    g = P.load(golden, 'MPG-v1')
    learner = _learner(g, 'MPG-v1')
    pw = learner.policy_with_value
    obs0, act0 = dev(g['batch_obs']), dev(g['batch_actions'])
    ro = learner.sample(obs0, act0)
    env = InvertedPendulumContiEnv(num_agent=64, device=DEV)
    obs = env.reset(init_obs=obs0)
    rewards = []
    for t in range(learner.sample_num_in_learner):
        action = act0 if t == 0 else ops.policy_action(learner.cfg, pw.net('policy'), obs)
        obs, r, _, _ = env.step(action)
        rewards.append(r)
    assert ro['all_rewards'].shape == (25, 64) and torch.isfinite(ro['all_rewards']).all()
    assert torch.equal(bits(ro['all_rewards']), bits(torch.stack(rewards)))
    assert torch.equal(bits(ro['last_obs']), bits(obs))


def test_v1_sample_beyond_the_launchs_horizon_keeps_the_chain(golden, engine):
    """sample_num_in_learner 1030 > 1024: the learner builds its InvertedPendulumContiEnv and steps the chain; its first 1024 rewards
    are the one launch's at its longest horizon, bit for bit"""
    g = P.load(golden, 'MPG-v1')
    learner = _learner(g, 'MPG-v1')
    obs0, act0 = dev(g['batch_obs']), dev(g['batch_actions'])
    learner.sample_num_in_learner = 1030
    assert learner.env is None
    ro = learner.sample(obs0, act0)
    assert learner.env is not None and learner.env.kind == 1 and ro['all_rewards'].shape == (1030, 64)
    r, _ = ops.env_rollout_pendulum(learner.cfg, learner.policy_with_value.net('policy'), obs0, act0, 1024)
    assert torch.isfinite(r).all()
    assert torch.equal(bits(ro['all_rewards'][:1024]), bits(r))
    with pytest.raises(L.MpgError, match='n <= 1024'):
        ops.env_rollout_pendulum(learner.cfg, learner.policy_with_value.net('policy'), obs0, act0, 1025)


# ---- the loop -----------------------------------------------------------------------------------------------------------------------
def _stack(fused, seed=0):
    """the parser defaults (1 agent, 512 iterations per worker sample, replay_starts 3000, ...) with replay_batch_size 64 and
    num_batch_reuse 2"""
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import MPGLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    args = default_args('MPG-v1', env_id=P.PEND, seed=seed, replay_batch_size=64, num_batch_reuse=2)
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    learner = MPGLearner(PolicyWithQs, args)
    rb = ReplayBuffer(args, 0)
    opt = SingleProcessOffPolicyOptimizer(worker, learner, rb, None, args, sampling_interval=10, fused=fused)
    assert (opt._fused is not None) == fused            # the fused (native) optimizer accepts the MPG-v1 pendulum stack
    if fused:
        assert opt._fused.c.learner_version == 1 and opt._fused.c.cfg.env_kind == 1 and opt._fused.c.sample_iters == 512
    else:                                               # the method path's replay indices, draw by draw
        opt.drawn = []
        draw = rb.sample_idxes
        rb.sample_idxes = lambda n: (opt.drawn.append(draw(n)), opt.drawn[-1])[1]
    return opt


def _steps(opt, k, idx):
    """k iterations; idx collects the replay indices of the iterations that fetch a batch (every num_batch_reuse-th)"""
    for _ in range(k):
        fresh = opt.learner.counter % opt.learner.num_batch_reuse == 0
        opt.step()
        if fresh:
            idx.append((opt._fused.t['idx'] if opt._fused is not None else opt.drawn[-1]).clone())


def _state(opt):
    pw, rb, w, ln = opt.worker.policy_with_value, opt.replay_buffer, opt.worker, opt.learner
    torch.cuda.synchronize()
    n = len(rb)
    tensors = [t.clone() for t in (pw.params, pw.targets, pw.m, pw.v, rb.obs[:n], rb.act[:n], rb.rew[:n], rb.obs2[:n], rb.done[:n], w.obs,
                                   ln.batch_data['batch_targets'], pw.status)]
    counters = (dict(pw.opt_steps), rb._next_idx, n, rb.replay_times, w._noise_ctr, w.env._ctr, ln.counter, opt.num_sampled_steps,
                opt.iteration)
    return tensors, counters


def _same(a, b):
    (ta, ca), (tb, cb) = a, b
    assert ca == cb, (ca, cb)
    for i, (x, y) in enumerate(zip(ta, tb)):
        assert torch.equal(bits(x), bits(y)), i


def test_native_step_driver_equals_method_by_method_path_and_resumes(tmp_path, engine):
    """12 iterations (worker samples at 0 and 10, a fresh batch and its clipped n-step target every second call) by the native driver
    and by the python classes: parameters, targets, Adam moments, ring, the cached targets, status word, counters and the replay
    indices of every fetched batch are bit-identical; a checkpoint written at iteration 5 - inside a window of the reused batch - and
    resumed in a fresh stack of another seed ends in the same state"""
    from mpg_amd.checkpoint import load_checkpoint, save_checkpoint
    a, ia = _stack(True), []
    _steps(a, 5, ia)
    path = save_checkpoint(str(tmp_path / 'ckpt.npz'), a)
    _steps(a, 7, ia)
    b, ib = _stack(False), []
    _steps(b, 12, ib)
    assert len(ia) == len(ib) == 6
    for x, y in zip(ia, ib):
        assert torch.equal(x, y)
    _same(_state(a), _state(b))
    assert a.learner.counter == 12 and a.replay_buffer.replay_times == 12
    sa = a.learner.get_stats()
    assert np.isfinite(sa['q_loss1']) and torch.isfinite(a.worker.policy_with_value.params).all()
    c = _stack(True, seed=99)                           # different seed: every stream must come from the file
    meta = load_checkpoint(path, c)
    assert meta['optimizer']['iteration'] == 5 and c.iteration == 5 and meta['learner_cls'] == 'MPGLearner'
    _steps(c, 7, [])
    _same(_state(a), _state(c))


def test_native_driver_with_the_chain_forced_equals_the_one_launch_form(engine):
    """sample_iters < 0 keeps the chains (include/mpg_hip.h): the learner's mpg_env_reset_from_obs + 25 x (mpg_policy_action,
    mpg_env_step) instead of mpg_env_rollout_pendulum, and the worker's pairs instead of its one launch.  Both forms take the clipped
    target; everything the 12 iterations leave is bit-identical."""
    a, b = _stack(True), _stack(True)
    b._fused.c.sample_iters = -512
    assert not a._fused.l_env_state.any() and not b._fused.l_env_state.any()
    ia, ib = [], []
    _steps(a, 12, ia)
    _steps(b, 12, ib)
    for x, y in zip(ia, ib):
        assert torch.equal(x, y)
    _same(_state(a), _state(b))
    # the switch took: the chain's mpg_env_reset_from_obs / mpg_env_step wrote the learner's state block - its rows are the last
    # observations - and the launch, which holds the agents in registers, left its own untouched
    assert not a._fused.l_env_state.any()
    assert torch.equal(bits(b._fused.l_env_state[:4].t().contiguous()), bits(b._fused.t['l_obs'])) and b._fused.l_env_state[:4].any()
    assert torch.equal(bits(a._fused.t['l_rewards']), bits(b._fused.t['l_rewards'])) and torch.equal(bits(a._fused.t['l_obs']), bits(b._fused.t['l_obs']))
    # the targets the driver left are the CLIPPED ones: the method path's, recomputed from the driver's own rollout buffers
    # (y - sum_t gamma^t r_t = gamma^n clip(q) lies in [-0.5 gamma^n, 0] whatever the critic says; float32 sums of 26 terms)
    t = a._fused.t
    gam = torch.as_tensor(0.98 ** np.arange(25), dtype=torch.float32, device=DEV)
    s = (gam[:, None] * t['l_rewards']).sum(0)
    rest, tol = (t['b_targets'] - s).cpu().numpy(), 1e-5 * (1 + s.abs().cpu().numpy())
    assert (rest <= tol).all() and (rest >= -0.5 * 0.98 ** 25 - tol).all(), (rest.min(), rest.max())
