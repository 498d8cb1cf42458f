"""n-step DPG on the GPU: the one-launch real-env rollout (mpg_env_rollout) against the chain of stand-alone launches it replaces, bit
for bit; the single-critic policy gradient (mpg_dpg_policy_grad) against float64 autograd and against mpg_td3_policy_grad(q1, q1);
NDPGLearner against the fixtures of the unmodified reference (tests/golden/make_golden_ndpg.py); the native step driver
(learner_version 5) against the method-by-method path; checkpoint resume; a training loop."""
import ctypes

import numpy as np
import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops
from tests import ndpg_oracle as N
from tests import yardstick as Y

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BATCH_KEYS = ('batch_obs', 'batch_actions', 'batch_rewards', 'batch_obs_tp1', 'batch_dones')


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(params=['split', 'f32'])
def engine(request):
    """both builds of the library (mpg_amd/_lib.py ENGINES): the split-fp16 product and the exact-fp32 engine"""
    with L.engine(request.param):
        yield request.param


# ---- 1 / 2: mpg_env_rollout ------------------------------------------------------------------------------------------------
def start_rows(rng, rows, od):
    """start observations from the reset law; every fourth row far beyond the env's done thresholds (|delta_y| > 3,
    |delta_phi| > pi / 4: "done" agents keep stepping - nothing resets them); replay actions like make_golden.make_replay_batch_pt"""
    from tests.golden_inputs import reset_law_obs
    obs = np.concatenate([reset_law_obs(rng, rows), rng.standard_normal((rows, od - 6)).astype(np.float32)], 1)
    far = np.arange(rows) % 4 == 1
    obs[far, 3] = np.where(rng.uniform(size=far.sum()) < 0.5, -1., 1.) * rng.uniform(5., 9., far.sum())
    obs[far, 4] = np.where(rng.uniform(size=far.sum()) < 0.5, -1., 1.) * rng.uniform(1.2, 2.0, far.sum())
    act = np.clip(rng.uniform(-1, 1, (rows, 2)) + 0.1 * rng.standard_normal((rows, 2)), -1.2, 1.2)
    return obs.astype(np.float32), act.astype(np.float32)


def chain(cfg, pol, obs0, act0, n):
    """the sequence mpg_env_rollout replaces, through the existing entry points: mpg_env_reset_from_obs, then per step
    mpg_policy_action (from the second step on) and mpg_env_step"""
    rows, od = obs0.shape
    state = torch.zeros(8, rows, device=DEV)
    obs = torch.empty(rows, od, device=DEV)
    act = torch.empty(rows, 2, device=DEV)
    rew = torch.empty(n, rows, device=DEV)
    done, done_i = torch.empty(rows, dtype=torch.uint8, device=DEV), torch.empty(rows, dtype=torch.uint8, device=DEV)
    L.call('mpg_env_reset_from_obs', L.c_int(0), L.c_int(rows), L.c_int(od), L.ptr(state), L.ptr(obs0), L.stream())
    for t in range(n):
        if t > 0:
            L.call('mpg_policy_action', ctypes.byref(cfg), L.ptr(pol), L.c_int(rows), L.ptr(obs), L.c_float(0.), L.c_u64(0), L.c_u64(0),
                   L.ptr(act), L.stream())
        L.call('mpg_env_step', L.c_int(0), L.c_int(rows), L.c_int(od), L.ptr(state), L.ptr(act0 if t == 0 else act), L.ptr(obs),
               L.ptr(rew[t]), L.ptr(done), L.ptr(done_i), L.stream())
    return rew, obs


def both(od, cache, rows, n, poison=None, seed=0):
    """(chain, one launch, [status of the chain, status of the launch]) on the same inputs"""
    from tests.golden_inputs import mlp_weights_flat
    rng = np.random.Generator(np.random.PCG64(1000 * od + 10 * rows + n + seed))
    cfg = ops.make_cfg(obs_dim=od)
    pol = dev(mlp_weights_flat(rng, od, 4))
    wc = None
    if cache:                                         # the packed-image instantiation: cfg.wcache[0] -> the policy's images
        wc = ops.WeightCache(pol, [(od, 4)])
        cfg.wcache[0] = wc.pointer
    o, a = start_rows(rng, rows, od)
    if poison is not None:
        o[poison] = np.nan
    obs0, act0 = dev(o), dev(a)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    cfg.status = st.data_ptr()
    ra, oa = chain(cfg, pol, obs0, act0, n)
    status = [int(st.item())]
    st.zero_()
    rb, ob = ops.env_rollout(cfg, pol, obs0, act0, n)
    torch.cuda.synchronize()
    status.append(int(st.item()))
    del wc
    return (ra, oa), (rb, ob), status


@pytest.mark.parametrize('cache', [False, True], ids=['strided', 'packed'])
@pytest.mark.parametrize('od', [6, 9, 16])
@pytest.mark.parametrize('n', [1, 2, 25])
@pytest.mark.parametrize('rows', [16, 40, 256])
def test_env_rollout_equals_the_per_step_sequence_bit_for_bit(engine, rows, n, od, cache):
    """rows: one full 16-row group, a partial last group, many groups.  n = 1 runs no policy pass, n = 2 the first hand-over through
    LDS.  obs_dim 6 (the eight-wide input block), 9 and 16 (the 16-wide one, partly and completely filled)."""
    a, b, status = both(od, cache, rows, n)
    assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all()
    assert torch.equal(bits(a[0]), bits(b[0])), 'rewards'
    assert torch.equal(bits(a[1]), bits(b[1])), 'last observations'
    assert status[0] == status[1] == 0, status


@pytest.mark.parametrize('od,cache', [(9, False), (6, True)])
def test_env_rollout_reports_a_nan_start_row_like_the_sequence(engine, od, cache):
    """one NaN entry in one row of obs0: that row's agent is NaN from the reset on, its observation reaches the policy pass at the
    second step, and both paths OR MPG_STATUS_NAN into the status word; every other row agrees bit for bit"""
    rows, row = 40, 21
    a, b, status = both(od, cache, rows, 25, poison=(row, 3))
    assert status[0] == status[1] and status[1] & ops.STATUS_NAN, status
    keep = torch.ones(rows, dtype=torch.bool, device=DEV)
    keep[row] = False
    assert torch.isnan(b[0][:, row]).all() and torch.isnan(a[0][:, row]).all()
    assert torch.isfinite(b[0][:, keep]).all() and torch.isfinite(b[1][keep]).all()
    assert torch.equal(bits(a[0][:, keep]), bits(b[0][:, keep])) and torch.equal(bits(a[1][keep]), bits(b[1][keep]))


@pytest.mark.parametrize('od', [6, 9])
def test_env_rollout_repeated_launches_are_bit_identical(engine, od):
    """300 launches on the same inputs: the loop's LDS hand-overs between wave 0 and the policy pass are the new thing here"""
    from tests.golden_inputs import mlp_weights_flat
    rows, n = 256, 25
    rng = np.random.Generator(np.random.PCG64(50 + od))
    cfg = ops.make_cfg(obs_dim=od)
    pol = dev(mlp_weights_flat(rng, od, 4))
    wc = ops.WeightCache(pol, [(od, 4)])
    cfg.wcache[0] = wc.pointer
    o, a = start_rows(rng, rows, od)
    obs0, act0 = dev(o), dev(a)
    r0, o0 = ops.env_rollout(cfg, pol, obs0, act0, n)
    diff = torch.zeros(1, dtype=torch.int64, device=DEV)
    for _ in range(300):
        r, o = ops.env_rollout(cfg, pol, obs0, act0, n)
        diff += (bits(r) != bits(r0)).sum() + (bits(o) != bits(o0)).sum()
    assert int(diff.item()) == 0
    assert torch.isfinite(r0).all()
    del wc


# ---- 3: mpg_dpg_policy_grad ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [0, 3])
def test_dpg_policy_grad_vs_float64_autograd_and_vs_the_td3_entry_point(golden, engine, K):
    g = golden('ndpg_H256_B64%s.npz' % ('_K%d' % K if K else ''))
    w = N.fixture_weights(int(g['weights_seed']), K)
    cfg = ops.make_cfg(obs_dim=6 + K)
    pol, q1, obs = dev(w['policy']), dev(w['Q1']), dev(g['batch_obs'])
    stats, grad = ops.dpg_policy_grad(cfg, pol, q1, obs)
    stats, grad = stats.cpu().numpy().astype(np.float64), grad.cpu().numpy()
    ref = {}
    for dt in (torch.float32, torch.float64):
        ocfg, nets = N.fixture_nets(g, K, 256, dt)
        po = N.O.process_obses(ocfg, torch.as_tensor(g['batch_obs']).to(dt))
        q = nets.q('Q1', po, nets.compute_action(po))
        pg = torch.autograd.grad(-q.mean(), nets.w['policy'])
        ref[dt] = (np.concatenate([x.numpy().ravel() for x in pg]).astype(np.float64), q.detach().numpy().astype(np.float64))
    worst = Y.check_gradients(grad, ref[torch.float32][0].astype(np.float32), ref[torch.float64][0][::8], [('policy', 6 + K, 4)],
                              where='mpg_dpg_policy_grad K=%d (%s)' % (K, engine))
    q64 = ref[torch.float64][1]
    e_sum, e_sq = abs(stats[0] - q64.sum()) / abs(q64.sum()), abs(stats[1] - (q64 ** 2).sum()) / (q64 ** 2).sum()
    print('mpg_dpg_policy_grad K=%d %s: gradient worst error / allowance %.3f; q_sum rel err %.2e, q_sqsum rel err %.2e'
          % (K, engine, worst, e_sum, e_sq))
    assert e_sum <= 1e-6 and e_sq <= 1e-6, (e_sum, e_sq)
    # the two-critic entry point with the same critic twice: every row takes Q1 (ties go to the first critic)
    st3, g3 = ops.td3_policy_grad(cfg, pol, q1, q1, obs)
    st3, g3 = st3.cpu().numpy().astype(np.float64), g3.cpu().numpy()
    assert abs(st3[0] - stats[0]) <= 1e-6 * abs(stats[0]) and abs(st3[1] - stats[1]) <= 1e-6 * abs(stats[1]), (st3, stats)
    assert Y.rel_l2(grad, g3) <= 1e-6, Y.rel_l2(grad, g3)


# ---- 4: the learner against the reference's fixtures ---------------------------------------------------------------------------
def _learner(g, K, **kw):
    from mpg_amd.config import default_args
    from mpg_amd.learners import NDPGLearner
    from mpg_amd.policy import PolicyWithQs
    args = default_args('NDPG', replay_batch_size=64, num_batch_reuse=1, num_future_data=K, **kw)
    learner = NDPGLearner(PolicyWithQs, args)
    pw = learner.policy_with_value
    assert pw.names == ['Q1', 'policy']
    w = N.fixture_weights(int(g['weights_seed']), K)
    flat = np.concatenate([w[n] for n in pw.names])
    pw.set_flat(flat, (flat * np.float32(g['target_scale'])).astype(np.float32))
    return learner


@pytest.mark.parametrize('K', [0, 3])
def test_compute_gradient_vs_reference_golden(golden, engine, K):
    """the list the reference's NDPGLearner.compute_gradient returns (clipped Q1 and policy gradients), its targets, its sampler's
    rewards / last observation, its stats and td error, on the same minibatch and weights"""
    g = golden('ndpg_H256_B64%s.npz' % ('_K%d' % K if K else ''))
    learner = _learner(g, K)
    pw = learner.policy_with_value
    batch = [dev(g[k]) for k in BATCH_KEYS]
    grads = learner.compute_gradient(batch, None, None, 0)
    assert len(grads) == 12
    got = torch.cat([x.reshape(-1) for x in grads]).cpu().numpy()
    where = 'NDPG K=%d (%s)' % (K, engine)
    worst = Y.check_gradients(got, g['grads'], g['grads_f64'], [(n,) + tuple(pw.dims[n]) for n in pw.names], where=where,
                              small64=g['small64'])
    print(where, 'worst error / allowance %.3f' % worst)
    Y.check_values(learner.batch_data['batch_targets'].cpu().numpy(), g['targets'], g['targets_f64'], what='targets ' + where)
    ro = learner.sample(batch[0], batch[1])
    # (the tolerances the MPG-v1 fixture's same keys are checked at: rewards tests/test_networks_gpu.py, last observation
    # tests/test_oracle_golden.py)
    np.testing.assert_allclose(ro['all_rewards'].cpu().numpy(), g['nstep_all_rewards'], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(ro['last_obs'].cpu().numpy(), g['nstep_last_obs'], rtol=0, atol=2e-3)
    st = learner.get_stats()
    # stats: means of float32 results inside the 1e-4 bar of the yardstick; the un-clipped norms likewise
    for k in ('q_loss', 'policy_loss', 'mb_targets_mean', 'value_mean', 'q_gradient_norm', 'policy_gradient_norm'):
        np.testing.assert_allclose(st[k], g[k], rtol=1e-4, atol=1e-7, err_msg=k)
    assert st['q_gradient_norm'] > 3.0                                # the clip is exercised
    # value_var = E[Q^2] - mean^2: the two terms' 1e-4 relative errors against a difference that is smaller than either
    mean, var = float(g['value_mean_f64']), float(g['value_var_f64'])
    np.testing.assert_allclose(st['value_var'], g['value_var'], rtol=1e-4 * (var + 3 * mean * mean) / var)
    # the clipped norms of the returned arrays: Q1 was clipped to 3, the policy's norm is below the clip
    off = np.cumsum([0] + list(pw.sizes))
    nq, npi = np.linalg.norm(got[off[0]:off[1]].astype(np.float64)), np.linalg.norm(got[off[1]:off[2]].astype(np.float64))
    np.testing.assert_allclose(nq, min(3.0, float(g['q_gradient_norm'])), rtol=1e-5)
    np.testing.assert_allclose(npi, min(3.0, float(g['policy_gradient_norm'])), rtol=1e-4)
    np.testing.assert_allclose(learner.compute_td_error().cpu().numpy(), g['td_error'], rtol=1e-4, atol=2e-5)


def test_learner_refuses_every_other_env():
    from mpg_amd.config import default_args
    from mpg_amd.learners import NDPGLearner
    from mpg_amd.policy import PolicyWithQs
    for env_id in ('InvertedPendulumConti-v0', 'InvertedDoublePendulum-v2'):
        with pytest.raises(ValueError, match='PathTracking-v0 only'):
            NDPGLearner(PolicyWithQs, default_args('NDPG', env_id=env_id))


# ---- 5 / 6 / 7: the loop ------------------------------------------------------------------------------------------------------
def _stack(fused, seed=0, interval=10, **kw):
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import NDPGLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    args = default_args('NDPG', seed=seed, **kw)
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    learner = NDPGLearner(PolicyWithQs, args)
    rb = ReplayBuffer(args, 0)
    opt = SingleProcessOffPolicyOptimizer(worker, learner, rb, None, args, sampling_interval=interval, fused=fused)
    assert (opt._fused is not None) == fused
    return opt


def _state(opt):
    pw, rb, w, ln = opt.worker.policy_with_value, opt.replay_buffer, opt.worker, opt.learner
    torch.cuda.synchronize()
    tensors = [t.clone() for t in (pw.params, pw.targets, pw.m, pw.v, rb.obs, rb.act, rb.rew, rb.obs2, rb.done, w.obs)]
    counters = (dict(pw.opt_steps), rb._next_idx, len(rb), rb.replay_times, w._noise_ctr, w.env._ctr, ln.counter, opt.num_sampled_steps)
    return tensors, counters


@pytest.mark.parametrize('reuse', [10, 1])
def test_native_step_driver_equals_method_by_method_path(engine, reuse):
    """learner_version 5 enqueues what the python classes enqueue: 25 iterations from the same seeds, B = 256, 8 agents, sampling
    every 10th iteration - parameters, targets, Adam moments, ring contents and counters are bit-identical"""
    def run(fused):
        opt = _stack(fused, num_agent=8, batch_size=512, replay_batch_size=256, replay_starts=1024, max_buffer_size=4096,
                     num_batch_reuse=reuse)
        for _ in range(25):
            opt.step()
        return _state(opt), opt.learner.get_stats()
    (a, ca), sa = run(True)
    (b, cb), sb = run(False)
    assert ca == cb, (ca, cb)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), i
    for k in N.STATS:
        assert sa[k] == sb[k], (k, sa[k], sb[k])


def test_stock_methods_interleaved_with_native_steps(engine):
    """tests/test_learner_gpu.py::test_stock_methods_interleaved_with_native_steps for NDPG: worker.sample() + rb.add_batch()
    between native steps end in the same ring, counters and parameters as the method-by-method path doing the same calls"""
    def run(fused):
        opt = _stack(fused, interval=2, num_agent=64, batch_size=64, replay_batch_size=96, replay_starts=256, max_buffer_size=700,
                     num_batch_reuse=3)
        for it in range(12):
            opt.step()
            if it % 3 == 1:                      # extra samples through the stock methods (wraps the 700-slot ring)
                batch, n = opt.worker.sample_with_count()
                opt.replay_buffer.add_batch(batch)
        return _state(opt)
    a, ca = run(True)
    b, cb = run(False)
    assert ca == cb, (ca, cb)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), i


@pytest.mark.parametrize('fused', [True, False], ids=['native', 'methods'])
def test_checkpoint_resume_is_bit_identical(tmp_path, engine, fused):
    """save after 12 iterations (inside a window of the reused batch: num_batch_reuse 10), continue 9 more; a freshly built optimizer
    that loads the file and runs the same 9 iterations ends bit-identical"""
    from mpg_amd.checkpoint import load_checkpoint, save_checkpoint

    def build(seed):
        return _stack(fused, seed=seed, interval=3, num_agent=64, batch_size=64, replay_batch_size=128, replay_starts=256,
                      max_buffer_size=1024)
    a = build(5)
    assert a.learner.num_batch_reuse == 10
    for _ in range(12):
        a.step()
    path = save_checkpoint(str(tmp_path / 'ckpt.npz'), a)
    for _ in range(9):
        a.step()
    b = build(99)                        # different seed: every stream must come from the file
    meta = load_checkpoint(path, b)
    assert meta['optimizer']['iteration'] == 12 and b.iteration == 12 and meta['learner_cls'] == 'NDPGLearner'
    for _ in range(9):
        b.step()
    (ta, ca), (tb, cb) = _state(a), _state(b)
    assert ca == cb, (ca, cb)
    for i, (x, y) in enumerate(zip(ta, tb)):
        assert torch.equal(x, y), i


def test_training_loop_learns_the_critic(engine):
    """300 iterations at the NDPG defaults (B = 256, 8 agents, batch reused 10 times): the critic loss at the end is below its value
    at iteration 20"""
    opt = _stack(True)
    args = opt.args
    assert (args.replay_batch_size, args.num_agent, args.num_batch_reuse, args.replay_starts) == (256, 8, 10, 3000)
    pw = opt.worker.policy_with_value
    losses = []
    for i in range(300):
        opt.step()
        if i % 5 == 0 or i >= 290:
            losses.append((i, opt.learner.get_stats()['q_loss']))
    d = dict(losses)
    assert all(np.isfinite(v) for v in d.values()) and torch.isfinite(pw.params).all()
    assert pw.opt_steps == {'Q1': 300, 'policy': 300}                 # delay_update 1
    print('q_loss (%s) at 20: %.4e, at 299: %.4e' % (engine, d[20], d[299]))
    assert d[299] < d[20]
    pw.check_status()
