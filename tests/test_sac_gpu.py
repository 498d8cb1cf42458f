"""The Gaussian policy head on the GPU: the four-output network pass (k_forward<IN, 4>) against a float64 MLP and, on its first two
columns, bit for bit against the two-output pass; mpg_policy_sample (actions bit for bit from the returned logits, log-densities
against float64, repeated launches); mpg_sac_targets and mpg_sac_policy_grad against torch autograd in float64 on the same draws,
under the tolerance rule of tests/yardstick.py with float32 autograd as the reference's own float32 run.  Both engines, with and
without the packed weight image."""
import functools

import numpy as np
import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops
from oracle import mpg_oracle as O
from tests import yardstick as Y
from tests.golden_inputs import mlp_weights_flat, reset_law_obs

pytestmark = pytest.mark.gpu
DEV = 'cuda'
HALF_LOG_2PI = 0.5 * np.log(2 * np.pi)
ALPHA = 0.03                                   # train_script.py:672-792 (built_SAC_parser)


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def sigma32(log_std):
    """exp(clip(log_std, -5, 1)) as a float32 value: the correctly rounded one (include/mpg_hip.h, mpg_policy_sample)"""
    return torch.exp(torch.clamp(log_std, -5., 1.).double()).float()


@pytest.fixture(params=['split', 'f32'])
def engine(request):
    with L.engine(request.param):
        yield request.param


# ---- 1: the four-output forward --------------------------------------------------------------------------------------------
# 8200 rows = 513 row groups: the paired pass (forward_group2) with a ragged last pair and a ragged last group
@pytest.mark.parametrize('act', [ops.ACT_LINEAR, ops.ACT_TANH], ids=['linear', 'tanh'])
@pytest.mark.parametrize('din', [6, 9, 16])
@pytest.mark.parametrize('cache', [False, True], ids=['strided', 'packed'])
def test_four_output_forward(engine, cache, din, act):
    rng = np.random.Generator(np.random.PCG64(400 + din))
    flat = mlp_weights_flat(rng, din, 4)
    scale = rng.uniform(0.5, 2.0, din)
    ws = O.unflatten(flat, din, 256, 4, dtype=torch.float64)
    params = dev(flat)
    wc = ops.WeightCache(params, [(din, 4)]) if cache else None
    for rows in (1, 16, 17, 40, 8200):
        x = rng.standard_normal((rows, din)).astype(np.float32)
        y4 = ops.mlp_forward(params, din, 4, 4, act, dev(x), in_scale=scale, n_scaled=din, wcache=wc)
        y2 = ops.mlp_forward(params, din, 4, 2, act, dev(x), in_scale=scale, n_scaled=din, wcache=wc)
        assert y4.shape == (rows, 4)
        assert torch.equal(bits(y4[:, :2]), bits(y2)), (rows, 'the first two columns are the two-output pass')
        ref = O.mlp(ws, torch.as_tensor(x, dtype=torch.float64) * torch.as_tensor(scale.astype(np.float32)).double(),
                    'tanh' if act else 'linear').numpy()
        err = np.abs(y4.cpu().numpy() - ref).max()
        assert err <= 2e-5 * max(1.0, np.abs(ref).max()), (rows, err)              # the bar of test_mlp_forward_vs_oracle


# ---- 2 / 3: the entry points ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_case(seed, rows, K, spread=None, shift=None):
    """(computed once per set of arguments and shared by the engines / weight-image forms; nothing in it is written to later)
    random networks, observations from the reset law (+ K look-ahead entries), draws.  spread: the log-std columns of the policy's
    output kernel multiplied (logits on both sides of the clip and inside it); shift: added to the two log-std biases"""
    rng = np.random.Generator(np.random.PCG64(seed))
    od = 6 + K
    w = {'policy': mlp_weights_flat(rng, od, 4), 'Q1': mlp_weights_flat(rng, od + 2, 1), 'Q2': mlp_weights_flat(rng, od + 2, 1)}
    pol = w['policy']
    w3 = pol[-(256 * 4 + 4):-4].reshape(256, 4)           # a view: edits land in the flat vector
    if spread is not None:
        w3[:, 2:] *= spread
    if shift is not None:
        pol[-2:] += np.asarray(shift, np.float32)
    scale = list(O.OBS_SCALE_PT) + [1.] * K
    obs = np.concatenate([reset_law_obs(rng, rows), rng.standard_normal((rows, K)).astype(np.float32)], 1)
    c = dict(rows=rows, od=od, scale=scale, w=w, obs=obs, eps=rng.standard_normal((rows, 2)).astype(np.float32),
             rew=(-rng.uniform(0, 5, rows)).astype(np.float32), gamma=0.98)
    c['r32'], c['r64'] = reference(c, torch.float32), reference(c, torch.float64)
    return c


def attach_cache(case, cache):
    """the case on the device: its own cfg and tensors (the shared case stays as it is)"""
    c = dict(case)
    c['cfg'] = ops.make_cfg(obs_dim=c['od'], obs_scale=c['scale'], policy_out_activation='linear', gamma=c['gamma'])
    c['wp'], c['wq1'], c['wq2'] = dev(c['w']['policy']), dev(c['w']['Q1']), dev(c['w']['Q2'])
    if cache:           # the packed-image instantiations: cfg.wcache[0] -> the images of the three networks, one flat vector
        flat = torch.cat([c['wq1'], c['wq2'], c['wp']]).contiguous()
        nq = c['wq1'].numel()
        c['wq1'], c['wq2'], c['wp'] = flat[:nq], flat[nq:2 * nq], flat[2 * nq:]
        c['wc'] = ops.WeightCache(flat, [(c['od'] + 2, 1), (c['od'] + 2, 1), (c['od'], 4)])
        c['cfg'].wcache[0] = c['wc'].pointer
    return c


def reference(c, dtype, alpha=ALPHA):
    """policy.py:179-204 (action_range None) and sac.py:67-80 / 119-136 in torch at `dtype` on the recorded draws: logits, sample,
    log-density, soft target (the same networks stand in for the targets), policy loss pieces and the policy gradient"""
    t = lambda x: torch.as_tensor(x).to(dtype)
    wp = O.unflatten(c['w']['policy'], c['od'], 256, 4, dtype=dtype, requires_grad=True)
    q1 = O.unflatten(c['w']['Q1'], c['od'] + 2, 256, 1, dtype=dtype)
    q2 = O.unflatten(c['w']['Q2'], c['od'] + 2, 256, 1, dtype=dtype)
    po = t(c['obs']) * torch.tensor(c['scale'], dtype=torch.float32).to(dtype)
    eps = t(c['eps'])
    logits = O.mlp(wp, po, 'linear')
    mean, ls = logits[:, :2], torch.clamp(logits[:, 2:], -5., 1.)
    a = mean + torch.exp(ls) * eps
    logp = (-0.5 * eps ** 2 - ls - torch.tensor(HALF_LOG_2PI, dtype=dtype)).sum(1)
    qa = torch.cat([po, a], 1)
    qmin = torch.minimum(O.mlp(q1, qa, 'linear')[:, 0], O.mlp(q2, qa, 'linear')[:, 0])
    y = (t(c['rew']) + 0.) * torch.tensor(0.01, dtype=torch.float32).to(dtype) + \
        torch.tensor(c['gamma'], dtype=torch.float32).to(dtype) * (qmin - torch.tensor(alpha, dtype=torch.float32).to(dtype) * logp)
    loss = torch.mean(torch.tensor(alpha, dtype=torch.float32).to(dtype) * logp - qmin)
    grad = np.concatenate([g.numpy().ravel() for g in torch.autograd.grad(loss, wp)])
    return dict(logits=logits.detach().numpy(), a=a.detach().numpy(), logp=logp.detach().numpy(), y=y.detach().numpy(), grad=grad,
                qmin=qmin.detach().numpy())


@pytest.mark.parametrize('K', [0, 3])
@pytest.mark.parametrize('cache', [False, True], ids=['strided', 'packed'])
def test_policy_sample(engine, cache, K):
    for rows in (40, 8200):                  # the one-block and the many-block head
        c = attach_cache(make_case(500 + rows + K, rows, K, spread=30.0), cache)
        obs, eps = dev(c['obs']), dev(c['eps'])
        act, logp, logits = ops.policy_sample(c['cfg'], c['wp'], obs, eps, want_logits=True)
        ls = logits[:, 2:]
        assert (ls > 1).any() and (ls < -5).any() and ((ls > -5) & (ls < 1)).any(), 'the case is meant to sit on both sides of the clip'
        formed = logits[:, :2] + sigma32(ls) * eps                                  # float32, one rounding per operation
        assert torch.equal(bits(act), bits(formed)), (rows, (act - formed).abs().max().item())
        r32, r64 = c['r32'], c['r64']
        print('policy_sample rows %d K %d: logp vs float64 %.2e (float32 torch %.2e)' % (rows, K, Y.rel_l2(logp.cpu().numpy(), r64['logp']),
                                                                                       Y.rel_l2(r32['logp'], r64['logp'])))
        Y.check_values(logp.cpu().numpy(), r32['logp'], r64['logp'], what='logp')
        a2, lp2 = ops.policy_sample(c['cfg'], c['wp'], obs, eps)                    # without logits_out: the workspace's own block
        assert torch.equal(bits(a2), bits(act)) and torch.equal(bits(lp2), bits(logp))
    keep = (act.clone(), logp.clone())
    for _ in range(100):
        a, lp = ops.policy_sample(c['cfg'], c['wp'], obs, eps)
        assert torch.equal(bits(a), bits(keep[0])) and torch.equal(bits(lp), bits(keep[1]))


def check_arrays(got, r32, r64, od, where):
    """every array of the flat policy gradient: error against float64 at most 4 x float32 autograd's own + FLOOR (tests/yardstick.py)"""
    worst, o = 0.0, 0
    for shp in O.mlp_shapes(od, 256, 4):
        n = int(np.prod(shp))
        e_ref, e_got = Y.rel_l2(r32[o:o + n], r64[o:o + n]), Y.rel_l2(got[o:o + n], r64[o:o + n])
        allow = 4.0 * e_ref + Y.FLOOR
        print('%s %s: got %.2e, float32 autograd %.2e, allowance %.2e' % (where, shp, e_got, e_ref, allow))
        assert e_got <= allow, (where, shp, e_got, e_ref)
        worst = max(worst, e_got / allow)
        o += n
    return worst


@pytest.mark.parametrize('K', [0, 3])                  # both sides of backward_takes_thin for the critics' and the policy's widths
@pytest.mark.parametrize('rows', [16, 40, 272, 8200])
@pytest.mark.parametrize('cache', [False, True], ids=['strided', 'packed'])
def test_sac_targets_and_policy_grad_vs_float64_autograd(engine, cache, rows, K):
    c = attach_cache(make_case(600 + rows + K, rows, K), cache)
    obs, eps = dev(c['obs']), dev(c['eps'])
    r32, r64 = c['r32'], c['r64']
    y = ops.sac_targets(c['cfg'], c['wp'], c['wq1'], c['wq2'], dev(c['rew']), obs, eps, ALPHA).cpu().numpy()
    print('targets: got %.2e, float32 torch %.2e' % (Y.rel_l2(y, r64['y']), Y.rel_l2(r32['y'], r64['y'])))
    Y.check_values(y, r32['y'], r64['y'], what='soft targets')
    stats, grad = ops.sac_policy_grad(c['cfg'], c['wp'], c['wq1'], c['wq2'], obs, eps, ALPHA)
    check_arrays(grad.cpu().numpy(), r32['grad'], r64['grad'], c['od'], 'rows %d K %d' % (rows, K))
    s = stats.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(s[0], r64['qmin'].sum(), rtol=2e-5, atol=2e-5 * rows)
    np.testing.assert_allclose(s[1], (r64['qmin'] ** 2).sum(), rtol=1e-4, atol=1e-6 * rows)
    np.testing.assert_allclose(s[2], r64['logp'].sum(), rtol=2e-5, atol=2e-5 * rows)


@pytest.mark.parametrize('K', [0, 3])
def test_clipped_log_std(engine, K):
    """the clip of the log-std logits.  (a) logits spread over both sides of [-5, 1] and its inside: the gradient against float64
    autograd, whose clamp has the same rule.  (b) the two log-std biases shifted so that every row of the first sits above +1 and every
    row of the second below -5: the gradients of the log-std columns of the output layer are EXACTLY zero, and the actions use
    sigma = exp(1) and exp(-5)."""
    rows = 272
    c = attach_cache(make_case(700 + K, rows, K, spread=30.0), False)
    obs, eps = dev(c['obs']), dev(c['eps'])
    r32, r64 = c['r32'], c['r64']
    ls = r64['logits'][:, 2:]
    assert (ls > 1).any() and (ls < -5).any() and ((ls > -5) & (ls < 1)).any()
    _, grad = ops.sac_policy_grad(c['cfg'], c['wp'], c['wq1'], c['wq2'], obs, eps, ALPHA)
    check_arrays(grad.cpu().numpy(), r32['grad'], r64['grad'], c['od'], 'spread K %d' % K)

    c = attach_cache(make_case(710 + K, rows, K, shift=(8.0, -12.0)), False)
    obs, eps = dev(c['obs']), dev(c['eps'])
    act, logp, logits = ops.policy_sample(c['cfg'], c['wp'], obs, eps, want_logits=True)
    assert (logits[:, 2] > 1).all() and (logits[:, 3] < -5).all()
    sig = sigma32(torch.tensor([1., -5.], device=DEV))
    assert torch.equal(bits(act), bits(logits[:, :2] + sig * eps))
    _, grad = ops.sac_policy_grad(c['cfg'], c['wp'], c['wq1'], c['wq2'], obs, eps, ALPHA)
    g = grad.cpu().numpy()
    w3, b3 = g[-(256 * 4 + 4):-4].reshape(256, 4), g[-4:]
    assert not w3[:, 2:].any() and not b3[2:].any(), 'a clipped log-std logit has no gradient'
    assert np.abs(w3[:, :2]).max() > 0 and np.abs(b3[:2]).max() > 0
    r32, r64 = c['r32'], c['r64']
    assert not r64['grad'][-2:].any()
    for lo, hi, nm in ((0, c['od'] * 256 + 256 + 65536 + 256, 'hidden'),):
        assert Y.rel_l2(g[lo:hi], r64['grad'][lo:hi]) <= 4.0 * Y.rel_l2(r32['grad'][lo:hi], r64['grad'][lo:hi]) + Y.FLOOR, nm


# ---- 4: SACLearner against the fixtures of the unmodified reference ---------------------------------------------------------
BATCH_KEYS = ('batch_obs', 'batch_actions', 'batch_rewards', 'batch_obs_tp1', 'batch_dones')


def _learner(g, K, **kw):
    from mpg_amd.config import default_args
    from mpg_amd.learners import SACLearner
    from mpg_amd.policy import PolicyWithQs
    from tests import sac_oracle as S
    args = default_args('SAC', replay_batch_size=64, num_future_data=K, gradient_clip_norm=S.CLIP, **kw)
    learner = SACLearner(PolicyWithQs, args)
    pw = learner.policy_with_value
    assert pw.names == ['Q1', 'Q2', 'policy'] and pw.alpha == S.ALPHA
    w = S.fixture_weights(int(g['weights_seed']), K)
    flat = np.concatenate([w[n] for n in pw.names])
    pw.set_flat(flat, (flat * np.float32(g['target_scale'])).astype(np.float32))
    return learner


@pytest.mark.parametrize('K', [0, 3])
def test_compute_gradient_vs_reference_golden(golden, engine, K):
    """the list the reference's SACLearner.compute_gradient returns (18 arrays: clipped Q1, Q2 and policy gradients), its targets and
    its stats, on the same minibatch, weights and recorded draws (tests/golden/make_golden_sac.py)"""
    from tests import sac_oracle as S
    g = golden('sac_H256_B64%s.npz' % ('_K%d' % K if K else ''))
    learner = _learner(g, K)
    pw = learner.policy_with_value
    batch = [dev(g[k]) for k in BATCH_KEYS]
    grads = learner.compute_gradient(batch, None, None, 0, eps_target=dev(g['eps_target']), eps_policy=dev(g['eps_policy']))
    assert len(grads) == 18
    got = torch.cat([x.reshape(-1) for x in grads]).cpu().numpy()
    where = 'SAC K=%d (%s)' % (K, engine)
    worst = Y.check_gradients(got, g['grads'], g['grads_f64'], [(n,) + tuple(pw.dims[n]) for n in pw.names], where=where,
                              small64=g['small64'])
    print(where, 'worst error / allowance %.3f' % worst)
    Y.check_values(learner.batch_data['batch_targets'].cpu().numpy(), g['targets'], g['targets_f64'], what='targets ' + where)
    # the head's log-densities on both draws, through the policy object
    for key, obs_key, eps_key in (('logp_target', 'batch_obs_tp1', 'eps_target'), ('logp_policy', 'batch_obs', 'eps_policy')):
        logp = pw.compute_action(dev(g[obs_key]), dev(g[eps_key]))[1].cpu().numpy()
        Y.check_values(logp, g[key], g[key + '_f64'], what=key + ' ' + where)
    st = learner.get_stats()
    # stats: the tolerances tests/test_ndpg_gpu.py uses for the same quantities
    for k in ('q_loss1', 'q_loss2', 'policy_loss', 'policy_entropy', 'mb_targets_mean', 'value_mean', 'q_gradient_norm1', 'q_gradient_norm2',
              'policy_gradient_norm'):
        np.testing.assert_allclose(st[k], g[k], rtol=1e-4, atol=1e-7, err_msg=k)
    # value_var = E[Q^2] - mean^2: the two terms' 1e-4 relative errors against a difference that is smaller than either
    mean, var = float(g['value_mean_f64']), float(g['value_var_f64'])
    np.testing.assert_allclose(st['value_var'], g['value_var'], rtol=1e-4 * (var + 3 * mean * mean) / var)
    # the returned arrays' norms: min(clip, reference norm) - the critics clipped, the policy not
    assert max(st['q_gradient_norm1'], st['q_gradient_norm2']) > S.CLIP > st['policy_gradient_norm']
    off = np.cumsum([0] + list(pw.sizes))
    for i, k in enumerate(('q_gradient_norm1', 'q_gradient_norm2', 'policy_gradient_norm')):
        n = np.linalg.norm(got[off[i]:off[i + 1]].astype(np.float64))
        np.testing.assert_allclose(n, min(S.CLIP, float(g[k])), rtol=1e-5 if float(g[k]) > S.CLIP else 1e-4, err_msg=k)


# ---- 5: the loop ---------------------------------------------------------------------------------------------------------------
def _stack(seed=0, interval=10, **kw):
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import SACLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    args = default_args('SAC', seed=seed, **kw)
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    learner = SACLearner(PolicyWithQs, args)
    opt = SingleProcessOffPolicyOptimizer(worker, learner, ReplayBuffer(args, 0), None, args, sampling_interval=interval)
    assert opt._fused is None                  # SAC runs through the method-by-method path
    return opt


def _state(opt):
    pw, rb, w, ln = opt.worker.policy_with_value, opt.replay_buffer, opt.worker, opt.learner
    torch.cuda.synchronize()
    tensors = [t.clone() for t in (pw.params, pw.targets, pw.m, pw.v, rb.obs, rb.act, rb.rew, rb.obs2, rb.done, w.obs)]
    counters = (dict(pw.opt_steps), rb._next_idx, len(rb), rb.replay_times, w._noise_ctr, w.env._ctr, ln.counter, pw._sample_ctr,
                opt.num_sampled_steps)
    return tensors, counters


SMALL = dict(interval=3, num_agent=64, batch_size=64, replay_batch_size=128, replay_starts=256, max_buffer_size=1024)


def test_loop_is_finite_reproducible_and_resumes_bit_identically(tmp_path, engine):
    """20 iterations of SingleProcessOffPolicyOptimizer with SACLearner: every parameter finite; a second run from the same seed is
    bit-identical; a checkpoint written at iteration 7 and loaded into a fresh stack built with ANOTHER seed, run for iterations
    8 .. 19, ends with parameters, Adam moments, ring and counters bit-identical to the uninterrupted run"""
    from mpg_amd.checkpoint import load_checkpoint, save_checkpoint
    a = _stack(seed=5, **SMALL)
    for _ in range(8):
        a.step()
    path = save_checkpoint(str(tmp_path / 'ckpt.npz'), a)
    for _ in range(12):
        a.step()
    ta, ca = _state(a)
    assert all(torch.isfinite(t).all() for t in ta[:4])
    assert ca[0] == {'Q1': 20, 'Q2': 20, 'policy': 20}                 # delay_update 1
    st = a.learner.get_stats()
    assert all(np.isfinite(st[k]) for k in ('q_loss1', 'q_loss2', 'policy_loss', 'policy_entropy', 'value_mean', 'value_var'))
    a.worker.policy_with_value.check_status()
    b = _stack(seed=5, **SMALL)
    for _ in range(20):
        b.step()
    tb, cb = _state(b)
    assert ca == cb, (ca, cb)
    for i, (x, y) in enumerate(zip(ta, tb)):
        assert torch.equal(x, y), i
    c = _stack(seed=99, **SMALL)                # different seed: every stream must come from the file
    meta = load_checkpoint(path, c)
    assert meta['optimizer']['iteration'] == 8 and c.iteration == 8 and meta['learner_cls'] == 'SACLearner'
    for _ in range(12):
        c.step()
    tc, cc = _state(c)
    assert ca == cc, (ca, cc)
    for i, (x, y) in enumerate(zip(ta, tc)):
        assert torch.equal(x, y), i


# ---- 6: the worker -------------------------------------------------------------------------------------------------------------
def test_worker_samples_from_the_stochastic_policy(engine):
    from mpg_amd.config import default_args
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    n = 4096
    args = default_args('SAC', seed=3, num_agent=n, batch_size=n)

    def worker():
        w = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
        pw = w.policy_with_value
        # an output layer with some weight on the log-std columns and a shifted bias: sigma varies over the agents, some clipped at e
        rng = np.random.Generator(np.random.PCG64(11))
        flat = mlp_weights_flat(rng, 6, 4)
        flat[-(256 * 4 + 4):-4].reshape(256, 4)[:, 2:] *= 4.0
        flat[-2:] += np.float32(0.5)
        pw.set_flat(np.concatenate([pw.net('Q1').cpu().numpy(), pw.net('Q2').cpu().numpy(), flat]))
        return w
    w1, w2 = worker(), worker()
    pw = w1.policy_with_value
    obs0 = w1.obs.clone()
    assert w1.explore_sigma is None
    b1, b2 = w1.sample(), w2.sample()
    for x, y in zip(b1, b2):
        assert torch.equal(x, y)                                  # two workers, one seed
    obs, act = b1[0], b1[1]
    assert torch.equal(obs, obs0) and act.shape == (n, 2)
    # the stored action is the sample itself, un-clipped: the head on the worker's own draw (counter 0 of its stream)
    eps = ops.normal_fill(n * 2, w1.seed, 0, obs.device).view(n, 2)
    a_ref, _, logits = ops.policy_sample(pw.cfg, pw.net('policy'), obs, eps, want_logits=True)
    assert torch.equal(bits(act), bits(a_ref))
    assert act.abs().max().item() > 1.2                           # beyond anything a clip to the env's action range would leave
    mode = pw.compute_mode(obs)
    assert torch.equal(bits(mode), bits(logits[:, :2]))
    sigma = sigma32(logits[:, 2:])
    assert sigma.max().item() > 2 * sigma.min().item()            # (sigma varies over the agents)
    z = ((act - mode) / sigma).double().cpu().numpy()
    # z is the standard-normal draw: its mean over the 4096 agents is within 5 standard errors of 0, per action dimension
    se = z.std(0) / np.sqrt(n)
    assert (np.abs(z.mean(0)) <= 5 * se).all(), (z.mean(0), se)
    assert (np.abs(z.std(0) - 1) < 0.05).all()
    b3 = w1.sample()
    assert not torch.equal(b3[1], act)                            # the next call draws anew
