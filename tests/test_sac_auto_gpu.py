"""SAC's learned temperature (alpha = 'auto') on the GPU, both engines.
 1. the device-temperature entry points equal the host-alpha ones bit for bit, given alpha = float32(exp(float64(log_alpha)));
 2. the second sum of the head's pass (k_row_sums<HeadRow2>): the same tree as logp_sum on the same draw, and the float64 sum of
    mpg_policy_sample's log-densities on an independent one, in the one-block and the many-block form;
 3. mpg_sac_alpha_update: clip, snapshot, Adam against mpg_adam_polyak on a one-element segment, skip flags;
 4. SACLearner / PolicyWithQs with alpha = 'auto': repeated launches, the training loop (reproducible, resumes bit-identically, the
    temperature's Adam steps on even iterations only under delay_update 2), two unequal shards;
 5. SACLearner('auto') against the fixtures of the unmodified reference (tests/golden/make_golden_sac_auto.py): compute_gradient on
    one process and on two ranks, and the six-iteration loop of the H = 32 fixture's batch and draws at H = 256 against the
    restatement (tests/sac_auto_oracle.py, which that fixture pins)."""
import numpy as np
import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops
from mpg_amd.policy import adam_step_size
from tests.test_sac_gpu import attach_cache, bits, dev, make_case

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LOG_ALPHA = np.float32(np.log(0.2))             # alpha neither 1 nor the fixed default 0.03
ROWS = (16, 272, 8200)                          # one block; one block beyond 256 rows; the many-block form (ERR_MB_MIN_ROWS = 8192)


@pytest.fixture(params=['split', 'f32'])
def engine(request):
    with L.engine(request.param):
        yield request.param


def host_alpha(log_alpha):
    """the kernels' rule, re-formed on the host: the correctly rounded float32 exponential"""
    return float(np.float32(np.exp(np.float64(log_alpha))))


def case_on_device(rows, K):
    c = attach_cache(make_case(900 + rows + K, rows, K), False)
    rng = np.random.Generator(np.random.PCG64(77 + rows + K))
    c['d'] = dict(obs=dev(c['obs']), eps=dev(c['eps']), rew=dev(c['rew']), eps_alpha=dev(rng.standard_normal((rows, 2)).astype(np.float32)),
                  log_alpha=dev(np.array([LOG_ALPHA])))
    return c


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [0, 3])
@pytest.mark.parametrize('rows', ROWS)
def test_device_temperature_forms_equal_the_host_alpha_ones(engine, rows, K):
    c = case_on_device(rows, K)
    d, cfg, alpha = c['d'], c['cfg'], host_alpha(LOG_ALPHA)
    y_host = ops.sac_targets(cfg, c['wp'], c['wq1'], c['wq2'], d['rew'], d['obs'], d['eps'], alpha)
    y_auto = ops.sac_targets_auto(cfg, c['wp'], c['wq1'], c['wq2'], d['rew'], d['obs'], d['eps'], d['log_alpha'])
    assert torch.equal(bits(y_auto), bits(y_host))
    s_host, g_host = ops.sac_policy_grad(cfg, c['wp'], c['wq1'], c['wq2'], d['obs'], d['eps'], alpha)
    s_auto, g_auto, ag = ops.sac_policy_grad_auto(cfg, c['wp'], c['wq1'], c['wq2'], d['obs'], d['eps'], d['log_alpha'], d['eps_alpha'], -2.0)
    assert torch.equal(bits(g_auto), bits(g_host))
    assert torch.equal(bits(s_auto), bits(s_host))            # qmin_sum, qmin_sqsum, logp_sum
    assert torch.isfinite(ag).all()
    # alpha is READ on the device: another log_alpha, another alpha term, without a new call argument
    d['log_alpha'].fill_(0.0)
    y_one = ops.sac_targets_auto(cfg, c['wp'], c['wq1'], c['wq2'], d['rew'], d['obs'], d['eps'], d['log_alpha'])
    assert torch.equal(bits(y_one), bits(ops.sac_targets(cfg, c['wp'], c['wq1'], c['wq2'], d['rew'], d['obs'], d['eps'], 1.0)))
    assert not torch.equal(bits(y_one), bits(y_host))


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [0, 3])
@pytest.mark.parametrize('rows', ROWS)
def test_second_sum(engine, rows, K):
    c = case_on_device(rows, K)
    d, cfg = c['d'], c['cfg']
    args = (cfg, c['wp'], c['wq1'], c['wq2'], d['obs'], d['eps'], d['log_alpha'])
    for inv_b in (1.0 / rows, 1.0 / (rows + 40)):             # the whole batch, and a shard of a larger one
        # the same draw and target_entropy 0: the second sum is the first one's tree, finished as -inv_b * sum
        stats, _, ag = ops.sac_policy_grad_auto(*args, d['eps'], 0.0, inv_b_global=inv_b)
        want = -torch.tensor(inv_b, dtype=torch.float32, device=DEV) * stats[2:3]
        assert torch.equal(bits(ag), bits(want)), (ag.item(), want.item())
    # an independent draw: against the float64 sum of the head's own log-densities on it
    for h in (-2.0, 3.0):
        inv_b = 1.0 / rows
        _, _, ag = ops.sac_policy_grad_auto(*args, d['eps_alpha'], h, inv_b_global=inv_b)
        logp = ops.policy_sample(cfg, c['wp'], d['obs'], d['eps_alpha'])[1].double().cpu().numpy()
        terms = logp + h
        want = -inv_b * terms.sum()
        bound = rows * 2.0 ** -24 * np.abs(terms).sum() * inv_b         # the standard bound of a float32 sum of `rows` terms
        print('rows %d K %d H %g: alpha_grad %.7g, float64 %.7g, error %.2e, bound %.2e' % (rows, K, h, ag.item(), want, abs(ag.item() - want), bound))
        assert abs(ag.item() - want) <= bound


def test_hundred_launches_are_bit_identical(engine):
    for rows in (272, 8200):
        c = case_on_device(rows, 0)
        d, cfg = c['d'], c['cfg']
        args = (cfg, c['wp'], c['wq1'], c['wq2'], d['obs'], d['eps'], d['log_alpha'], d['eps_alpha'], -2.0)
        keep = [t.clone() for t in ops.sac_policy_grad_auto(*args)]
        for _ in range(100):
            for a, b in zip(ops.sac_policy_grad_auto(*args), keep):
                assert torch.equal(bits(a), bits(b))


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
SCHED = (8e-5, 100000, 8e-6)


def make_desc(state, opt_steps=0):
    d = ops.SacAlphaStruct()
    d.state, d.target_entropy, d.opt_steps = state.data_ptr(), -2.0, opt_steps
    for i in range(3):
        d.lr[i] = SCHED[i]
    return d


def fresh_state(m=0.0, v=0.0):
    return dev(np.array([LOG_ALPHA, m, v, 0, 0, 0, 0, 0], np.float32))


@pytest.mark.parametrize('g0,clip', [(5.27, 1.0), (-5.05, 1.0), (-0.2, 1.0), (0.75, 0.5), (1.0, 1.0)])
def test_alpha_update_clip_and_snapshot(engine, g0, clip):
    """tf.clip_by_global_norm of the one-element list, in float32 like the kernel: norm |g|, g * clip * min(1 / |g|, 1 / clip)"""
    f = np.float32
    state, g = fresh_state(), dev(np.array([g0], f))
    d = make_desc(state)
    ops.sac_alpha_update(d, g, clip=clip, do_clip=True)
    nrm = abs(f(g0))
    want = f(g0) * (f(clip) * min(f(1) / nrm, f(1) / f(clip)))
    assert g.item() == want and (abs(want) <= clip * (1 + 2 ** -23))
    assert (abs(g0) <= clip) == (g.item() == f(g0))                      # below the clip the gradient passes as it is
    s = state.cpu().numpy()
    assert s[0] == LOG_ALPHA and s[1] == 0 and s[2] == 0                  # no Adam step was asked for
    assert s[3] == f(host_alpha(LOG_ALPHA)) and s[4] == LOG_ALPHA * f(g0) and s[5] == nrm and s[6] == 0 and s[7] == 0
    assert d.opt_steps == 0


def adam_reference(la, m, v, g, steps_done, skip=None):
    """mpg_adam_polyak on a one-element segment (it accepts one: sizes [1], no weight cache, no target)"""
    w, mm, vv = dev(np.array([la], np.float32)), dev(np.array([m], np.float32)), dev(np.array([v], np.float32))
    ops.adam_polyak(w, mm, vv, None, dev(np.array([g], np.float32)), [1], [adam_step_size(SCHED, steps_done)], [1], [0], 0.005, skip_flag=skip)
    return torch.cat([w, mm, vv])


def test_alpha_update_adam_is_adam_polyak_on_one_element(engine):
    state = fresh_state()
    d = make_desc(state, opt_steps=40)
    for step, g0 in enumerate((5.27, -0.2, 1e-3, -3.0)):
        before = state.cpu().numpy()
        g = dev(np.array([g0], np.float32))
        ops.sac_alpha_update(d, g, do_adam=True)
        want = adam_reference(before[0], before[1], before[2], g0, 40 + step)
        assert torch.equal(bits(state[:3]), bits(want)), (step, state[:3].tolist(), want.tolist())
        assert g.item() == np.float32(g0) and d.opt_steps == 41 + step
    assert state[0].item() != LOG_ALPHA and not state[3:].any()          # do_adam alone leaves the snapshot alone


@pytest.mark.parametrize('g0', [5.27, -0.2])
def test_clip_then_adam_in_two_calls_is_the_one_call(engine, g0):
    a, b = fresh_state(0.3, 0.01), fresh_state(0.3, 0.01)
    ga, gb = dev(np.array([g0], np.float32)), dev(np.array([g0], np.float32))
    da, db = make_desc(a, 7), make_desc(b, 7)
    ops.sac_alpha_update(da, ga, clip=1.0, do_clip=True)
    ops.sac_alpha_update(da, ga, do_adam=True)
    ops.sac_alpha_update(db, gb, clip=1.0, do_clip=True, do_adam=True)
    assert torch.equal(bits(a), bits(b)) and torch.equal(bits(ga), bits(gb)) and da.opt_steps == db.opt_steps == 8
    # and the step was made with the CLIPPED gradient
    want = adam_reference(LOG_ALPHA, 0.3, 0.01, ga.item(), 7)
    assert torch.equal(bits(b[:3]), bits(want))
    assert b[3].item() == np.float32(host_alpha(LOG_ALPHA))               # the snapshot is alpha BEFORE the step


def test_skip_flags_and_a_non_finite_gradient_give_adam_a_zero_gradient(engine):
    zero = adam_reference(LOG_ALPHA, 0.3, 0.01, 0.0, 5)
    # a network's flag (optimizer.py:357-361: any NaN zeroes the whole list); the counter still advances
    state, flags = fresh_state(0.3, 0.01), torch.tensor([0, 1, 0], dtype=torch.int32, device=DEV)
    d = make_desc(state, 5)
    ops.sac_alpha_update(d, dev(np.array([5.27], np.float32)), clip=1.0, do_clip=True, do_adam=True, skip_flag=flags)
    assert torch.equal(bits(state[:3]), bits(zero)) and d.opt_steps == 6 and state[6].item() == 0
    # clear flags change nothing
    state = fresh_state(0.3, 0.01)
    d = make_desc(state, 5)
    ops.sac_alpha_update(d, dev(np.array([0.5], np.float32)), clip=1.0, do_clip=True, do_adam=True, skip_flag=torch.zeros_like(flags))
    assert torch.equal(bits(state[:3]), bits(adam_reference(LOG_ALPHA, 0.3, 0.01, 0.5, 5)))
    # the temperature's own gradient not finite: its flag is set at the clip and holds for the Adam call that follows
    for bad in (float('nan'), float('inf')):
        state = fresh_state(0.3, 0.01)
        d = make_desc(state, 5)
        g = dev(np.array([bad], np.float32))
        ops.sac_alpha_update(d, g, clip=1.0, do_clip=True)
        assert state[6].item() == 1
        ops.sac_alpha_update(d, g, do_adam=True)
        assert torch.equal(bits(state[:3]), bits(zero)) and torch.isfinite(state[:3]).all()


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
def _stack(seed=0, interval=10, **kw):
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import SACLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    args = default_args('SAC', seed=seed, alpha='auto', target_entropy=-2., delay_update=2, **kw)
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    learner = SACLearner(PolicyWithQs, args)
    opt = SingleProcessOffPolicyOptimizer(worker, learner, ReplayBuffer(args, 0), None, args, sampling_interval=interval)
    assert opt._fused is None                  # the method-by-method path
    return opt


def _state(opt):
    pw, rb, w, ln = opt.worker.policy_with_value, opt.replay_buffer, opt.worker, opt.learner
    torch.cuda.synchronize()
    tensors = [t.clone() for t in (pw.params, pw.targets, pw.m, pw.v, pw.alpha_state, rb.obs, rb.act, rb.rew, rb.obs2, rb.done, w.obs)]
    counters = (dict(pw.opt_steps), pw.alpha_opt_steps, rb._next_idx, len(rb), rb.replay_times, w._noise_ctr, w.env._ctr, ln.counter,
                pw._sample_ctr, opt.num_sampled_steps)
    return tensors, counters


SMALL = dict(interval=3, num_agent=64, batch_size=64, replay_batch_size=128, replay_starts=256, max_buffer_size=1024)


def test_loop_learns_the_temperature_reproducibly_and_resumes_bit_identically(tmp_path, engine):
    """20 iterations of SingleProcessOffPolicyOptimizer with SACLearner('auto'), delay_update 2: log_alpha moves on even iterations only
    (policy.py:136-143), with its own Adam and counter; a second run from the same seed is bit-identical; a checkpoint written at
    iteration 8 and loaded into a stack built with ANOTHER seed ends bit-identical to the uninterrupted run"""
    from mpg_amd.checkpoint import load_checkpoint, save_checkpoint
    a = _stack(seed=5, **SMALL)
    pw = a.worker.policy_with_value
    assert a.learner.policy_with_value is pw and pw.log_alpha.item() == 0.0
    trace = []
    for it in range(8):
        a.step()
        st = a.learner.get_stats()
        trace.append((pw.log_alpha.item(), st))
    path = save_checkpoint(str(tmp_path / 'ckpt.npz'), a)
    for i, (la, st) in enumerate(trace):
        before = 0.0 if i == 0 else trace[i - 1][0]
        assert (la != before) == (i % 2 == 0), (i, la, before)                 # the temperature's Adam: even iterations only
        # the snapshot is alpha BEFORE the update of the same iteration, under the kernels' rule
        assert st['alpha'] == np.float32(host_alpha(np.float32(before)))
        assert np.isfinite(st['alpha_loss']) and st['alpha_gradient_norm'] > 0 and st['alpha_time'] is None
        assert (st['alpha_loss'] == 0.0) == (i == 0)                            # alpha_loss = log_alpha * g, and log_alpha starts at 0
    # the first step: m = 0.1 g, v = 0.001 g^2 => log_alpha moves by lr_t * m / (sqrt(v) + eps) ~ lr, against the gradient's sign;
    # entropy above the target of -2 => the gradient -(mean logp + H) is positive => log_alpha falls
    assert trace[0][0] < 0 and abs(trace[0][0] + 8e-5) < 1e-6
    for _ in range(12):
        a.step()
    ta, ca = _state(a)
    assert all(torch.isfinite(t).all() for t in ta[:5])
    assert ca[0] == {'Q1': 20, 'Q2': 20, 'policy': 10} and ca[1] == 10
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
    assert meta['optimizer']['iteration'] == 8 and c.iteration == 8 and meta['policy']['alpha_opt_steps'] == 4
    for _ in range(12):
        c.step()
    tc, cc = _state(c)
    assert ca == cc, (ca, cc)
    for i, (x, y) in enumerate(zip(ta, tc)):
        assert torch.equal(x, y), i


def test_checkpoints_of_fixed_and_learned_temperature_do_not_mix(tmp_path, engine):
    from mpg_amd.checkpoint import load_checkpoint, save_checkpoint, state_of
    from tests.test_sac_gpu import _stack as fixed_stack
    fixed, auto = fixed_stack(seed=5, **SMALL), _stack(seed=5, **SMALL)
    meta, arrays = state_of(fixed)
    assert 'policy/alpha_state' not in arrays and 'alpha_opt_steps' not in meta['policy']        # a fixed-alpha file keeps its content
    with pytest.raises(ValueError, match='temperature'):
        load_checkpoint(save_checkpoint(str(tmp_path / 'fixed.npz'), fixed), auto)
    with pytest.raises(ValueError, match='temperature'):
        load_checkpoint(save_checkpoint(str(tmp_path / 'auto.npz'), auto), fixed)


@pytest.mark.parametrize('K', [0, 3])
def test_two_unequal_shards(engine, K):
    """24 + 40 rows with inv_b_global = 1 / 64, in one process with the harness of tests/test_sharding_gpu.py (sharded / check_arrays /
    check_scaling): the shares of the temperature's gradient add up to the whole batch's -(mean logp_alpha + target_entropy) within the
    summation bound of test_second_sum, the policy gradient's to float64 autograd's under the rule of tests/yardstick.py, with alpha
    read on the device"""
    from tests import test_sharding_gpu as T
    from tests.test_sac_gpu import reference
    B, cut, H = 64, 24, -2.0
    c = T.net_case(970 + K, B, K)
    alpha = host_alpha(LOG_ALPHA)
    r32, r64 = reference(c, torch.float32, alpha), reference(c, torch.float64, alpha)
    cfg = ops.make_cfg(obs_dim=c['od'], obs_scale=c['scale'], policy_out_activation='linear', gamma=c['gamma'])
    wp, q1, q2, obs, eps = dev(c['w']['policy']), dev(c['w']['Q1']), dev(c['w']['Q2']), dev(c['obs']), dev(c['eps'])
    eps_alpha = dev(np.random.Generator(np.random.PCG64(5 + K)).standard_normal((B, 2)).astype(np.float32))
    log_alpha = dev(np.array([LOG_ALPHA]))

    def run(lo, hi, inv_b):
        stats, grad, ag = ops.sac_policy_grad_auto(cfg, wp, q1, q2, T.rows_of(obs, lo, hi), T.rows_of(eps, lo, hi), log_alpha,
                                                   T.rows_of(eps_alpha, lo, hi), H, inv_b_global=inv_b)
        return dict(stats=stats, grad=grad, alpha_grad=ag)
    whole, parts = T.sharded(run, B, cut)
    where = 'sac_policy_grad_auto B %d = %d + %d K %d (%s)' % (B, cut, B - cut, K, engine)
    T.check_arrays(T.host(parts[0]['grad'] + parts[1]['grad']), T.host(whole['grad']), r32['grad'], r64['grad'], [('policy', c['od'], 4)], where)
    terms = ops.policy_sample(cfg, wp, obs, eps_alpha)[1].double().cpu().numpy() + H
    want, bound = -terms.sum() / B, B * 2.0 ** -24 * np.abs(terms).sum() / B
    got = (parts[0]['alpha_grad'] + parts[1]['alpha_grad']).item()               # the all-reduce's float32 sum of the two shares
    print('   %s: temperature gradient %.7g, float64 %.7g, unsharded %.7g, bound %.2e' % (where, got, want, whole['alpha_grad'].item(), bound))
    assert abs(got - want) <= bound and abs(whole['alpha_grad'].item() - want) <= bound
    for lo, hi in ((0, cut), (cut, B)):
        T.check_scaling(run, lo, hi, ('grad', 'alpha_grad'), ('stats',), where)


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
BATCH_KEYS = ('batch_obs', 'batch_actions', 'batch_rewards', 'batch_obs_tp1', 'batch_dones')
NEW_STATS = ('alpha', 'alpha_loss', 'alpha_gradient_norm')


def _learner(g, K, rows=64, weights=None, **kw):
    from mpg_amd.config import default_args
    from mpg_amd.learners import SACLearner
    from mpg_amd.policy import PolicyWithQs
    from tests import sac_oracle as S
    args = default_args('SAC', replay_batch_size=rows, num_future_data=K, gradient_clip_norm=S.CLIP, alpha='auto',
                        target_entropy=float(g['target_entropy']), **kw)
    learner = SACLearner(PolicyWithQs, args)
    pw = learner.policy_with_value
    assert pw.names == ['Q1', 'Q2', 'policy'] and pw.alpha == 'auto' and learner.alpha == 'auto'
    w = weights if weights is not None else S.fixture_weights(int(g['weights_seed']), K)
    flat = np.concatenate([w[n] for n in pw.names])
    pw.set_flat(flat, (flat * np.float32(g['target_scale'])).astype(np.float32))
    pw.log_alpha.fill_(float(LOG_ALPHA))
    return learner


def check_against_fixture(learner, grads, g, where, targets_rows=slice(None)):
    from tests import sac_oracle as S
    from tests import yardstick as Y
    pw = learner.policy_with_value
    assert len(grads) == 19 and grads[18].shape == ()
    got = torch.cat([x.reshape(-1) for x in grads[:18]]).cpu().numpy()
    assert torch.equal(learner.flat_grad[:-1], torch.cat([x.reshape(-1) for x in grads[:18]])) and learner.flat_grad[-1] == grads[18]
    worst = Y.check_gradients(got, g['grads'], g['grads_f64'], [(n,) + tuple(pw.dims[n]) for n in pw.names], where=where,
                              small64=g['small64'])
    print(where, 'worst error / allowance %.3f' % worst)
    Y.check_values(grads[18].cpu().numpy(), g['alpha_grad'], g['alpha_grad_f64'], what='temperature gradient ' + where)
    Y.check_values(learner.batch_data['batch_targets'].cpu().numpy(), g['targets'][targets_rows], g['targets_f64'][targets_rows],
                   what='targets ' + where)
    st = learner.get_stats()
    for k in NEW_STATS + ('q_loss1', 'q_loss2', 'policy_loss', 'policy_entropy', 'value_mean', 'q_gradient_norm1', 'q_gradient_norm2',
                          'policy_gradient_norm'):              # the tolerances of tests/test_sac_gpu.py for the same quantities
        np.testing.assert_allclose(st[k], g[k], rtol=1e-4, atol=1e-7, err_msg=k)
    assert st['alpha_time'] is None and st['alpha'] == np.float32(host_alpha(LOG_ALPHA))
    assert st['alpha_gradient_norm'] > S.CLIP and abs(abs(grads[18].item()) - 1.0) < 1e-6        # clipped: g / |g|
    return st


@pytest.mark.parametrize('K', [0, 3])
def test_compute_gradient_vs_reference_golden(golden, engine, K):
    g = golden('sac_auto_H256_B64%s.npz' % ('_K%d' % K if K else ''))
    learner = _learner(g, K)
    grads = learner.compute_gradient([dev(g[k]) for k in BATCH_KEYS], None, None, 0, eps_target=dev(g['eps_target']),
                                     eps_policy=dev(g['eps_policy']), eps_alpha=dev(g['eps_alpha']))
    st = check_against_fixture(learner, grads, g, 'SAC auto K=%d (%s)' % (K, engine))
    np.testing.assert_allclose(st['mb_targets_mean'], g['mb_targets_mean'], rtol=1e-4, atol=1e-7)
    # the statistics are a snapshot: the update that follows does not move them
    pw = learner.policy_with_value
    pw.apply_gradients(0, learner.flat_grad)
    assert pw.log_alpha.item() != LOG_ALPHA and pw.alpha_opt_steps == 1
    again = learner.get_stats()
    assert all(again[k] == st[k] for k in NEW_STATS)
    # the reference's call - the list of 19 host arrays - is taken too
    pw.apply_gradients(2, [x.cpu().numpy() for x in grads])
    assert pw.alpha_opt_steps == 2


@pytest.mark.parametrize('K', [0, 3])
def test_learner_two_shards_vs_reference_golden(golden, monkeypatch, engine, K):
    """two ranks of 32 rows each through the harness of tests/test_sharding_gpu.py (one all-reduce of [grads | alpha grad | stats]):
    rank 0 holds the whole batch's gradients, the temperature's included"""
    from tests import test_sharding_gpu as T
    g = golden('sac_auto_H256_B64%s.npz' % ('_K%d' % K if K else ''))
    learner, grads = T.on_two_ranks(monkeypatch, lambda: _learner(g, K, rows=32), lambda ln, lo, hi: ln.compute_gradient(
        T.shard_batch(g, lo, hi), None, None, 0, eps_target=dev(g['eps_target'][lo:hi]), eps_policy=dev(g['eps_policy'][lo:hi]),
        eps_alpha=dev(g['eps_alpha'][lo:hi])))
    lo, hi = T.SHARDS[0]
    check_against_fixture(learner, grads, g, 'SAC auto K=%d two shards (%s)' % (K, engine), slice(lo, hi))


def test_six_iteration_loop_vs_the_restatement(golden, engine):
    """compute_gradient + apply_gradients for six iterations, delay_update 2, on the loop fixture's batch and recorded draws with
    256-unit networks, against tests/sac_auto_oracle.py (float32 and float64) - the restatement that the fixture, made by the reference
    itself at H = 32, pins in tests/test_sac_auto_golden.py"""
    from tests import sac_oracle as S
    from tests import yardstick as Y
    g = golden('sac_auto_loop_H32_B64.npz')
    n, w = int(g['n_iter']), S.fixture_weights(2, 0)
    oracle = _oracle_loop()
    learner = _learner(g, 0, weights=w, delay_update=2)
    pw = learner.policy_with_value
    batch = [dev(g[k]) for k in BATCH_KEYS]
    la, ag, an = [], [], []
    for it in range(n):
        grads = learner.compute_gradient(batch, None, None, it, *[dev(e) for e in g['eps'][it]])
        ag.append(grads[18].item()), an.append(learner.get_stats()['alpha_gradient_norm'])
        pw.apply_gradients(it, learner.flat_grad)
        la.append(pw.log_alpha.item())
    before = [float(LOG_ALPHA)] + la[:-1]
    assert all((la[it] != before[it]) == (it % 2 == 0) for it in range(n))          # the temperature's Adam: even iterations only
    assert pw.alpha_opt_steps == 3 and pw.opt_steps == {'Q1': 6, 'Q2': 6, 'policy': 3}
    o32, o64 = oracle[torch.float32], oracle[torch.float64]
    Y.check_values(la, o32['la'], o64['la'], what='log_alpha trajectory')
    move = lambda x: np.asarray(x, np.float64) - float(LOG_ALPHA)
    e_ref, e_got = Y.rel_l2(move(o32['la']), move(o64['la'])), Y.rel_l2(move(la), move(o64['la']))
    print('log_alpha movement (%s): device %.2e, float32 restatement %.2e from the float64 one' % (engine, e_got, e_ref))
    # (floor: a float32 log_alpha in [1, 2) is stored to half an ulp, 2^-24, per entry; tests/test_sac_auto_golden.py)
    assert e_got <= 4.0 * e_ref + np.sqrt(n) * 2.0 ** -24 / np.linalg.norm(move(o64['la']))
    Y.check_values(ag, o32['ag'], o64['ag'], what='temperature gradients')
    Y.check_values(an, o32['an'], o64['an'], what='their norms')
    w0 = np.concatenate([w[k] for k in pw.names]).astype(np.float64)
    e_ref, e_got = Y.rel_l2(o32['w'] - w0, o64['w'] - w0), Y.rel_l2(pw.params.cpu().numpy() - w0, o64['w'] - w0)
    print('parameter update (%s): device %.2e, float32 restatement %.2e from the float64 one' % (engine, e_got, e_ref))
    assert e_got <= 4.0 * e_ref + Y.FLOOR


_ORACLE = {}


def _oracle_loop():
    """the restatement's six iterations at H = 256 in float32 and float64: computed once, shared by the engines, never written to"""
    if not _ORACLE:
        import os
        from tests import sac_auto_oracle as A
        from tests import sac_oracle as S
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sac_auto_loop_H32_B64.npz'))
        w = S.fixture_weights(2, 0)
        for dt in (torch.float32, torch.float64):
            cfg = S.make_cfg(0, 256)
            cfg.delay_update = 2
            loop = A.Loop(cfg, w, {k: (v * np.float32(g['target_scale'])).astype(np.float32) for k, v in w.items()}, LOG_ALPHA,
                          float(g['target_entropy']), dt)
            la, ag, an = [], [], []
            for it in range(int(g['n_iter'])):
                grads, st = loop.step(it, [g[k] for k in BATCH_KEYS], *g['eps'][it])
                la.append(float(loop.log_alpha[0])), ag.append(float(grads[18])), an.append(float(st['alpha_gradient_norm']))
            _ORACLE[dt] = dict(la=np.array(la), ag=np.array(ag), an=np.array(an),
                               w=np.concatenate([loop.w[k] for k in ('Q1', 'Q2', 'policy')]).astype(np.float64))
    return _ORACLE
