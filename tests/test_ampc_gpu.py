"""AMPC on the device, both engines: AMPCLearner against the fixtures of the unmodified reference (tests/golden/make_golden_ampc.py),
mpg_ampc_pg against float64 torch autograd of the restated rollout (tests/ampc_oracle.py) under the rule of tests/yardstick.py (error
against float64 at most 4 x float32 autograd's own + FLOOR, and at most 1e-4), the missing discount, the existing critic path at a zero
critic, refusals, determinism, checkpoint resume, the optimizer step and data-parallel scaling in one process."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops
from oracle import mpg_oracle as O
from tests import ampc_oracle as A
from tests import dp_oracle as DP
from tests import yardstick as Y
from tests.golden_inputs import mlp_weights_flat, reset_law_obs

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PD = 'InvertedPendulumConti-v0'
PT = 'PathTracking-v0'
BAR = 1e-4


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(params=['split', 'f32'])
def engine(request):
    """both builds of the library (mpg_amd/_lib.py ENGINES): the split-fp16 product and the exact-fp32 engine"""
    with L.engine(request.param):
        yield request.param


# ---- 1: the learner against the reference ---------------------------------------------------------------------------------------
def _learner(g, name):
    from mpg_amd.config import default_args
    from mpg_amd.learners import AMPCLearner
    from mpg_amd.policy import PolicyWithQs
    env, K = A.FIXTURES[name]
    rows = g['batch_obs'].shape[0]
    args = default_args('AMPC', env_id=env, num_future_data=K, replay_batch_size=rows, M=int(g['M']),
                        num_rollout_list_for_policy_update=[int(g['n'])], gradient_clip_norm=float(g['clip']))
    learner = AMPCLearner(PolicyWithQs, args)
    pw = learner.policy_with_value
    assert pw.names == ['policy'] and len(pw.get_weights()) == 1
    cfg = A.make_cfg(env, K, n=int(g['n']), M=int(g['M']))
    assert (pw.cfg.obs_dim, pw.cfg.act_dim) == (cfg.obs_dim, cfg.act_dim)
    pw.set_flat(A.fixture_weights(int(g['weights_seed']), cfg)['policy'])
    return learner, cfg


@pytest.mark.parametrize('name', sorted(A.FIXTURES))
def test_compute_gradient_vs_reference_golden(golden, engine, name):
    """the list the reference's AMPCLearner.compute_gradient returns (the policy's six clipped gradient arrays) and its stats, on the
    same start observations, weights and recorded model noise"""
    g = golden(name)
    learner, cfg = _learner(g, name)
    obs, rows = dev(g['batch_obs']), g['batch_obs'].shape[0]
    batch = [obs, torch.zeros(rows, cfg.act_dim, device=DEV), torch.zeros(rows, device=DEV), obs, torch.zeros(rows, device=DEV)]
    grads = learner.compute_gradient(batch, None, None, 0, eps=dev(g['eps']) if 'eps' in g else None)
    assert len(grads) == 6
    got = torch.cat([x.reshape(-1) for x in grads]).cpu().numpy()
    st = learner.get_stats()
    assert set(st) == {'iteration', 'pg_time', 'policy_loss', 'policy_gradient_norm'}
    where = '%s (%s)' % (name, engine)
    for k in A.STATS:          # every figure before anything is asserted
        print('%s %-22s vs float64 %.3e (reference float32 %.3e)' % (where, k, Y.rel_l2(st[k], g[k + '_f64']), Y.rel_l2(g[k], g[k + '_f64'])))
    lay, _ = Y.layout([('policy',) + A.policy_dims(cfg)])
    for nm, shp, o, cnt in lay:
        idx = np.arange((o + 7) // 8 * 8, o + cnt, 8)
        if idx.size >= 8:
            r64 = g['grads_f64'][idx // 8]
            e_ref, e_got = Y.rel_l2(g['grads'][idx], r64), Y.rel_l2(got[idx], r64)
            print('   %s %-10s vs float64 %.3e  reference float32 %.3e  error / allowance %.3f' % (where, shp, e_got, e_ref, e_got / (4 * e_ref + Y.FLOOR)))
    worst = Y.check_gradients(got, g['grads'], g['grads_f64'], [('policy',) + A.policy_dims(cfg)], where=where, small64=g['small64'])
    print(where, 'gradient: worst error / allowance %.3f' % worst)
    for k in A.STATS:
        Y.check_values(st[k], g[k], g[k + '_f64'], what='%s %s' % (where, k))
    assert learner.policy_with_value.check_status() == 0


# ---- 2: the entry point against float64 autograd -------------------------------------------------------------------------------
# (env, rows, M, n, K, output activation, packed weight image, noise: 'eps' given / 'philox' drawn in the kernel / None: no noise)
# Forms: packed, M = 1 and the base width take the THIN reverse sweep (n = 1, 2, 25, 31 below; 4112 rows = 257 row groups, more than
# the 256 workgroups that leave a thin partial); K > 0 and the double pendulum the WIDE sweeps; everything else the base sweeps.
CASES = [
    (PT, 16, 1, 1, 0, 'tanh', True, 'eps'),
    (PT, 48, 1, 2, 0, 'tanh', True, 'eps'),
    (PT, 48, 1, 31, 0, 'tanh', True, 'eps'),
    (PT, 48, 1, 25, 0, 'tanh', True, 'eps'),
    (PT, 4112, 1, 25, 0, 'tanh', True, 'philox'),
    (PT, 24, 2, 25, 0, 'tanh', False, 'eps'),
    (PT, 48, 1, 2, 0, 'linear', False, 'philox'),
    (PT, 16, 1, 5, 0, 'linear', True, 'eps'),
    (PT, 48, 1, 25, 3, 'tanh', True, 'eps'),
    (PT, 24, 2, 31, 3, 'tanh', False, 'eps'),
    (PT, 16, 1, 2, 10, 'linear', True, 'philox'),
    (PD, 16, 1, 10, 0, 'linear', True, 'eps'),
    (PD, 48, 1, 10, 0, 'linear', False, 'philox'),
    (DP.ENV_ID, 16, 1, 10, 0, 'linear', False, None),
    (DP.ENV_ID, 48, 1, 10, 0, 'linear', True, None),
]
PHILOX_SEED, PHILOX_CTR = 0x1234567 + (5 << 32), 77
IDS = ['%s-%dx%d-n%d-K%d-%s-%s-%s' % (c[0][:8], c[1], c[2], c[3], c[4], c[5], 'packed' if c[6] else 'strided', c[7]) for c in CASES]


@functools.lru_cache(maxsize=None)
def make_case(case):
    """(computed once per case and shared by the engines; nothing in it is written to later) a random policy, start observations from
    the env's law, the model noise, and the restated rollout's autograd in float32 and float64"""
    env, rows, M, n, K, act, packed, noise = case
    rng = np.random.Generator(np.random.PCG64(7000 + CASES.index(case)))
    kw = dict(policy_out_act=act) if env == PT else {}
    ocfg = A.make_cfg(env, K, n=n, M=M, **kw)
    wp = mlp_weights_flat(rng, ocfg.obs_dim, 2 * ocfg.act_dim)
    if env == PT:
        obs = reset_law_obs(rng, rows)
        if K:       # look-ahead entries of a start observation: near delta_y, not equal to it
            obs = np.concatenate([obs, obs[:, 3:4] + 0.3 * rng.standard_normal((rows, K)).astype(np.float32)], 1).astype(np.float32)
    elif env == PD:
        obs = (rng.standard_normal((rows, 4)) * np.array([0.5, 0.1, 0.5, 0.5])).astype(np.float32)
    else:
        obs = DP.start_obs(rng, rows)
    eps = {'eps': lambda: rng.standard_normal((n, rows * M)).astype(np.float32),
           'philox': lambda: O.model_noise_philox(n, rows * M, PHILOX_SEED, PHILOX_CTR), None: lambda: None}[noise]()
    ref = {}
    for dt in (torch.float32, torch.float64):
        nets = O.Nets(ocfg, {'policy': wp}, dtype=dt)
        grads, st = A.compute_gradient(ocfg, nets, obs, eps, clip=False)
        ref[dt] = dict(grad=np.concatenate([x.ravel() for x in grads]), rsum=st['rewards_sum'])
    return dict(ocfg=ocfg, wp=wp, obs=obs, eps=eps, ref=ref)


def device_cfg(case):
    env, rows, M, n, K, act, packed, noise = case
    if env == PT:
        return ops.make_cfg(PT, obs_dim=6 + K, obs_scale=list(O.OBS_SCALE_PT) + [1.] * K, policy_out_activation=act, gamma=0.98)
    return ops.make_cfg(env, gamma=0.98)


def attach(case, cfg=None):
    """the case on the device: its own cfg and tensors, with the policy's packed weight image registered where the case asks for it"""
    env, rows, M, n, K, act, packed, noise = case
    c = dict(make_case(case))
    c['cfg'] = cfg if cfg is not None else device_cfg(case)
    c['pol'], c['o'] = dev(c['wp']), dev(c['obs'])
    if packed:
        c['wc'] = ops.WeightCache(c['pol'], [A.policy_dims(c['ocfg'])])
        c['cfg'].wcache[0] = c['wc'].pointer
    c['e'] = dev(c['eps']) if noise == 'eps' else None
    return c


def run(case, c, lo=None, hi=None, inv_b=None):
    """mpg_ampc_pg on the case (rows lo .. hi of it) -> dict of clones"""
    env, rows, M, n, K, act, packed, noise = case
    o, e = c['o'], c['e']
    if lo is not None:
        o = o[lo:hi].clone()
        if e is not None:
            e = dev(host(e).reshape(n, M, rows)[:, :, lo:hi].reshape(n, M * (hi - lo)))
    rs, rq, grad = ops.ampc_pg(c['cfg'], c['pol'], o, e, M=M, n=n, inv_b_global=inv_b, noise_seed=PHILOX_SEED, noise_ctr=PHILOX_CTR)
    return dict(ret_sum=rs.clone(), ret_sqsum=rq.clone(), grad=grad.clone())


def check_arrays(got, r32, r64, ocfg, where):
    """every array of the flat policy gradient: error against float64 at most 4 x float32 autograd's own + FLOOR, and the 1e-4 bar.
    Every figure is printed before anything is asserted."""
    o, rows = 0, []
    for shp in O.mlp_shapes(ocfg.obs_dim, 256, 2 * ocfg.act_dim):
        cnt = int(np.prod(shp))
        a, b, c = got[o:o + cnt], r32[o:o + cnt], r64[o:o + cnt]
        o += cnt
        if np.linalg.norm(c) == 0:          # (the unused log-std half of the output layer)
            assert np.linalg.norm(a) == 0, (where, shp, 'the float64 gradient is exactly zero')
            continue
        e_ref, e_got = Y.rel_l2(b, c), Y.rel_l2(a, c)
        print('   %s %-10s got %.2e  float32 autograd %.2e  allowance %.2e' % (where, shp, e_got, e_ref, 4 * e_ref + Y.FLOOR))
        rows.append((shp, e_got, e_ref))
    assert o == got.size == r32.size == r64.size
    for shp, e_got, e_ref in rows:
        assert e_got <= 4 * e_ref + Y.FLOOR and e_got <= BAR, (where, shp, 'vs float64: got %.3e, float32 autograd %.3e' % (e_got, e_ref))
    return max(r[1] / (4 * r[2] + Y.FLOOR) for r in rows)


def check_sums(ret_sum, ret_sqsum, ref, rows, M, where):
    """ret_sum / ret_sqsum against the float64 rollout.  The reference's own error: float32 autograd's rel-L2 over the per-row reward
    sums (every term of either sum has one sign, so the sum's relative error is a weighted mean of the terms': the vector's error is
    its scale, where the single float32 scalar's distance is one draw of it); the square doubles a relative error."""
    m32, m64 = [ref[dt]['rsum'].astype(np.float64).reshape(M, rows).mean(0) for dt in (torch.float32, torch.float64)]
    e_ref = Y.rel_l2(m32, m64)
    e_sum, e_sq = abs(ret_sum / m64.sum() - 1), abs(ret_sqsum / (m64 ** 2).sum() - 1)
    print('   %s ret_sum %.2e  ret_sqsum %.2e  float32 rollout (per-row sums) %.2e' % (where, e_sum, e_sq, e_ref))
    assert e_sum <= 4 * e_ref + Y.FLOOR and e_sum <= BAR, (where, 'ret_sum', e_sum, e_ref)
    assert e_sq <= 2 * (4 * e_ref + Y.FLOOR) and e_sq <= 2 * BAR, (where, 'ret_sqsum', e_sq, e_ref)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_ampc_pg_vs_float64_autograd(engine, case):
    env, rows, M, n, K, act, packed, noise = case
    c = attach(case)
    out = run(case, c)
    where = '%s (%s)' % (IDS[CASES.index(case)], engine)
    r32, r64 = c['ref'][torch.float32], c['ref'][torch.float64]
    # the loss is -mean(rewards_sum) over the M * rows trajectories: the entry point's default inv_b_global is 1 / rows
    worst = check_arrays(host(out['grad']), r32['grad'], r64['grad'], c['ocfg'], where)
    print('   %s worst error / allowance %.3f' % (where, worst))
    check_sums(float(out['ret_sum']), float(out['ret_sqsum']), c['ref'], rows, M, where)
    if packed and M == 1 and K == 0 and env != DP.ENV_ID and rows >= 48:      # (16 rows: too few terms for the order to show)
        # the tripwire of tests/test_rollout_gpu.py: THIN sums dW1 / db1 inside the sweep in another order than the weight-gradient
        # launch, so first-layer arrays bit-equal to the uncached launch's mean the launch under test was not the THIN sweep
        plain = dict(c, cfg=device_cfg(case))
        first = c['ocfg'].obs_dim * 256 + 256
        assert not torch.equal(run(case, plain)['grad'][:first], out['grad'][:first]), 'the launch under test did not reach the THIN reverse sweep'


# ---- 3: properties ---------------------------------------------------------------------------------------------------------------
BASE = CASES[3]          # path tracking 48 x 1, n = 25, packed


@pytest.mark.parametrize('case', [CASES[3], CASES[5], CASES[8], CASES[12]], ids=[IDS[i] for i in (3, 5, 8, 12)])
def test_no_discount_whatever_gamma_says(engine, case):
    a, b = attach(case), attach(case)
    a['cfg'].gamma, b['cfg'].gamma = 0.98, 1.0
    ra, rb = run(case, a), run(case, b)
    for k in ra:
        assert torch.equal(bits(ra[k]), bits(rb[k])), k


@pytest.mark.parametrize('case', [CASES[3], CASES[5], CASES[9]], ids=[IDS[i] for i in (3, 5, 9)])
def test_equals_the_critic_path_at_a_zero_critic(engine, case):
    """mpg_rollout_pg(all_steps_param_grad = 1, select = [n], w = [1]) at gamma = 1 with an all-zero Q1: the critic adds exact zeros.
    The two paths run the same sweeps; they may differ by the order of a sum, so the bar is the yardstick's allowance for a reference
    without an error of its own - FLOOR (1e-6 relative) - per parameter array and on ret_sum."""
    env, rows, M, n, K, act, packed, noise = case
    c = attach(case)
    c['cfg'].gamma = 1.0
    mine = run(case, c)
    q1 = torch.zeros(ops.q_size(c['cfg']), device=DEV)
    rs, rq, grad = ops.rollout_pg(c['cfg'], c['pol'], q1, c['o'], c['e'], [n], [1.0], M=M, all_steps_param_grad=True, n=n,
                                  noise_seed=PHILOX_SEED, noise_ctr=PHILOX_CTR)
    o = 0
    got, ref = host(mine['grad']), host(grad)
    for shp in O.mlp_shapes(c['ocfg'].obs_dim, 256, 2 * c['ocfg'].act_dim):
        cnt = int(np.prod(shp))
        if np.linalg.norm(ref[o:o + cnt]) > 0:
            e = Y.rel_l2(got[o:o + cnt], ref[o:o + cnt])
            print('   %s %s: %.2e' % (IDS[CASES.index(case)], shp, e))
            assert e <= Y.FLOOR, (shp, e)
        else:
            assert not got[o:o + cnt].any(), shp
        o += cnt
    assert abs(float(mine['ret_sum']) / float(rs) - 1) <= Y.FLOOR and abs(float(mine['ret_sqsum']) / float(rq) - 1) <= 2 * Y.FLOOR


def test_refusals_write_nothing(engine):
    """rows * M = 24, n = 0 and n = 32 on real buffers: refused with their texts before anything is enqueued - the prefilled outputs
    do not move"""
    c = attach(BASE)
    cfg, lib = c['cfg'], L.lib()
    nbytes = lib.mpg_ampc_pg_workspace_bytes(ctypes.byref(cfg), L.c_int(48), L.c_int(1), L.c_int(31))
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=DEV)
    grad = torch.full((ops.policy_size(cfg),), 7.5, device=DEV)
    sums = torch.full((2,), -3.25, device=DEV)
    eps = dev(np.zeros((31, 48), np.float32))
    for rows, M, n, text in ((24, 1, 25, 'rows*M % 16 == 0 (got 24)'), (8, 3, 25, 'rows*M % 16 == 0 (got 24)'), (48, 1, 0, '0 < n < 32 (got 0)'),
                             (48, 1, 32, '0 < n < 32 (got 32)')):
        rc = lib.mpg_ampc_pg(ctypes.byref(cfg), L.ptr(c['pol']), L.c_int(rows), L.c_int(M), L.c_int(n), L.ptr(c['o']), L.ptr(eps), L.c_u64(1),
                             L.c_u64(0), L.c_float(1. / 48), L.ptr(sums[0:1]), L.ptr(sums[1:2]), L.ptr(grad), L.ptr(ws), L.c_size_t(ws.numel()),
                             L.stream())
        msg = lib.mpg_last_error().decode()
        assert rc == -1000 and msg.startswith('mpg_ampc_pg:') and text in msg, (rc, msg)
        with pytest.raises(L.MpgError, match='unsupported configuration'):      # the wrapper's workspace query refuses the same requests
            ops.ampc_pg(cfg, c['pol'], c['o'][:rows].contiguous(), None, M=M, n=n)
    torch.cuda.synchronize()
    assert bool((grad == 7.5).all()) and bool((sums == -3.25).all())


def test_one_hundred_launches_are_bit_identical(engine):
    c = attach(BASE)
    keep = run(BASE, c)
    assert bool(torch.isfinite(keep['grad']).all()) and float(keep['grad'].abs().max()) > 0
    for _ in range(100):
        rs, rq, grad = ops.ampc_pg(c['cfg'], c['pol'], c['o'], c['e'], M=1, n=25)
        assert torch.equal(bits(grad), bits(keep['grad'])) and torch.equal(bits(rs), bits(keep['ret_sum'])) and \
            torch.equal(bits(rq), bits(keep['ret_sqsum']))


@pytest.mark.parametrize('case', [CASES[3], CASES[5], CASES[8]], ids=[IDS[i] for i in (3, 5, 8)])
def test_two_half_batches_sum_to_the_full_batch(engine, case):
    """the scheme of tests/test_sharding_gpu.py: two unequal shards (16 + 32 of 48 rows; 8 + 16 of 24 with M = 2), each called with
    inv_b_global = 1 / B, sum to the gradient of the full batch - the sum under the same rule against float64 autograd as the
    unsharded call - and to its statistics; halving inv_b_global halves the gradient exactly and moves no bit of the statistics"""
    env, rows, M, n, K, act, packed, noise = case
    cut = rows // 3
    c = attach(case)
    whole = run(case, c, 0, rows, 1.0 / rows)
    parts = [run(case, c, 0, cut, 1.0 / rows), run(case, c, cut, rows, 1.0 / rows)]
    where = '%s = %d + %d (%s)' % (IDS[CASES.index(case)], cut, rows - cut, engine)
    r32, r64 = c['ref'][torch.float32], c['ref'][torch.float64]
    check_arrays(host(parts[0]['grad'] + parts[1]['grad']), r32['grad'], r64['grad'], c['ocfg'], 'sharded ' + where)
    check_arrays(host(whole['grad']), r32['grad'], r64['grad'], c['ocfg'], 'unsharded ' + where)
    rs = sum(float(p['ret_sum']) for p in parts)
    rq = sum(float(p['ret_sqsum']) for p in parts)
    check_sums(rs, rq, c['ref'], rows, M, 'sharded ' + where)
    for lo, hi in ((0, cut), (cut, rows)):
        u, h = run(case, c, lo, hi, 1.0 / (hi - lo)), run(case, c, lo, hi, 0.5 / (hi - lo))
        assert torch.equal(h['grad'], 0.5 * u['grad']) and float(u['grad'].abs().max()) > 0
        assert torch.equal(bits(h['ret_sum']), bits(u['ret_sum'])) and torch.equal(bits(h['ret_sqsum']), bits(u['ret_sqsum']))


def test_learner_on_two_ranks_vs_reference_golden(golden, monkeypatch, engine):
    """two 32-row shards of the 64-row fixture through the two-rank harness of tests/test_sharding_gpu.py: what rank 0 holds after the
    exchange, checked as the single-process golden test checks the full batch (clip after the reduce, B * world)"""
    from tests.test_sharding_gpu import on_two_ranks
    name = 'ampc_H256_B64.npz'
    g = golden(name)

    def make_learner():
        from mpg_amd.config import default_args
        from mpg_amd.learners import AMPCLearner
        from mpg_amd.policy import PolicyWithQs
        ln = AMPCLearner(PolicyWithQs, default_args('AMPC', replay_batch_size=32, gradient_clip_norm=float(g['clip'])))
        ln.policy_with_value.set_flat(A.fixture_weights(int(g['weights_seed']), A.make_cfg())['policy'])
        return ln

    def compute(ln, lo, hi):
        obs, z = dev(g['batch_obs'][lo:hi]), torch.zeros(hi - lo, device=DEV)
        return ln.compute_gradient([obs, torch.zeros(hi - lo, 2, device=DEV), z, obs, z], None, None, 0, eps=dev(g['eps'][:, lo:hi]))
    learner, grads = on_two_ranks(monkeypatch, make_learner, compute)
    got = torch.cat([x.reshape(-1) for x in grads]).cpu().numpy()
    where = 'two shards of %s (%s)' % (name, engine)
    worst = Y.check_gradients(got, g['grads'], g['grads_f64'], [('policy', 6, 4)], where=where, small64=g['small64'])
    print(where, 'worst error / allowance %.3f' % worst)
    st = learner.get_stats()
    for k in A.STATS:
        print('%s %-22s vs float64 %.3e (reference float32 %.3e)' % (where, k, Y.rel_l2(st[k], g[k + '_f64']), Y.rel_l2(g[k], g[k + '_f64'])))
    for k in A.STATS:
        Y.check_values(st[k], g[k], g[k + '_f64'], what='%s %s' % (where, k))


# ---- 4: the loop -----------------------------------------------------------------------------------------------------------------
SMALL = dict(interval=3, num_agent=64, batch_size=64, replay_batch_size=64, replay_starts=256, max_buffer_size=1024,
             num_rollout_list_for_policy_update=[10])


def _stack(seed=0, interval=10, **kw):
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.evaluator import Evaluator
    from mpg_amd.learners import AMPCLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    args = default_args('AMPC', seed=seed, **kw)
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    learner = AMPCLearner(PolicyWithQs, args)
    evaluator = Evaluator(PolicyWithQs, args.env_id, args)
    opt = SingleProcessOffPolicyOptimizer(worker, learner, ReplayBuffer(args, 0), evaluator, args, sampling_interval=interval)
    assert opt._fused is None                  # AMPC runs through the method-by-method path
    return opt


def _state(opt):
    pw, rb, w, ln = opt.worker.policy_with_value, opt.replay_buffer, opt.worker, opt.learner
    torch.cuda.synchronize()
    tensors = [t.clone() for t in (pw.params, pw.m, pw.v, rb.obs, rb.act, rb.rew, rb.obs2, rb.done, w.obs)]
    counters = (dict(pw.opt_steps), rb._next_idx, len(rb), rb.replay_times, w._noise_ctr, w.env._ctr, ln.counter, opt.num_sampled_steps)
    return tensors, counters


def test_every_step_runs_the_policys_adam(engine):
    """no delay_update in a policy-only stack (policy.py:125-127): the policy's Adam counter advances on iteration 0 and on iteration 1
    (an odd one: the iteration a delay_update of 2 slipping through would skip); the weights move, nothing is a Polyak target"""
    opt = _stack(seed=2, **SMALL)
    pw = opt.worker.policy_with_value
    assert pw is opt.learner.policy_with_value and pw.names == ['policy'] and pw.opt_steps == {'policy': 0}
    for it in (0, 1, 2):
        before = pw.params.clone()
        assert opt.iteration == it
        opt.step()
        assert pw.opt_steps == {'policy': it + 1}
        assert not torch.equal(before, pw.params)
        st = opt.learner.get_stats()
        assert st['iteration'] == it and np.isfinite(st['policy_loss']) and st['policy_gradient_norm'] > 0
    assert pw.check_status() == 0
    # worker and evaluator run on the one-model stack
    opt.evaluator.share_policy(pw)
    opt.evaluator.fixed_steps = 5
    _, mean = opt.evaluator.run_n_episodes_parallel()
    assert np.isfinite(mean['episode_return'])
    assert len(opt.worker.get_weights()) == 1


def test_loop_is_reproducible_and_resumes_bit_identically(tmp_path, engine):
    """20 iterations of SingleProcessOffPolicyOptimizer with AMPCLearner: every parameter finite; a second run from the same seed is
    bit-identical; a checkpoint written at iteration 8 and loaded into a fresh stack built with ANOTHER seed, run for iterations
    8 .. 19, ends with parameters, Adam moments, ring and counters bit-identical to the uninterrupted run"""
    from mpg_amd.checkpoint import load_checkpoint, save_checkpoint
    a = _stack(seed=5, **SMALL)
    for _ in range(8):
        a.step()
    path = save_checkpoint(str(tmp_path / 'ckpt.npz'), a)
    for _ in range(12):
        a.step()
    ta, ca = _state(a)
    assert all(bool(torch.isfinite(t).all()) for t in ta[:3])
    assert ca[0] == {'policy': 20}
    b = _stack(seed=5, **SMALL)
    for _ in range(20):
        b.step()
    tb, cb = _state(b)
    assert ca == cb, (ca, cb)
    for i, (x, y) in enumerate(zip(ta, tb)):
        assert torch.equal(x, y), i
    c = _stack(seed=99, **SMALL)                # different seed: every stream must come from the file
    meta = load_checkpoint(path, c)
    assert meta['optimizer']['iteration'] == 8 and c.iteration == 8 and meta['learner_cls'] == 'AMPCLearner' and meta['names'] == ['policy']
    for _ in range(12):
        c.step()
    tc, cc = _state(c)
    assert ca == cc, (ca, cc)
    for i, (x, y) in enumerate(zip(ta, tc)):
        assert torch.equal(x, y), i
