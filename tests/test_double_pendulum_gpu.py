"""InvertedDoublePendulum-v2 on the device: NADP on the model and the rollout entry points, both engines, against the fixtures of the
unmodified reference (tests/golden/make_golden_dp.py) and the float64 restatement (tests/dp_oracle.py) under the project's rule
(tests/yardstick.py: error against float64 at most 4 x the reference's own float32 error + 1e-6, and at most 1e-4)."""
import os

import numpy as np
import pytest
import torch

from tests import dp_oracle as DP
from tests import yardstick as Y

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NETS = [('Q1', 12, 1), ('policy', 11, 2)]
STATS = ('q_loss', 'policy_loss', 'value_mean', 'q_gradient_norm', 'policy_gradient_norm')


@pytest.fixture(params=['split', 'f32'])
def engine(request):
    """both builds of the library (mpg_amd/_lib.py ENGINES): the split-fp16 product and the exact-fp32 engine"""
    from mpg_amd import _lib as L
    with L.engine(request.param):
        yield request.param


def dev(x, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dt).to(DEV)


def _learner(B, n=25):
    from mpg_amd.config import default_args
    from mpg_amd.learners import NADPLearner
    from mpg_amd.policy import PolicyWithQs
    args = default_args('NADP', env_id=DP.ENV_ID, replay_batch_size=B, num_rollout_list_for_policy_update=[n],
                        num_rollout_list_for_q_estimation=[n])
    return NADPLearner(PolicyWithQs, args)


def _set(learner, w, target_scale=None):
    pw = learner.policy_with_value
    flat = np.concatenate([w[n] for n in pw.names]).astype(np.float32)
    pw.set_flat(flat, (flat * np.float32(target_scale)).astype(np.float32) if target_scale is not None else flat.copy())
    return pw


def _batch(obs, act):
    B = obs.shape[0]
    return [dev(obs), dev(act), torch.zeros(B, device=DEV), dev(obs), torch.zeros(B, device=DEV)]


def _restated(n, w, target_scale, obs, act, dtype, clip=True):
    cfg = DP.make_cfg(n)
    nets = DP.O.Nets(cfg, w, target_scale=target_scale, dtype=dtype)
    grads, st = DP.nadp_compute_gradient(cfg, nets, [obs, act], clip=clip)
    return np.concatenate([x.ravel() for x in grads]), st


@pytest.mark.parametrize('n', [25, 10])
def test_nadp_gradient_vs_reference(engine, n):
    """NADPLearner.compute_gradient on the reference's fixture, horizon 25 (the pendulum falls: |theta| reaches 7) and horizon 10
    (|theta| < 1.1).  The whole rule is asserted for both engines at both horizons."""
    inp, g = DP.load_case(GOLDEN, 256, n)
    learner = _learner(64, n)
    pw = _set(learner, {'Q1': inp['w_Q1'], 'policy': inp['w_policy']}, inp['target_scale'])
    learner.compute_gradient(_batch(inp['batch_obs'], inp['batch_actions']), None, None, 0)
    got = learner.flat_grad.cpu().numpy()
    st = learner.get_stats()
    tg = learner.batch_data['batch_targets'].cpu().numpy()
    print('%s n=%d: Q targets rel L2 vs float64 %.3e (reference float32 %.3e)' % (engine, n, Y.rel_l2(tg, g['targets_f64']),
                                                                                Y.rel_l2(g['targets'], g['targets_f64'])))
    for k in STATS:
        print('   %-22s %.3e (reference float32 %.3e)' % (k, Y.rel_l2(st[k], g[k + '_f64']), Y.rel_l2(g[k], g[k + '_f64'])))
    lay, _ = Y.layout(NETS)
    for name, shp, o, cnt in lay:          # every figure before anything is asserted
        idx = np.arange((o + 7) // 8 * 8, o + cnt, 8)
        if idx.size >= 8:
            r64 = g['grads_f64'][idx // 8]
            e_ref, e_got = Y.rel_l2(g['grads'][idx], r64), Y.rel_l2(got[idx], r64)
            print('   %-6s %-10s vs float64 %.3e  reference float32 %.3e  error / allowance %.3f' %
                  (name, shp, e_got, e_ref, e_got / (4 * e_ref + Y.FLOOR)))
    worst = Y.check_gradients(got, g['grads'], g['grads_f64'], NETS, where='%s n=%d' % (engine, n), small64=g['small64'])
    print('%s n=%d: worst error / allowance %.3f' % (engine, n, worst))
    Y.check_values(tg, g['targets'], g['targets_f64'], what='targets')
    for k in STATS:
        Y.check_values(st[k], g[k], g[k + '_f64'], what=k)
    assert pw.check_status() == 0           # velocities reach 30 and more: with obs_scale of ones far inside the 4094 envelope


@pytest.mark.parametrize('M', [1, 2])
def test_rollout_q_estimation_vs_restatement(engine, M):
    from mpg_amd import ops
    inp, _ = DP.load_case(GOLDEN, 256, 25)
    learner = _learner(64)
    pw = _set(learner, {'Q1': inp['w_Q1'], 'policy': inp['w_policy']}, inp['target_scale'])
    sel = [0, 10, 25]
    y = ops.rollout_q_estimation(pw.cfg, pw.net('policy'), pw.net('Q1', True), dev(inp['batch_obs']), dev(inp['batch_actions']), None,
                                 sel, M=M).cpu().numpy()
    ref = {}
    for dt in (torch.float32, torch.float64):
        cfg = DP.make_cfg(25)
        nets = DP.nets_of(cfg, inp, dt)
        obs, act = [torch.as_tensor(inp[k]).to(dt) for k in ('batch_obs', 'batch_actions')]
        ref[dt] = DP.rollout_q_estimation(cfg, nets, obs, act, sel, M=M)[0].numpy()
    for k in range(3):
        sl = slice(k * 64, (k + 1) * 64)
        print('%s M=%d slice %d: vs float64 %.3e (restated float32 %.3e)' % (engine, M, sel[k], Y.rel_l2(y[sl], ref[torch.float64][sl]),
                                                                          Y.rel_l2(ref[torch.float32][sl], ref[torch.float64][sl])))
    for k in range(3):
        sl = slice(k * 64, (k + 1) * 64)
        Y.check_values(y[sl], ref[torch.float32][sl], ref[torch.float64][sl], what='slice %d' % sel[k])


def test_start_observation_entries_reach_the_first_evaluation_only(engine):
    """entries 8..10 (the env's constraint forces) of a START observation are network inputs; the state ignores them and every
    model observation carries zeros"""
    from mpg_amd import ops
    inp, _ = DP.load_case(GOLDEN, 256, 25)
    learner = _learner(64)
    pw = _set(learner, {'Q1': inp['w_Q1'], 'policy': inp['w_policy']}, inp['target_scale'])
    obs2 = inp['batch_obs'].copy()
    obs2[:, 8:] = -obs2[:, 8:] + 0.05
    act = dev(inp['batch_actions'])
    ys = [ops.rollout_q_estimation(pw.cfg, pw.net('policy'), pw.net('Q1', True), dev(o), act, None, [0, 10, 25]).cpu().numpy()
          for o in (inp['batch_obs'], obs2)]
    assert (ys[0][:64] != ys[1][:64]).all()                       # part of the first critic input
    assert np.array_equal(ys[0][64:], ys[1][64:])                 # slices 10 and 25: bit-identical
    gs = []
    for o in (inp['batch_obs'], obs2):
        learner.compute_gradient(_batch(o, inp['batch_actions']), None, None, 0)
        gs.append(learner.flat_grad.clone())
    assert not torch.equal(gs[0], gs[1]) and Y.rel_l2(gs[0].cpu().numpy(), gs[1].cpu().numpy()) > 1e-3


N_ROWS = 10        # horizon of the 50-row case (see its docstring)


def test_rows_not_a_multiple_of_16(engine):
    """50 rows (the last row group has two live trajectories): the rollout gradient in the form that accepts any row count (parameter
    gradient through the first evaluation, mpg_rollout_pg with all_steps_param_grad 0), weights (0.3, 0.7) on slices (0, N_ROWS).
    Horizon N_ROWS = 10: the rule presupposes that the reference's own float32 run is inside the 1e-4 bar, and at horizon 25 it is
    not for this loss on these rows (float32 restatement against float64 on the CPU, per array: 1.2e-4 .. 3.2e-4 at 25,
    2.4e-7 .. 2.7e-7 at 10)."""
    from mpg_amd import ops
    inp, _ = DP.load_case(GOLDEN, 256, 25)
    learner = _learner(64)
    pw = _set(learner, {'Q1': inp['w_Q1'], 'policy': inp['w_policy']}, inp['target_scale'])
    obs = inp['batch_obs'][:50]
    runs = []
    for _ in range(2):
        rs, _, grad = ops.rollout_pg(pw.cfg, pw.net('policy'), pw.net('Q1'), dev(obs), None, [0, N_ROWS], [0.3, 0.7], n=N_ROWS)
        runs.append((rs.clone(), grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    ref = {}
    for dt in (torch.float32, torch.float64):
        cfg = DP.make_cfg(N_ROWS)
        nets = DP.nets_of(cfg, inp, dt)
        red = DP.rollout_policy_update(cfg, nets, torch.as_tensor(obs).to(dt), N_ROWS, all_steps_param_grad=False)
        loss = -(0.3 * red[0] + 0.7 * red[N_ROWS])
        ref[dt] = (np.concatenate([x.numpy().ravel() for x in torch.autograd.grad(loss, nets.w['policy'])]),
                   np.array([red[0].item(), red[N_ROWS].item()]) * 50)
    worst = DP.check_arrays(runs[0][1].cpu().numpy(), ref[torch.float32][0], ref[torch.float64][0], NETS[1:], 256, engine + ' rows 50')
    print('%s rows 50: worst error / allowance %.3f' % (engine, worst))
    Y.check_values(runs[0][0].cpu().numpy(), ref[torch.float32][1], ref[torch.float64][1], what='return sums')


def test_more_row_groups_than_workgroups(engine):
    """rows = 4096 + 4800 = 556 row groups on 256 workgroups: NADP's gradient at horizon 25 against the restatement (whose own float32
    run is within 1.7e-7 of its float64 run on every array here), two launches bit-identical"""
    B = 4096 + 4800
    inp, _ = DP.load_case(GOLDEN, 256, 25)
    rng = np.random.Generator(np.random.PCG64(11))
    obs, act = DP.start_obs(rng, B), rng.uniform(-1, 1, (B, 1)).astype(np.float32)
    learner = _learner(B)
    w = {'Q1': inp['w_Q1'], 'policy': inp['w_policy']}
    _set(learner, w, inp['target_scale'])
    flats = []
    for _ in range(2):
        learner.counter = 0
        learner.compute_gradient(_batch(obs, act), None, None, 0)
        flats.append(learner.flat_grad.clone())
    assert torch.equal(flats[0], flats[1])
    r32, _ = _restated(25, w, inp['target_scale'], obs, act, torch.float32)
    r64, _ = _restated(25, w, inp['target_scale'], obs, act, torch.float64)
    worst = DP.check_arrays(flats[0].cpu().numpy(), r32, r64, NETS, 256, engine + ' rows 8896')
    print('%s rows 8896: worst error / allowance %.3f' % (engine, worst))


LOOP_ITERS, LOOP_B = 28, 64


@pytest.fixture(scope='module')
def restated_loops():
    cfg = DP.make_cfg(25)
    w0, batches = DP.loop_weights(7), DP.loop_batches(8, LOOP_ITERS, LOOP_B)
    return w0, batches, DP.nadp_loop(cfg, w0, batches, torch.float64), DP.nadp_loop(cfg, w0, batches, torch.float32)


def test_short_learner_loop(engine, restated_loops):
    """40 iterations of compute_gradient + apply_gradients on seeded batches (no worker: the env does not exist here): the device's
    parameter update (final minus initial, per network) is at most 4 x as far (+ 1e-6) from the float64 restated loop as the float32
    restated loop is, in relative L2"""
    w0, batches, w64, w32 = restated_loops
    learner = _learner(LOOP_B)
    pw = _set(learner, w0)
    for it, (obs, act) in enumerate(batches):
        learner.compute_gradient(_batch(obs, act), None, None, it)
        pw.apply_gradients(it, learner.flat_grad)
    got = pw.params.cpu().numpy()
    res = []
    for i, nm in enumerate(pw.names):
        d = got[pw.offsets[i]:pw.offsets[i + 1]] - w0[nm]
        e_got, e_ref = Y.rel_l2(d, w64[nm] - w0[nm]), Y.rel_l2(w32[nm] - w0[nm], w64[nm] - w0[nm])
        print('%s loop of %d, %-6s update vs float64 loop: device %.3e, restated float32 %.3e' % (engine, LOOP_ITERS, nm, e_got, e_ref))
        res.append((nm, e_got, e_ref))
    for nm, e_got, e_ref in res:
        assert e_ref <= 1e-4, (nm, e_ref)           # the yard-stick itself stays meaningful over this length
        assert e_got <= 4 * e_ref + 1e-6, (nm, e_got, e_ref)
    assert pw.check_status() == 0


def test_nan_and_envelope_are_reported(engine):
    from mpg_amd import ops
    from mpg_amd._lib import MpgError
    inp, _ = DP.load_case(GOLDEN, 256, 25)
    learner = _learner(64)
    pw = _set(learner, {'Q1': inp['w_Q1'], 'policy': inp['w_policy']}, inp['target_scale'])
    act = dev(inp['batch_actions'])
    for col in (1, 9):                         # an entry the state is made of, and one only the first evaluation sees
        obs = inp['batch_obs'].copy()
        obs[3, col] = np.nan
        ops.rollout_q_estimation(pw.cfg, pw.net('policy'), pw.net('Q1', True), dev(obs), act, None, [0, 25])
        assert int(pw.status.item()) & ops.STATUS_NAN, col
        with pytest.raises(MpgError, match='judge_is_nan'):
            pw.check_status()
    # |first-layer activation| beyond the split engine's envelope (4094): a cart velocity of 1e5 with obs_scale of ones
    obs = inp['batch_obs'].copy()
    obs[5, 5] = 1e5
    ops.rollout_q_estimation(pw.cfg, pw.net('policy'), pw.net('Q1', True), dev(obs), act, None, [0, 25])
    bits = int(pw.status.item())
    pw.status.zero_()
    if engine == 'split':                  # (the envelope is the split engine's; the exact-fp32 engine computes such a row correctly)
        assert bits & ops.STATUS_ACTIVATION_RANGE
