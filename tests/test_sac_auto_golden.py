"""SAC with the learned temperature without a GPU: the torch-CPU restatement (tests/sac_auto_oracle.py) against the fixtures of the
unmodified reference (tests/golden/make_golden_sac_auto.py), float32 and float64, by the rule of tests/yardstick.py: the 18 network
gradient arrays, the temperature's gradient, the statistics, and the six-iteration loop with delay_update 2 (log_alpha moves on even
iterations only)."""
import os

import numpy as np
import pytest
import torch

from tests import dp_oracle as DP
from tests import sac_auto_oracle as A
from tests import sac_oracle as S
from tests import yardstick as Y

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = [('sac_auto_H256_B64.npz', 256, 0), ('sac_auto_H256_B64_K3.npz', 256, 3), ('sac_auto_H32_B64.npz', 32, 0)]
IDS = [c[0][:-4] for c in CASES]
LOOP = 'sac_auto_loop_H32_B64.npz'


def nets_of(K):
    return [('Q1', 8 + K, 1), ('Q2', 8 + K, 1), ('policy', 6 + K, 4)]


@pytest.mark.parametrize('name,H,K', CASES, ids=IDS)
def test_restated_learned_temperature_reproduces_the_reference(golden, name, H, K):
    g = golden(name)
    assert g['log_alpha'] == A.LOG_ALPHA0 and float(g['target_entropy']) == -2.0
    # the generator's own condition: the temperature's gradient is above the clip (1.0), so the returned one is g / |g|
    assert float(g['alpha_gradient_norm']) > S.CLIP and abs(abs(float(g['alpha_grad'])) - 1.0) < 1e-6
    for dt, tag in ((torch.float32, ''), (torch.float64, '_f64')):
        cfg, nets = S.fixture_nets(g, K, H, dt)
        grads, st = A.compute_gradient(cfg, nets, S.fixture_batch(g), g['eps_target'], g['eps_policy'], g['eps_alpha'], g['log_alpha'],
                                       float(g['target_entropy']))
        assert len(grads) == 19 and grads[18].shape == ()
        got = np.concatenate([x.ravel() for x in grads[:18]])
        where = '%s %s' % (name, 'float32' if tag == '' else 'float64')
        if H == 256:
            worst = Y.check_gradients(got, g['grads'], g['grads_f64'], nets_of(K), where=where, small64=g['small64'])
        else:
            worst = DP.check_arrays(got, g['grads'], g['grads_f64'], nets_of(K), H, where)
        print(where, 'worst error / allowance %.3f' % worst)
        Y.check_values(grads[18], g['alpha_grad'], g['alpha_grad_f64'], what='temperature gradient ' + where)
        for k in ('targets', 'logp_target', 'logp_policy', 'logp_alpha'):
            Y.check_values(st[k], g[k], g[k + '_f64'], what=k)
        for k in A.STATS:
            ref = float(g[k + tag])
            assert abs(float(st[k]) - ref) <= 1e-5 * abs(ref), (where, k, float(st[k]), ref)
        # the gradient before the clip is -(mean logp_alpha + target_entropy), and alpha_loss = log_alpha times it
        raw = -(np.asarray(g['logp_alpha' + tag], np.float64).mean() + float(g['target_entropy']))
        assert abs(float(g['alpha_gradient_norm' + tag]) - abs(raw)) <= 1e-5 * abs(raw)
        assert abs(float(g['alpha_loss' + tag]) - float(g['log_alpha']) * raw) <= 1e-5 * abs(raw)
        if 'small_alpha_grad' in g:
            # target_entropy 3.0: |g| below the clip, the gradient passes as it is
            grads, st = A.compute_gradient(cfg, nets, S.fixture_batch(g), g['eps_target'], g['eps_policy'], g['eps_alpha'], g['log_alpha'], 3.0)
            assert 0 < float(g['small_alpha_gradient_norm']) < S.CLIP
            Y.check_values(grads[18], g['small_alpha_grad'], g['small_alpha_grad_f64'], what='temperature gradient below the clip')
            Y.check_values(st['alpha_gradient_norm'], g['small_alpha_gradient_norm'], g['small_alpha_gradient_norm_f64'], what='its norm')
            Y.check_values(st['alpha_loss'], g['small_alpha_loss'], g['small_alpha_loss_f64'], what='alpha_loss')


def run_loop(g, dtype):
    cfg = S.make_cfg(0, 32)
    cfg.delay_update = int(g['delay_update'])
    w = {k: g['w_' + k] for k in ('policy', 'Q1', 'Q2')}
    t = {k: (v * np.float32(g['target_scale'])).astype(np.float32) for k, v in w.items()}
    loop = A.Loop(cfg, w, t, g['log_alpha0'], float(g['target_entropy']), dtype)
    la, ag, an = [], [], []
    for it in range(int(g['n_iter'])):
        grads, st = loop.step(it, S.fixture_batch(g), *g['eps'][it])
        la.append(loop.log_alpha[0]), ag.append(grads[18]), an.append(st['alpha_gradient_norm'])
    return loop, np.array(la), np.array(ag), np.array(an)


def test_loop_fixture_pins_the_temperatures_adam(golden):
    g = golden(LOOP)
    n = int(g['n_iter'])
    ref = g['log_alpha']
    assert n == 6 and int(g['delay_update']) == 2
    # the reference itself: log_alpha is unchanged after odd iterations and moves after even ones; its Adam has its own counter
    assert all(ref[it] == ref[it - 1] for it in range(1, n, 2)) and all(ref[it] != ref[it - 1] for it in range(2, n, 2))
    assert ref[0] != g['log_alpha0'] and list(g['opt_iterations'][-1]) == [6, 6, 3, 3]
    loop, la, ag, an = run_loop(g, torch.float32)
    assert all(la[it] == la[it - 1] for it in range(1, n, 2))
    assert loop.alpha_opt.step == 3 and loop.opt['policy'].step == 3 and loop.opt['Q1'].step == 6
    Y.check_values(la, g['log_alpha'], g['log_alpha_f64'], what='log_alpha trajectory')
    # the trajectory's MOVEMENT under the same rule (log_alpha itself is -1.6: 1e-4 of it would hide a wrong step of 8e-5)
    move = lambda x: np.asarray(x, np.float64) - float(g['log_alpha0'])
    e_ref, e_got = Y.rel_l2(move(g['log_alpha']), move(g['log_alpha_f64'])), Y.rel_l2(move(la), move(g['log_alpha_f64']))
    print('log_alpha movement: restatement %.2e, reference float32 %.2e from the float64 run' % (e_got, e_ref))
    # (floor: a float32 log_alpha in [1, 2) is stored to half an ulp, 2^-24, per entry - 1.5e-3 of one 8e-5 step)
    assert e_got <= 4.0 * e_ref + np.sqrt(n) * 2.0 ** -24 / np.linalg.norm(move(g['log_alpha_f64']))
    Y.check_values(ag, g['alpha_grad'], g['alpha_grad_f64'], what='temperature gradients')
    Y.check_values(an, g['alpha_gradient_norm'], g['alpha_gradient_norm_f64'], what='their norms')
    # the parameters at the end: the UPDATE of six iterations, each array of the flat vectors as a whole
    w0 = np.concatenate([g['w_' + k] for k in ('Q1', 'Q2', 'policy')]).astype(np.float64)
    got = np.concatenate([loop.w[k] for k in ('Q1', 'Q2', 'policy')]).astype(np.float64)
    e_ref, e_got = Y.rel_l2(g['params'] - w0, g['params_f64'] - w0), Y.rel_l2(got - w0, g['params_f64'] - w0)
    print('parameter update: restatement %.2e, reference float32 %.2e from the float64 run' % (e_got, e_ref))
    assert e_got <= 4.0 * e_ref + Y.FLOOR


def test_fixture_files_fit_the_size_limit(golden):
    for name in [c[0] for c in CASES] + [LOOP]:
        assert os.path.getsize(os.path.join(GOLDEN, name)) <= 1 << 20
    for name, H, K in CASES:
        g = golden(name)
        assert g['eps_alpha'].shape == (64, 2) and not np.array_equal(g['eps_alpha'], g['eps_policy'])
        assert ('w_policy' in g) == (H == 32) and ('small_alpha_grad' in g) == (H == 32)
    assert golden(LOOP)['eps'].shape == (6, 3, 64, 2)
