"""n-step DPG without a GPU: the torch-CPU restatement of NDPGLearner.compute_gradient (tests/ndpg_oracle.py) against the fixtures of
the unmodified reference (tests/golden/make_golden_ndpg.py), float32 and float64, by the rule of tests/yardstick.py."""
import os

import numpy as np
import pytest
import torch

from tests import dp_oracle as DP
from tests import ndpg_oracle as N
from tests import yardstick as Y

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = [('ndpg_H256_B64.npz', 256, 0), ('ndpg_H256_B64_K3.npz', 256, 3), ('ndpg_H32_B64.npz', 32, 0)]
IDS = [c[0][:-4] for c in CASES]


def nets_of(K):
    return [('Q1', 8 + K, 1), ('policy', 6 + K, 4)]


@pytest.mark.parametrize('name,H,K', CASES, ids=IDS)
def test_restated_ndpg_reproduces_the_reference(golden, name, H, K):
    g = golden(name)
    assert float(g['q_gradient_norm']) > 3.0                       # the generator's own condition: the clip is exercised
    for dt, tag in ((torch.float32, ''), (torch.float64, '_f64')):
        cfg, nets = N.fixture_nets(g, K, H, dt)
        grads, st = N.compute_gradient(cfg, nets, N.fixture_batch(g))
        got = np.concatenate([x.ravel() for x in grads])
        where = '%s %s' % (name, 'float32' if tag == '' else 'float64')
        # (the float64 restatement is judged by the same rule: what a float32 implementation has to meet, it meets with room)
        if H == 256:
            worst = Y.check_gradients(got, g['grads'], g['grads_f64'], nets_of(K), where=where, small64=g['small64'])
        else:
            worst = DP.check_arrays(got, g['grads'], g['grads_f64'], nets_of(K), H, where)
        print(where, 'worst error / allowance %.3f' % worst)
        Y.check_values(st['targets'], g['targets'], g['targets_f64'], what='targets')
        for k in N.STATS:
            ref = float(g[k + tag])
            assert abs(float(st[k]) - ref) <= 1e-5 * abs(ref), (where, k, float(st[k]), ref)


@pytest.mark.parametrize('name,H,K', CASES, ids=IDS)
def test_fixture_files_fit_the_size_limit_and_carry_both_precisions(golden, name, H, K):
    assert os.path.getsize(os.path.join(GOLDEN, name)) <= 1 << 20
    g = golden(name)
    for k in ('grads', 'targets') + N.STATS:
        assert k in g and k + '_f64' in g, k
    for k in ('batch_obs', 'batch_actions', 'batch_rewards', 'batch_obs_tp1', 'batch_dones', 'td_error', 'nstep_all_rewards',
              'nstep_last_obs', 'weights_seed', 'target_scale', 'small64'):
        assert k in g, k
    assert g['batch_obs'].shape == (64, 6 + K) and g['nstep_all_rewards'].shape == (25, 64) and g['nstep_last_obs'].shape == (64, 6 + K)
    assert ('w_policy' in g) == (H == 32)                           # the 256-unit files are lean: a seed instead of the weights


@pytest.mark.parametrize('name,H,K', CASES[:2], ids=IDS[:2])
def test_regenerated_weights_reproduce_the_recorded_float32_result(golden, name, H, K):
    """the lean files store `weights_seed` only: the weights it regenerates give the recorded float32 targets and critic loss to
    float32 rounding (any other weights: O(1) off), and the real-env sampler's rewards / last observation"""
    from oracle import mpg_oracle as O
    g = golden(name)
    cfg, nets = N.fixture_nets(g, K, H, torch.float32)
    _, st = N.compute_gradient(cfg, nets, N.fixture_batch(g))
    assert Y.rel_l2(st['targets'], g['targets']) <= 2e-5
    assert abs(float(st['q_loss']) - float(g['q_loss'])) <= 1e-5 * float(g['q_loss'])
    r, o = O.n_step_env_rollout(cfg, nets, g['batch_obs'], g['batch_actions'])
    # (the tolerances of tests/test_oracle_golden.py for the MPG-v1 fixture's same keys)
    np.testing.assert_allclose(r, g['nstep_all_rewards'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(o[-1], g['nstep_last_obs'], rtol=0, atol=2e-3)
    other = N.fixture_weights(int(g['weights_seed']) + 1, K, H)
    assert not np.array_equal(other['Q1'], N.fixture_weights(int(g['weights_seed']), K, H)['Q1'])
