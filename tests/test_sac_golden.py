"""SAC without a GPU: the torch-CPU restatement of SACLearner.compute_gradient (tests/sac_oracle.py) against the fixtures of the
unmodified reference (tests/golden/make_golden_sac.py), float32 and float64, by the rule of tests/yardstick.py; and
default_args('SAC') against the reference parser's values."""
import json
import os

import numpy as np
import pytest
import torch

from tests import dp_oracle as DP
from tests import sac_oracle as S
from tests import yardstick as Y

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = [('sac_H256_B64.npz', 256, 0), ('sac_H256_B64_K3.npz', 256, 3), ('sac_H32_B64.npz', 32, 0)]
IDS = [c[0][:-4] for c in CASES]


def nets_of(K):
    return [('Q1', 8 + K, 1), ('Q2', 8 + K, 1), ('policy', 6 + K, 4)]


@pytest.mark.parametrize('name,H,K', CASES, ids=IDS)
def test_restated_sac_reproduces_the_reference(golden, name, H, K):
    g = golden(name)
    # the generator's own conditions: the clip (1.0 in these fixtures) is exercised on both sides
    assert max(float(g['q_gradient_norm1']), float(g['q_gradient_norm2'])) > S.CLIP > float(g['policy_gradient_norm'])
    for dt, tag in ((torch.float32, ''), (torch.float64, '_f64')):
        cfg, nets = S.fixture_nets(g, K, H, dt)
        grads, st = S.compute_gradient(cfg, nets, S.fixture_batch(g), g['eps_target'], g['eps_policy'])
        got = np.concatenate([x.ravel() for x in grads])
        where = '%s %s' % (name, 'float32' if tag == '' else 'float64')
        # (the float64 restatement is judged by the same rule: what a float32 implementation has to meet, it meets with room)
        if H == 256:
            worst = Y.check_gradients(got, g['grads'], g['grads_f64'], nets_of(K), where=where, small64=g['small64'])
        else:
            worst = DP.check_arrays(got, g['grads'], g['grads_f64'], nets_of(K), H, where)
        print(where, 'worst error / allowance %.3f' % worst)
        for k in ('targets', 'logp_target', 'logp_policy'):
            Y.check_values(st[k], g[k], g[k + '_f64'], what=k)
        for k in S.STATS:
            ref = float(g[k + tag])
            assert abs(float(st[k]) - ref) <= 1e-5 * abs(ref), (where, k, float(st[k]), ref)


@pytest.mark.parametrize('name,H,K', CASES, ids=IDS)
def test_fixture_files_fit_the_size_limit_and_carry_both_precisions(golden, name, H, K):
    assert os.path.getsize(os.path.join(GOLDEN, name)) <= 1 << 20
    g = golden(name)
    for k in ('grads', 'targets', 'logp_target', 'logp_policy') + S.STATS:
        assert k in g and k + '_f64' in g, k
    for k in ('batch_obs', 'batch_actions', 'batch_rewards', 'batch_obs_tp1', 'batch_dones', 'eps_target', 'eps_policy', 'weights_seed',
              'target_scale', 'small64'):
        assert k in g, k
    assert g['batch_obs'].shape == (64, 6 + K) and g['eps_target'].shape == g['eps_policy'].shape == (64, 2)
    assert g['eps_target'].dtype == np.float32 and not np.array_equal(g['eps_target'], g['eps_policy'])
    assert ('w_policy' in g) == (H == 32)                           # the 256-unit files are lean: a seed instead of the weights


# optimizer_type: the parser's is the Ray optimizer ('OffPolicyAsync'); this project has the single-process one only, for every learner
# obs_dim / act_dim: None in the parser, filled in from the env by the train script (train_script.py:794-811)
# target_entropy: exists for alpha = 'auto' only, which is not built
NOT_COMPARED = ('optimizer_type', 'obs_dim', 'act_dim', 'target_entropy')


def test_default_args_equal_the_reference_parser():
    from mpg_amd.config import default_args
    with open(os.path.join(GOLDEN, 'sac_parser_defaults.json')) as fh:
        ref = json.load(fh)
    ours = vars(default_args('SAC'))
    assert ours['alg_name'] == 'SAC' and ours['env_id'] == 'PathTracking-v0'
    both = sorted(k for k in ref if k in ours and k not in NOT_COMPARED)
    for k in ('alpha', 'alpha_lr_schedule', 'explore_sigma', 'num_batch_reuse', 'delay_update', 'double_Q', 'deterministic_policy',
              'policy_out_activation', 'action_range', 'target', 'buffer_type', 'gradient_clip_norm'):
        assert k in both, k
    wrong = {k: (ours[k], ref[k]) for k in both if ours[k] != ref[k]}
    assert not wrong, wrong
    assert ours['alpha'] == 0.03 and ours['deterministic_policy'] is False and ours['delay_update'] == 1 and ours['explore_sigma'] is None
    assert 'target_entropy' not in ours
    k3 = vars(default_args('SAC', num_future_data=3))
    assert k3['obs_dim'] == 9 and k3['obs_scale'] == ref['obs_scale'] + [1.] * 3
