"""AMPC without a GPU: the torch-CPU restatement of AMPCLearner.compute_gradient (tests/ampc_oracle.py) against the fixtures of the
unmodified reference (tests/golden/make_golden_ampc.py), float32 and float64, by the rule of tests/yardstick.py with the allowance the
NADP fixtures get (4 x the reference's own float32 error + 1e-6, and the 1e-4 bar); default_args('AMPC') against the recorded parser."""
import json
import os

import numpy as np
import pytest
import torch

from tests import ampc_oracle as A
from tests import yardstick as Y

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = sorted(A.FIXTURES)


@pytest.mark.parametrize('name', CASES)
def test_restated_ampc_reproduces_the_reference(golden, name):
    g = golden(name)
    for dt, tag in ((torch.float32, ''), (torch.float64, '_f64')):
        cfg, nets, obs, eps = A.fixture_case(g, name, dt)
        grads, st = A.compute_gradient(cfg, nets, obs, eps)
        got = np.concatenate([x.ravel() for x in grads])
        where = '%s %s' % (name, 'float32' if tag == '' else 'float64')
        for k in A.STATS:
            print('%s %-22s vs float64 %.3e (reference float32 %.3e)' % (where, k, Y.rel_l2(st[k], g[k + '_f64']), Y.rel_l2(g[k], g[k + '_f64'])))
        # (the float64 restatement is judged by the same rule: what a float32 implementation has to meet, it meets with room)
        worst = Y.check_gradients(got, g['grads'], g['grads_f64'], [('policy',) + A.policy_dims(cfg)], where=where, small64=g['small64'])
        print(where, 'gradient: worst error / allowance %.3f' % worst)
        for k in A.STATS:
            Y.check_values(st[k], g[k], g[k + '_f64'], what='%s %s' % (where, k))


def test_the_fixtures_are_the_three_cases_of_the_issue_and_one_exercises_the_clip(golden):
    shape = {}
    for name in CASES:
        assert os.path.getsize(os.path.join(GOLDEN, name)) <= 1 << 20, name
        g = golden(name)
        for k in ('grads', 'policy_loss', 'policy_gradient_norm'):
            assert k in g and k + '_f64' in g, (name, k)
        shape[name] = (g['batch_obs'].shape, int(g['n']), int(g['M']), g['eps'].shape if 'eps' in g else None)
    assert shape['ampc_H256_B64.npz'] == ((64, 6), 25, 1, (25, 64))
    assert shape['ampc_H256_B64_K3_M2.npz'] == ((32, 9), 10, 2, (10, 64))
    assert shape['ampc_dp_H256_B64_n10.npz'] == ((64, 11), 10, 1, None)          # the model draws no noise
    # policy_gradient_norm is the UN-clipped norm (tf.clip_by_global_norm's second result): above the clip in at least one case ...
    over = [n for n in CASES if float(golden(n)['policy_gradient_norm']) > float(golden(n)['clip'])]
    assert over, 'no fixture exercises the clip'
    for n in over:      # ... and there the recorded gradient is the clipped one
        g = golden(n)
        assert abs(np.linalg.norm(g['grads'].astype(np.float64)) - float(g['clip'])) <= 1e-5 * float(g['clip']), n


def test_the_rollout_is_not_discounted(golden):
    """no gamma in the rollout (ampc.py:73-87): the restated loss does not move with cfg.gamma, and it differs from the discounted sum
    by far more than the fixture's tolerance - a gamma slipping into the sum cannot hide"""
    name = 'ampc_H256_B64.npz'
    g = golden(name)
    cfg, nets, obs, eps = A.fixture_case(g, name, torch.float64)
    _, st = A.compute_gradient(cfg, nets, obs, eps)
    cfg.gamma = 0.98
    _, st98 = A.compute_gradient(cfg, nets, obs, eps)
    assert float(st['policy_loss']) == float(st98['policy_loss'])
    from oracle import mpg_oracle as O
    o = torch.as_tensor(obs).double()
    model = A.make_model(cfg)
    model.reset(o)
    disc = torch.zeros(64, dtype=torch.float64)
    with torch.no_grad():
        for t in range(cfg.n):
            o, rew = model.rollout_out(nets.compute_action(O.process_obses(cfg, o)), torch.as_tensor(eps[t]).double())
            disc = disc + 0.98 ** t * O.process_rewards(cfg, rew)
    assert abs(float(-disc.mean()) - float(g['policy_loss_f64'])) > 1e-2 * abs(float(g['policy_loss_f64']))


# optimizer_type: the parser's is the Ray optimizer ('OffPolicyAsync'); this project has the single-process one only, for every learner
# obs_dim / act_dim: None in the parser, filled in from the env by the train script (train_script.py:794-811)
NOT_COMPARED = ('optimizer_type', 'obs_dim', 'act_dim')


def test_default_args_equal_the_reference_parser():
    from mpg_amd.config import default_args
    with open(os.path.join(GOLDEN, 'ampc_parser_defaults.json')) as fh:
        ref = json.load(fh)
    ours = vars(default_args('AMPC'))
    assert ours['alg_name'] == 'AMPC' and ours['env_id'] == 'PathTracking-v0'
    both = sorted(k for k in ref if k in ours and k not in NOT_COMPARED)
    for k in ('policy_only', 'double_Q', 'target', 'tau', 'delay_update', 'alpha', 'gamma', 'M', 'num_rollout_list_for_policy_update',
              'gradient_clip_norm', 'explore_sigma', 'buffer_type', 'replay_batch_size'):
        assert k in both, k
    wrong = {k: (ours[k], ref[k]) for k in both if ours[k] != ref[k]}
    assert not wrong, wrong
    assert ours['policy_only'] is True and ours['target'] is False and ours['tau'] is None and ours['delay_update'] is None
    assert ours['gamma'] == 1.0 and ours['num_rollout_list_for_policy_update'] == [25] and ours['explore_sigma'] is None
    assert (ours['obs_dim'], ours['act_dim']) == (6, 2)
    k3 = vars(default_args('AMPC', num_future_data=3))
    assert k3['obs_dim'] == 9 and k3['obs_scale'] == ref['obs_scale'] + [1.] * 3          # train_script.py:147
