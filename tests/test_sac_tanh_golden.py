"""SAC with an action range (the tanh-squashed Gaussian head) without a GPU: the torch-CPU restatement (tests/sac_tanh_oracle.py)
against the fixtures of the unmodified reference (tests/golden/make_golden_sac_tanh.py), float32 and float64, by the rule of
tests/yardstick.py; and default_args('SAC', env_id='InvertedPendulumConti-v0') against the reference's mujoco parser."""
import json
import os

import numpy as np
import pytest
import torch

from tests import dp_oracle as DP
from tests import sac_auto_oracle as A
from tests import sac_tanh_oracle as T
from tests import yardstick as Y

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
# (file, env, H, action range, learned temperature)
CASES = [('sac_tanh_pend_H256_B64.npz', T.PEND, 256, 3., False), ('sac_tanh_pend_auto_H256_B64.npz', T.PEND, 256, 3., True),
         ('sac_tanh_pt_H256_B64.npz', T.PT, 256, 2., False), ('sac_tanh_pend_H32_B64.npz', T.PEND, 32, 3., False)]
IDS = [c[0][:-4] for c in CASES]


def draws(g, auto):
    return dict(eps_target=g['eps_target'], eps_policy=g['eps_policy'],
                **(dict(eps_alpha=g['eps_alpha'], log_alpha=g['log_alpha'], target_entropy=float(g['target_entropy'])) if auto else {}))


@pytest.mark.parametrize('name,env,H,R,auto', CASES, ids=IDS)
def test_restated_squashed_sac_reproduces_the_reference(golden, name, env, H, R, auto):
    g = golden(name)
    assert float(g['action_range']) == R
    # the generator's own conditions: the clip (1.0 in these fixtures) is exercised on both sides
    assert max(float(g['q_gradient_norm1']), float(g['q_gradient_norm2'])) > T.CLIP > float(g['policy_gradient_norm'])
    values = ('targets', 'logp_target', 'logp_policy') + (('logp_alpha',) if auto else ())
    for dt, tag in ((torch.float32, ''), (torch.float64, '_f64')):
        cfg, nets = T.fixture_nets(g, env, 0, H, dt)
        grads, st = T.compute_gradient(cfg, nets, [g['batch_' + k] for k in ('obs', 'actions', 'rewards', 'obs_tp1', 'dones')], **draws(g, auto))
        got = np.concatenate([x.ravel() for x in grads[:18]])
        where = '%s %s' % (name, 'float32' if tag == '' else 'float64')
        if H == 256:
            worst = Y.check_gradients(got, g['grads'], g['grads_f64'], T.net_list(env), where=where, small64=g['small64'])
        else:
            worst = DP.check_arrays(got, g['grads'], g['grads_f64'], T.net_list(env), H, where)
        print(where, 'worst error / allowance %.3f' % worst)
        for k in values:
            Y.check_values(st[k], g[k], g[k + '_f64'], what=k)
        for k in (A.STATS if auto else T.STATS):
            ref = float(g[k + tag])
            assert abs(float(st[k]) - ref) <= 1e-5 * abs(ref), (where, k, float(st[k]), ref)
        if auto:
            ref = float(g['alpha_grad' + tag])
            assert abs(float(grads[18]) - ref) <= 1e-5 * abs(ref), (where, float(grads[18]), ref)


@pytest.mark.parametrize('name,env,H,R,auto', CASES, ids=IDS)
def test_fixture_files_fit_the_size_limit_and_carry_both_precisions(golden, name, env, H, R, auto):
    assert os.path.getsize(os.path.join(GOLDEN, name)) <= 1 << 20
    g = golden(name)
    od, ad = T.dims(env)
    eps = ('eps_target', 'eps_policy') + (('eps_alpha',) if auto else ())
    for k in ('grads', 'targets') + tuple('logp_' + e[4:] for e in eps) + tuple('act_' + e[4:] for e in eps) + T.STATS:
        assert k in g and k + '_f64' in g, k
    for k in ('batch_obs', 'batch_actions', 'batch_rewards', 'batch_obs_tp1', 'batch_dones', 'weights_seed', 'target_scale', 'small64',
              'action_range') + eps:
        assert k in g, k
    assert g['batch_obs'].shape == (64, od) and g['batch_actions'].shape == (64, ad)
    for e in eps:
        assert g[e].shape == (64, ad) and g[e].dtype == np.float32
        # the recorded actions are the squashed ones: inside the range, and R tanh(u) moved them off mean + sigma eps
        assert np.abs(g['act_' + e[4:]]).max() <= R
    assert not np.array_equal(g['eps_target'], g['eps_policy'])
    assert ('w_policy' in g) == (H == 32)                           # the 256-unit files are lean: a seed instead of the weights


def test_the_density_is_the_published_one_at_large_arguments():
    """the restatement's Tanh log-det against log(1 - tanh(u)^2) in float64 where that is still representable, and its float32
    evaluation against the float64 one at |u| up to 17 (the size the device's saturation test reaches)"""
    u = torch.linspace(-17., 17., 1361, dtype=torch.float64)
    ldj = T.tanh_fldj(u)
    inner = u.abs() <= 8.
    assert Y.rel_l2(ldj[inner], torch.log1p(-torch.tanh(u[inner]) ** 2)) <= 1e-9
    assert torch.isfinite(ldj).all() and Y.rel_l2(T.tanh_fldj(u.float()), ldj) <= 2e-7


# optimizer_type: the parser's is the Ray optimizer; obs_dim / act_dim: None in the parser, filled in from the env by the train script;
# target_entropy: the parser adds it with alpha = 'auto' only
NOT_COMPARED = ('optimizer_type', 'obs_dim', 'act_dim', 'target_entropy')


def test_default_args_equal_the_reference_mujoco_parser():
    from mpg_amd.config import default_args
    with open(os.path.join(GOLDEN, 'sac_mujoco_parser_defaults.json')) as fh:
        ref = json.load(fh)
    ours = vars(default_args('SAC', env_id='InvertedPendulumConti-v0'))
    assert ref['env_id'] == ours['env_id'] == 'InvertedPendulumConti-v0' and ref['alg_name'] == ours['alg_name'] == 'SAC'
    both = sorted(k for k in ref if k in ours and k not in NOT_COMPARED)
    for k in ('alpha', 'alpha_lr_schedule', 'explore_sigma', 'num_batch_reuse', 'delay_update', 'double_Q', 'deterministic_policy',
              'policy_out_activation', 'action_range', 'target', 'buffer_type', 'gradient_clip_norm', 'obs_scale', 'rew_scale', 'num_agent'):
        assert k in both, k
    wrong = {k: (ours[k], ref[k]) for k in both if ours[k] != ref[k]}
    assert not wrong, wrong
    assert ours['action_range'] == 3. and ours['policy_out_activation'] == 'linear' and ours['obs_dim'] == 4 and ours['act_dim'] == 1
    assert 'squashed_head' not in ours              # the head is on request: default_args(..., squashed_head=True)
