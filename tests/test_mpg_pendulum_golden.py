"""MPG on the inverted pendulum without a GPU: the torch-CPU restatement of MPGLearner.compute_gradient on InvertedPendulumConti-v0
(tests/mpg_pendulum_oracle.py: sample() row by row, the clipped n-step target, MPG-v1 and MPG-v2) against the fixtures of the unmodified
reference (tests/golden/make_golden_mpg_pendulum.py), float32 and float64, by the rule of tests/yardstick.py; the generator's two
conditions on the committed files; default_args against the reference parser's defaults.

The env on BOTH sides is the documented closed-form stand-in oracle.InvertedPendulumContiOracle - MuJoCo is absent, and the stand-in's
parity with it is unpinned: what is pinned here is the learner on that env."""
import json
import os

import numpy as np
import pytest
import torch

from tests import mpg_pendulum_oracle as P
from tests import yardstick as Y

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
VERSIONS = ['MPG-v1', 'MPG-v2']
NOT_COMPARED = ('optimizer_type', 'obs_dim', 'act_dim')       # this project's optimizer; the parser leaves the dimensions to the env


@pytest.fixture(scope='module')
def restated(golden):
    """{(version, tag): {iteration: (flat grads, stats)}}: computed once, shared by the tests below"""
    out = {}
    for version in VERSIONS:
        g = P.load(golden, version)
        for dt, tag in ((torch.float32, ''), (torch.float64, '_f64')):
            cfg, nets = P.fixture_nets(g, version, dt)
            out[version, tag] = {}
            for it in P.ITERATIONS:
                grads, st = P.compute_gradient(cfg, nets, P.fixture_batch(g), g['eps'], it, version)
                out[version, tag][it] = (np.concatenate([x.ravel() for x in grads]), st)
    return out


@pytest.mark.parametrize('version', VERSIONS)
def test_restated_learner_reproduces_the_reference(golden, restated, version):
    g = P.load(golden, version)
    for tag in ('', '_f64'):
        for it in P.ITERATIONS:
            got, st = restated[version, tag][it]
            where = '%s pendulum it %d %s' % (version, it, 'float32' if tag == '' else 'float64')
            # (the float64 restatement is judged by the same rule: what a float32 implementation has to meet, it meets with room)
            worst = Y.check_gradients(got, P.flat_grads(g, it), g['it%d_grads_f64' % it], P.net_list(version), where=where,
                                      small64=g['it%d_small64' % it])
            print(where, 'worst error / allowance %.3f' % worst)
            Y.check_values(st['targets'], g['targets'], g['targets_f64'], what='targets ' + where)
            for k in P.STATS:
                if 'it%d_%s' % (it, k) in g:
                    ref = float(g['it%d_%s%s' % (it, k, tag)])
                    assert abs(float(st[k]) - ref) <= 1e-5 * abs(ref), (where, k, float(st[k]), ref)
            np.testing.assert_allclose(st['w_list'], g['it%d_w_list%s' % (it, tag)], rtol=1e-5)


def test_restated_sampler_and_bootstrap_values_reproduce_the_reference(golden, restated):
    """MPG-v1: sample()'s rewards and last observations and the UNclipped bootstrap values, both precisions"""
    g = P.load(golden, 'MPG-v1')
    for tag in ('', '_f64'):
        st = restated['MPG-v1', tag][P.ITERATIONS[0]][1]
        Y.check_values(st['all_rewards'], g['all_rewards'], g['all_rewards_f64'], what='all_rewards' + tag)
        Y.check_values(st['last_obs'], g['last_obs'], g['last_obs_f64'], what='last_obs' + tag)
        Y.check_values(st['q_boot'], g['q_boot'], g['q_boot_f64'], what='q_boot' + tag)


def test_the_generators_conditions_hold_on_the_committed_files(golden):
    g = P.load(golden, 'MPG-v1')
    # clip coverage: all three regimes of the clip are met by at least 8 of the 64 rows
    for tag in ('', '_f64'):
        q = g['q_boot' + tag]
        assert q.shape == (64,)
        assert (q < P.Q_LO).sum() >= 8 and ((q >= P.Q_LO) & (q <= P.Q_HI)).sum() >= 8 and (q > P.Q_HI).sum() >= 8, q
    # amplification: the reference's own float32 error leaves the yard-stick room (a quarter of the 1e-4 bar)
    for k in ('targets', 'all_rewards'):
        assert Y.rel_l2(g[k], g[k + '_f64']) <= 0.25e-4, (k, Y.rel_l2(g[k], g[k + '_f64']))
    assert Y.rel_l2(P.load(golden, 'MPG-v2')['targets'], P.load(golden, 'MPG-v2')['targets_f64']) <= 0.25e-4
    # start states from what the replay holds, some replay actions beyond the control clamp
    assert (np.abs(g['batch_obs'][:, 0]) < 2).all() and (np.abs(g['batch_obs'][:, 1]) <= 0.2).all()
    assert (np.abs(g['batch_actions']) > 3).any()
    # the rule-based weights differ between the two iterations under total_ite 4000
    a, b = (g['it%d_w_list' % it] for it in P.ITERATIONS)
    assert a[1] > 0.99 and b[0] > 0.9, (a, b)
    # the targets are the clipped ones: sum_t gamma^t r_t + gamma^n clip(q_boot)
    gam = np.float64(np.float32(0.98))
    disc = (gam ** np.arange(25))[:, None]
    y = (disc * g['all_rewards_f64'].astype(np.float64)).sum(0) + gam ** 25 * np.clip(g['q_boot_f64'].astype(np.float64), P.Q_LO, P.Q_HI)
    assert Y.rel_l2(y, g['targets_f64']) <= 1e-6
    unclipped = (disc * g['all_rewards_f64'].astype(np.float64)).sum(0) + gam ** 25 * g['q_boot_f64'].astype(np.float64)
    assert Y.rel_l2(unclipped, g['targets_f64']) > 1e-3            # (what mpg_nstep_targets, without the clip, would give)


@pytest.mark.parametrize('version', VERSIONS)
def test_fixture_files_fit_the_size_limit_and_regenerate_their_weights(golden, version):
    name = 'mpg_%s_pendulum_H256_B64.npz' % version[-2:]
    files = [name] + ([name[:-4] + '_it%d.npz' % P.ITERATIONS[1]] if int(golden(name)['split']) else [])
    for f in files:
        assert os.path.getsize(os.path.join(GOLDEN, f)) <= 1 << 20, f
    g = P.load(golden, version)
    assert 'w_policy' not in g and 'weights_seed' in g                 # lean: a seed instead of the weights
    w = P.fixture_weights(int(g['weights_seed']), version)
    other = P.fixture_weights(int(g['weights_seed']) + 1, version)
    assert not np.array_equal(w['Q1'], other['Q1'])
    assert g['q_grads'].size == 67585 * len(P.names_of(version)) and g['it100_policy_grads'].size == 67586
    assert (float(g['q_scale']), float(g['q_shift'])) == ((12.0, -0.25) if version == 'MPG-v1' else (1.0, 0.0))


@pytest.mark.parametrize('version', VERSIONS)
def test_default_args_equal_the_reference_parser(version):
    from mpg_amd.config import default_args
    with open(os.path.join(GOLDEN, 'mpg_mujoco_parser_defaults.json')) as fh:
        ref = json.load(fh)[version]
    ours = vars(default_args(version, env_id=P.PEND))
    assert ours['alg_name'] == 'MPG' and ours['env_id'] == ref['env_id'] == P.PEND and ours['learner_version'] == version
    both = sorted(k for k in ref if k in ours and k not in NOT_COMPARED)
    for k in ('rule_based_bias_total_ite', 'num_batch_reuse', 'double_Q', 'delay_update', 'action_range', 'obs_scale', 'rew_scale', 'eta',
              'num_rollout_list_for_policy_update', 'sample_num_in_learner', 'replay_batch_size', 'explore_sigma', 'num_agent',
              'policy_out_activation', 'gradient_clip_norm', 'gamma', 'M'):
        assert k in both, k
    wrong = {k: (ours[k], ref[k]) for k in both if ours[k] != ref[k]}
    assert not wrong, wrong
    assert ours['rule_based_bias_total_ite'] == 4000 and (ours['obs_dim'], ours['act_dim']) == (4, 1)
    # no other (alg, env) pair moved
    assert default_args(version).rule_based_bias_total_ite == 9000
    assert default_args('NADP').rule_based_bias_total_ite == 9000 and default_args('SAC', env_id=P.PEND).rule_based_bias_total_ite == 9000
