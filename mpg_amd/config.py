"""Default hyper-parameters = the reference's argparse defaults (train_scripts/train_script.py:177-306 MPG,
:57-175 AMPC, :431-549 NDPG, :551-670 TD3, :672-792 SAC; train_scripts/train_script4mujoco.py:169-293 MPG and :296-411 NADP on InvertedPendulumConti-v0), under the same names,
so `Namespace` objects are interchangeable with the reference's `args`."""
import argparse


def default_args(alg='MPG-v2', env_id=None, **overrides):
    pend = alg == 'NADP' if env_id is None else env_id == 'InvertedPendulumConti-v0'
    env_id = env_id or ('InvertedPendulumConti-v0' if pend else 'PathTracking-v0')
    d = dict(
        policy_type='PolicyWithQs', worker_type='OffPolicyWorker', buffer_type='normal', optimizer_type='SingleProcessOffPolicy',
        env_id=env_id, num_agent=8 if not pend else 1, num_future_data=0,
        alg_name=alg.split('-')[0], learner_version=alg, sample_num_in_learner=25, M=1, deriv_interval_policy=False,
        num_rollout_list_for_policy_update=[0, 25] if alg.startswith('MPG') else [25],
        num_rollout_list_for_q_estimation=[] if alg.startswith('MPG') else [25],
        eta=0.1, rule_based_bias_total_ite=9000, gamma=0.98, gradient_clip_norm=3.,
        num_batch_reuse=10 if alg in ('MPG-v1', 'NDPG') else 1,
        batch_size=512, explore_sigma=None if alg in ('NADP', 'NDPG', 'SAC', 'AMPC') else 0.1,
        max_buffer_size=500000, replay_starts=3000, replay_batch_size=256, replay_alpha=0.6, replay_beta=0.4,
        obs_dim=4 if pend else 6, act_dim=1 if pend else 2,
        value_model_cls='MLP', value_num_hidden_layers=2, value_num_hidden_units=256, value_hidden_activation='elu',
        value_lr_schedule=[8e-5, 100000, 8e-6],
        policy_model_cls='MLP', policy_num_hidden_layers=2, policy_num_hidden_units=256, policy_hidden_activation='elu',
        policy_out_activation='linear' if (pend or alg == 'SAC') else 'tanh', policy_lr_schedule=[3e-5, 100000, 3e-6],
        # SAC: the fixed temperature of built_SAC_parser; alpha='auto' learns it and needs target_entropy=... beside it (the parser adds it then)
        alpha=0.03 if alg == 'SAC' else None, alpha_lr_schedule=[8e-5, 100000, 8e-6] if alg == 'SAC' else None,
        policy_only=False, double_Q=alg in ('MPG-v2', 'TD3', 'SAC'), target=True, tau=0.005,
        delay_update=1 if alg in ('NADP', 'NDPG', 'SAC') else 2, deterministic_policy=alg != 'SAC', action_range=3. if pend else None,
        obs_ptype='scale', obs_scale=[0.001, 1 / 3, 0.1, 0.5] if pend else [1., 1., 2., 1., 2.4, 1 / 1200],
        rew_ptype='scale', rew_scale=1. if pend else 0.01, rew_shift=0.,
        policy_smoothing_sigma=0.2, policy_smoothing_clip=0.5,
        max_iter=100000, seed=0, init_seed=0)
    if env_id == 'InvertedDoublePendulum-v2':
        # the reference ships no parser for this env: the single pendulum's NADP settings with this env's dimensions, unit scales and
        # a = tanh(mean) (ops.make_cfg: this project's choice)
        d.update(num_agent=1, obs_dim=11, act_dim=1, policy_out_activation='linear', action_range=1., obs_scale=[1.] * 11, rew_scale=1.)
    if pend and alg in ('MPG-v1', 'MPG-v2'):
        # built_MPG_parser (train_script4mujoco.py:169-293): the one default that differs from train_script.py's beside the env's own
        d.update(rule_based_bias_total_ite=4000)
    if alg == 'AMPC':
        # built_AMPC_parser: the policy alone - no critic, no target (their settings are None); gamma = 1 reaches the Preprocessor only
        d.update(gamma=1., policy_only=True, double_Q=False, target=False, tau=None, delay_update=None)
    d.update(overrides)
    if not pend and d['num_future_data'] and 'obs_dim' not in overrides:       # train_script.py:146-147, 794-811
        d['obs_dim'] = 6 + d['num_future_data']
        if 'obs_scale' not in overrides:
            d['obs_scale'] = d['obs_scale'] + [1.] * d['num_future_data']
    return argparse.Namespace(**d)
