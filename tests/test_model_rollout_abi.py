"""mpg_model_step and mpg_model_rollout at the drop-in boundary, without a GPU: both libraries export them with the declared argument
types, every refusal comes back as MPG_EINVAL with a text of its own before any launch (every pointer is FAKE: a launch would fault),
env kind 2 is SERVED (the first thing refused for the double pendulum's cfg is what is wrong behind the cfg), the ops wrappers check
their arguments, and ModelEvaluator asks for start observations where there is no env - where Evaluator still raises."""
import ctypes
import re

import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops
from tests import abi_harness as H
from tests.abi_harness import ENGINES, FAKE, I, NULL, MPG_EINVAL, _with, built  # noqa: F401 (built: the module's autouse fixture)

STEP, ROLL = 'mpg_model_step', 'mpg_model_rollout'
PT_ID, PD_ID, DP_ID = 'PathTracking-v0', 'InvertedPendulumConti-v0', 'InvertedDoublePendulum-v2'


@pytest.mark.parametrize('engine', ENGINES)
def test_both_libraries_export_the_entry_points(engine):
    lib = ctypes.CDLL(L.ENGINES[engine])
    for name in (STEP, ROLL):
        assert name in L.declared_symbols()
        assert hasattr(lib, name)
        assert L.declared_return_types()[name] == 'int'
    assert lib.mpg_abi_version() == 10           # functions were added: no layout or signature changed


def _declared(name):
    src = re.sub(r'/\*.*?\*/', '', open(L.HEADER).read(), flags=re.S)
    m = re.search(r'\bint\s+%s\s*\((.*?)\)\s*;' % name, src, flags=re.S)
    assert m, name
    return [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')]


def test_declared_argument_types():
    assert _declared(STEP) == ['const mpg_cfg_t* cfg', 'int rows', 'const float* obs', 'const float* act', 'const float* eps',
                               'float* obs_next', 'float* rew', 'mpg_stream_t stream']
    assert _declared(ROLL) == ['const mpg_cfg_t* cfg', 'const float* policy_params', 'int n', 'int steps', 'const float* obs0',
                               'const float* eps', 'float* obs_traj', 'float* act_traj', 'float* rew_traj', 'float* last_obs',
                               'mpg_stream_t stream']


def _pt():
    return ops.make_cfg(PT_ID)


def _pd():
    return ops.make_cfg(PD_ID)


def _dp():
    return ops.make_cfg(DP_ID)


def _tanh_range(env_id, r):
    return lambda: ops.make_cfg(env_id, policy_out_activation='tanh', action_range=r)


# what every cfg of the three kinds can get wrong, for either entry point
CFG_REFUSALS = [
    (lambda: _with(_pt(), env_kind=3), {}, 'unknown env kind 3'),
    (lambda: _with(_dp(), env_kind=-1), {}, 'unknown env kind -1'),
    (lambda: _with(_pt(), obs_dim=5), {}, 'the path-tracking model has obs_dim 6 .. 16 (got 5)'),
    (lambda: _with(_pt(), obs_dim=17), {}, 'the path-tracking model has obs_dim 6 .. 16 (got 17)'),
    (lambda: _with(_pd(), obs_dim=6), {}, 'the pendulum model has obs_dim 4 (got 6)'),
    (lambda: _with(_dp(), obs_dim=6), {}, 'the double-pendulum model has obs_dim 11 (got 6)'),
    (lambda: _with(_dp(), obs_dim=12), {}, 'the double-pendulum model has obs_dim 11 (got 12)'),
    (lambda: _with(_pt(), act_dim=1), {}, 'the path-tracking model has act_dim 2 (got 1)'),
    (lambda: _with(_pd(), act_dim=2), {}, 'the pendulum model has act_dim 1 (got 2)'),
    (lambda: _with(_dp(), act_dim=2), {}, 'the double-pendulum model has act_dim 1 (got 2)'),
    (_tanh_range(PT_ID, 1.0), {}, 'tanh policy with an action range'),
    (_tanh_range(PD_ID, 3.0), {}, 'tanh policy with an action range'),
    (_tanh_range(DP_ID, 1.0), {}, 'tanh policy with an action range'),
]
CFGS = (_pt, _pd, _dp)

# ---- mpg_model_step ---------------------------------------------------------------------------------------------------------------
S_OK = dict(rows=5, obs=FAKE, act=FAKE, eps=FAKE, obs_next=FAKE, rew=FAKE)
S_REFUSALS = CFG_REFUSALS + [(c, dict(rows=r), 'no rows') for c in CFGS for r in (0, -3)] + \
    [(c, {k: NULL}, 'null pointer') for c in CFGS for k in ('obs', 'act', 'obs_next', 'rew')] + [
    # eps may be null: what answers is the next thing wrong
    (_dp, dict(eps=NULL, rew=NULL), 'null pointer'),
    (_tanh_range(DP_ID, 1.0), dict(eps=NULL), 'tanh policy with an action range'),
]

# ---- mpg_model_rollout ------------------------------------------------------------------------------------------------------------
R_OK = dict(policy=FAKE, n=5, steps=200, obs0=FAKE, eps=FAKE, obs_traj=FAKE, act_traj=FAKE, rew_traj=FAKE, last_obs=FAKE)
R_REFUSALS = CFG_REFUSALS + [(c, dict(n=r), 'no trajectories') for c in CFGS for r in (0, -3)] + \
    [(c, d, t) for c in CFGS for d, t in ((dict(steps=0), 'steps >= 1'), (dict(steps=-1), 'steps >= 1'), (dict(steps=1025), 'steps <= 1024'))] + \
    [(c, {k: NULL}, 'null pointer') for c in CFGS for k in ('policy', 'obs0', 'obs_traj', 'act_traj', 'rew_traj', 'last_obs')] + [
    (_dp, dict(eps=NULL, last_obs=NULL), 'null pointer'),
    (_tanh_range(DP_ID, 1.0), dict(eps=NULL), 'tanh policy with an action range'),
]


def _call_step(lib, cfg_ref, a):
    return lib.mpg_model_step(cfg_ref, I(a['rows']), a['obs'], a['act'], a['eps'], a['obs_next'], a['rew'], NULL)


def _call_roll(lib, cfg_ref, a):
    return lib.mpg_model_rollout(cfg_ref, a['policy'], I(a['n']), I(a['steps']), a['obs0'], a['eps'], a['obs_traj'], a['act_traj'],
                                 a['rew_traj'], a['last_obs'], NULL)


test_step_refusals = H.refusal_test(STEP, S_REFUSALS, S_OK, _call_step)
test_rollout_refusals = H.refusal_test(ROLL, R_REFUSALS, R_OK, _call_roll)


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('name, call, ok', [(STEP, _call_step, S_OK), (ROLL, _call_roll, R_OK)])
def test_a_null_configuration_is_refused(engine, name, call, ok):
    H.null_configuration_refused(engine, name, call, ok)


@pytest.mark.parametrize('name, at_least', [(STEP, 7), (ROLL, 9)])
def test_every_refusal_has_a_text_of_its_own(name, at_least):
    H.refusal_texts_are_unique(name, 'model_rollout.hip', at_least)


def test_every_listed_condition_is_in_the_tables():
    """the texts the source holds for an entry point are the texts the tables above provoke (null configuration: its own test)"""
    for name, table in ((STEP, S_REFUSALS), (ROLL, R_REFUSALS)):
        seen = set(t for _, _, t in table)
        for stem in ('unknown env kind', 'obs_dim', 'act_dim', 'null pointer', 'tanh policy with an action range'):
            assert any(stem in t for t in seen), (name, stem)
    assert any('no rows' in t for _, _, t in S_REFUSALS) and any('no trajectories' in t for _, _, t in R_REFUSALS)
    assert {'steps >= 1', 'steps <= 1024'} <= set(t for _, _, t in R_REFUSALS)


@pytest.mark.parametrize('engine', ENGINES)
def test_env_kind_2_is_served_where_the_env_entry_points_refuse_it(engine):
    """the double pendulum's cfg passes the cfg checks of both entry points - the refusal is the null pointer behind them - while
    mpg_eval_rollout answers the same cfg with the text of the real-env entry points, and mpg_eval_metrics keeps refusing kind 2"""
    with L.engine(engine):
        lib = L.lib()
        cfg = _dp()
        assert _call_step(lib, ctypes.byref(cfg), dict(S_OK, rew=NULL)) == MPG_EINVAL
        assert lib.mpg_last_error().decode() == STEP + ': null pointer'
        assert _call_roll(lib, ctypes.byref(cfg), dict(R_OK, last_obs=NULL)) == MPG_EINVAL
        assert lib.mpg_last_error().decode() == ROLL + ': null pointer'
        rc = lib.mpg_eval_rollout(ctypes.byref(cfg), FAKE, I(5), I(25), FAKE, FAKE, FAKE, FAKE, FAKE, NULL, NULL, NULL)
        assert rc == MPG_EINVAL and 'MuJoCo' in lib.mpg_last_error().decode()
        rc = lib.mpg_eval_metrics(I(2), I(5), I(25), I(11), FAKE, FAKE, FAKE, FAKE, FAKE, NULL)
        assert rc == MPG_EINVAL and 'no evaluation metrics' in lib.mpg_last_error().decode()


def test_a_refusal_reaches_python_as_mpg_error():
    cfg = _dp()
    with pytest.raises(L.MpgError, match=ROLL + ': steps <= 1024'):
        L.call(ROLL, ctypes.byref(cfg), FAKE, I(5), I(1025), FAKE, NULL, FAKE, FAKE, FAKE, FAKE, NULL)
    with pytest.raises(L.MpgError, match=STEP + ': no rows'):
        L.call(STEP, ctypes.byref(cfg), I(0), FAKE, FAKE, NULL, FAKE, FAKE, NULL)


# ---- the ops wrappers' own argument checks (before the library is called: host tensors never reach it) ----------------------------
def test_ops_wrappers_check_their_shapes():
    cfg = _dp()
    obs, act = torch.zeros(5, 11), torch.zeros(5, 1)
    with pytest.raises(ValueError, match=r'model_step: obs .* and act .* are not \[rows, 11\] and \[rows, 1\]'):
        ops.model_step(cfg, torch.zeros(5, 6), act)
    with pytest.raises(ValueError, match='model_step: obs'):
        ops.model_step(cfg, obs, torch.zeros(5, 2))
    with pytest.raises(ValueError, match='model_step: obs'):
        ops.model_step(cfg, obs, torch.zeros(4, 1))
    with pytest.raises(ValueError, match=r'model_step: eps has shape \(4,\)'):
        ops.model_step(cfg, obs, act, eps=torch.zeros(4))
    with pytest.raises(ValueError, match=r'model_rollout: obs0 \(5, 6\) is not \[n, 11\]'):
        ops.model_rollout(cfg, torch.zeros(10), torch.zeros(5, 6), 25)
    with pytest.raises(ValueError, match=r'model_rollout: eps has shape \(25, 4\), the model noise of this call is \(25, 5\)'):
        ops.model_rollout(cfg, torch.zeros(10), obs, 25, eps=torch.zeros(25, 4))
    with pytest.raises(ValueError, match='model_rollout: eps has shape'):
        ops.model_rollout(cfg, torch.zeros(10), obs, 25, eps=torch.zeros(5, 25))


# ---- the evaluators ---------------------------------------------------------------------------------------------------------------
class _NoPolicy(object):
    """stands for PolicyWithQs where no device exists: the evaluators build it and, in these tests, never reach it"""

    def __init__(self, **kw):
        self.kw = kw


def _args(env_id, **kw):
    from mpg_amd.config import default_args
    return default_args('NADP' if env_id == DP_ID else 'MPG-v2', env_id=env_id, **kw)


def test_model_evaluator_asks_for_start_observations_on_the_double_pendulum():
    from mpg_amd.evaluator import ModelEvaluator
    ev = ModelEvaluator(_NoPolicy, DP_ID, _args(DP_ID, fixed_steps=100), device='cpu')
    assert ev.env is None and ev.kind == 2 and ev.fixed_steps == 100
    with pytest.raises(ValueError, match='init_obs is required - there is no env for this id here .* hence no reset law'):
        ev.run_n_episodes_parallel()
    with pytest.raises(ValueError, match='gap_to_env compares with the env, and there is none'):
        ev.gap_to_env(torch.zeros(5, 11))
    assert callable(ev.set_weights) and callable(ev.share_policy) and callable(ev.run_n_episodes_parallel)
    other = _NoPolicy()
    ev.share_policy(other)
    assert ev.policy_with_value is other


@pytest.mark.parametrize('steps', [0, 1025])
def test_model_evaluator_refuses_a_step_count_the_launch_refuses(steps):
    from mpg_amd.evaluator import ModelEvaluator
    with pytest.raises(ValueError, match=r'1 \.\. 1024 steps per launch'):
        ModelEvaluator(_NoPolicy, DP_ID, _args(DP_ID, fixed_steps=steps), device='cpu')


def test_evaluator_still_raises_for_the_double_pendulum():
    from mpg_amd.evaluator import Evaluator
    with pytest.raises(ValueError, match='no device environment for .InvertedDoublePendulum-v2.'):
        Evaluator(_NoPolicy, DP_ID, _args(DP_ID), device='cpu')


def test_gap_of_two_equal_records_is_zero():
    from mpg_amd.evaluator import ModelEvaluator
    g = torch.Generator().manual_seed(3)
    rec = (torch.randn(7, 5, 6, generator=g), torch.randn(7, 5, 2, generator=g), torch.randn(7, 5, generator=g))
    gap = ModelEvaluator.gap_of_records(rec, rec)
    assert gap['obs_gap'].shape == (7, 6) and gap['rew_gap'].shape == (7,) and gap['obs_gap'].dtype == torch.float64
    assert not gap['obs_gap'].any() and not gap['rew_gap'].any() and gap['env_return'] == gap['model_return']
    shifted = (rec[0] + torch.tensor([0., 0., 0., 0.5, 0., 0.]), rec[1], rec[2] - 1.)
    gap = ModelEvaluator.gap_of_records(rec, shifted)
    assert torch.allclose(gap['obs_gap'][:, 3], torch.full((7,), 0.5, dtype=torch.float64), atol=1e-6) and not gap['obs_gap'][:, :3].any()
    assert torch.allclose(gap['rew_gap'], torch.ones(7, dtype=torch.float64), atol=1e-6)
    assert abs(gap['env_return'] - gap['model_return'] - 7.) < 1e-5
