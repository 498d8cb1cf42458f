"""The n-step DPG entry points at the drop-in boundary, without a GPU: both libraries export them, every refusal comes back as
MPG_EINVAL with its message before any launch (every pointer is FAKE: a launch would fault), the native step driver answers for
learner_version 5, and default_args('NDPG') carries the reference parser's values."""
import ctypes
import json
import os

import pytest

from mpg_amd import _lib as L
from mpg_amd import ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NULL, FAKE = ctypes.c_void_p(0), ctypes.c_void_p(0x1000)
I, F, SZ = ctypes.c_int, ctypes.c_float, ctypes.c_size_t
MPG_EINVAL = -1000
NEW = ('mpg_env_rollout', 'mpg_dpg_policy_grad', 'mpg_dpg_policy_grad_workspace_bytes')
ENGINES = sorted(L.ENGINES)


@pytest.fixture(scope='module')
def built():
    from mpg_amd import build as B
    return B.build(verbose=False)


@pytest.mark.parametrize('engine', ENGINES)
def test_both_libraries_export_the_new_entry_points(built, engine):
    assert set(NEW) <= set(L.declared_symbols())
    lib = ctypes.CDLL(L.ENGINES[engine])
    assert not [n for n in NEW if not hasattr(lib, n)]
    assert lib.mpg_abi_version() == 10           # functions and one accepted value of an int were added: no layout or signature changed


def _cfg(obs_dim=6):
    return ops.make_cfg('PathTracking-v0', obs_dim=obs_dim)


def _pendulum():
    return ops.make_cfg('InvertedPendulumConti-v0')


def _tanh_ranged():
    return ops.make_cfg('PathTracking-v0', policy_out_activation='tanh', action_range=1.0)


def _with(c, **kw):
    for k, v in kw.items():
        setattr(c, k, v)
    return c


ROLLOUT_REFUSALS = [
    # (cfg, (policy, rows, n, obs0, act0, rewards, last_obs), the text of the refusal)
    (_pendulum, (FAKE, 16, 25, FAKE, FAKE, FAKE, FAKE), 'path-tracking env only'),
    (lambda: ops.make_cfg('InvertedDoublePendulum-v2'), (FAKE, 16, 25, FAKE, FAKE, FAKE, FAKE), 'MuJoCo'),
    (lambda: _with(_cfg(), obs_dim=5), (FAKE, 16, 25, FAKE, FAKE, FAKE, FAKE), 'obs_dim 6 .. 16'),
    (lambda: _with(_cfg(), obs_dim=17), (FAKE, 16, 25, FAKE, FAKE, FAKE, FAKE), 'obs_dim 6 .. 16'),
    (lambda: _with(_cfg(), act_dim=1), (FAKE, 16, 25, FAKE, FAKE, FAKE, FAKE), 'act_dim 2 only'),
    (_cfg, (FAKE, 16, 0, FAKE, FAKE, FAKE, FAKE), '1 <= n < 32'),
    (_cfg, (FAKE, 16, 32, FAKE, FAKE, FAKE, FAKE), '1 <= n < 32'),
    (_cfg, (FAKE, 0, 25, FAKE, FAKE, FAKE, FAKE), 'no rows'),
    (_cfg, (NULL, 16, 25, FAKE, FAKE, FAKE, FAKE), 'null pointer'),
    (_cfg, (FAKE, 16, 25, NULL, FAKE, FAKE, FAKE), 'null pointer'),
    (_cfg, (FAKE, 16, 25, FAKE, NULL, FAKE, FAKE), 'null pointer'),
    (_cfg, (FAKE, 16, 25, FAKE, FAKE, NULL, FAKE), 'null pointer'),
    (_cfg, (FAKE, 16, 25, FAKE, FAKE, FAKE, NULL), 'null pointer'),
    (_tanh_ranged, (FAKE, 16, 25, FAKE, FAKE, FAKE, FAKE), 'tanh policy with an action range'),
]


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('case', range(len(ROLLOUT_REFUSALS)), ids=['%02d-%s' % (i, c[2].replace(' ', '_')) for i, c in enumerate(ROLLOUT_REFUSALS)])
def test_env_rollout_refusals(engine, case):
    make, (policy, rows, n, obs0, act0, rew, last), text = ROLLOUT_REFUSALS[case]
    with L.engine(engine):
        lib = L.lib()
        cfg = make()
        rc = lib.mpg_env_rollout(ctypes.byref(cfg), policy, I(rows), I(n), obs0, act0, rew, last, NULL)
        msg = lib.mpg_last_error().decode()
        assert rc == MPG_EINVAL, (rc, msg)
        assert msg.startswith('mpg_env_rollout:') and text in msg, msg
        with pytest.raises(L.MpgError, match='mpg_env_rollout'):
            L.call('mpg_env_rollout', ctypes.byref(cfg), policy, I(rows), I(n), obs0, act0, rew, last, NULL)


@pytest.mark.parametrize('engine', ENGINES)
def test_env_rollout_refuses_a_null_configuration(engine):
    with L.engine(engine):
        lib = L.lib()
        assert lib.mpg_env_rollout(NULL, FAKE, I(16), I(25), FAKE, FAKE, FAKE, FAKE, NULL) == MPG_EINVAL
        assert lib.mpg_last_error().decode().startswith('mpg_env_rollout:')


DPG_ARGS = dict(policy=FAKE, q1=FAKE, rows=64, obs=FAKE, q_sum=FAKE, q_sqsum=FAKE, grad=FAKE, ws=FAKE)
DPG_REFUSALS = [(k, NULL) for k in ('policy', 'q1', 'obs', 'q_sum', 'q_sqsum', 'grad', 'ws')] + [('rows', 0), ('cfg', 'tanh+range'), ('cfg', None)]


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('what,value', DPG_REFUSALS, ids=['%s-%s' % (k, 'null' if v is NULL else v) for k, v in DPG_REFUSALS])
def test_dpg_policy_grad_refusals(engine, what, value):
    with L.engine(engine):
        lib = L.lib()
        cfg = _tanh_ranged() if value == 'tanh+range' else _cfg()
        a = dict(DPG_ARGS)
        if what != 'cfg':
            a[what] = value
        ref = NULL if (what == 'cfg' and value is None) else ctypes.byref(cfg)
        rc = lib.mpg_dpg_policy_grad(ref, a['policy'], a['q1'], I(a['rows']), a['obs'], F(1.0 / 64), a['q_sum'], a['q_sqsum'], a['grad'],
                                     a['ws'], SZ(1 << 40), NULL)
        msg = lib.mpg_last_error().decode()
        assert rc == MPG_EINVAL, (rc, msg)
        assert msg.startswith('mpg_dpg_policy_grad:'), msg


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('obs_dim', [6, 9, 16])
def test_dpg_policy_grad_workspace(engine, obs_dim):
    """the query answers, is smaller than the two-critic entry point's, refuses what the entry point refuses, and a buffer one byte
    short is refused with both sizes"""
    with L.engine(engine):
        lib = L.lib()
        cfg = _cfg(obs_dim=obs_dim)
        need = lib.mpg_dpg_policy_grad_workspace_bytes(ctypes.byref(cfg), I(4096))
        assert 0 < need < lib.mpg_td3_policy_grad_workspace_bytes(ctypes.byref(cfg), I(4096))
        assert lib.mpg_dpg_policy_grad_workspace_bytes(ctypes.byref(cfg), I(0)) == 0
        tr = _tanh_ranged()
        assert lib.mpg_dpg_policy_grad_workspace_bytes(ctypes.byref(tr), I(4096)) == 0
        rc = lib.mpg_dpg_policy_grad(ctypes.byref(cfg), FAKE, FAKE, I(4096), FAKE, F(1.0 / 4096), FAKE, FAKE, FAKE, FAKE, SZ(need - 1), NULL)
        msg = lib.mpg_last_error().decode()
        assert rc == -1001 and msg.startswith('mpg_dpg_policy_grad:') and '%d < %d' % (need - 1, need) in msg, (rc, msg)


@pytest.mark.parametrize('engine', ENGINES)
def test_step_workspace_answers_for_version_5_and_refuses_6(engine):
    from mpg_amd.fused import TrainCtx
    with L.engine(engine):
        lib = L.lib()
        c = TrainCtx()
        c.cfg = _cfg()
        c.batch, c.n, c.M, c.n_select = 256, 25, 1, 1
        w0, w1 = SZ(0), SZ(0)
        c.learner_version = 5
        assert lib.mpg_step_workspace_bytes(ctypes.byref(c), ctypes.byref(w0), ctypes.byref(w1)) == 0
        assert w1.value == lib.mpg_dpg_policy_grad_workspace_bytes(ctypes.byref(c.cfg), I(256)) > 0
        assert w0.value >= max(lib.mpg_q_targets_workspace_bytes(ctypes.byref(c.cfg), I(256)),
                               lib.mpg_q_loss_grad_workspace_bytes(ctypes.byref(c.cfg), I(256))) > 0
        c.learner_version = 6
        assert lib.mpg_step_workspace_bytes(ctypes.byref(c), ctypes.byref(w0), ctypes.byref(w1)) == MPG_EINVAL
        assert 'mpg_step_workspace_bytes' in lib.mpg_last_error().decode()
        # ... and the driver itself: version 5 passes the context check as far as the buffers (all null here), 6 does not exist
        assert lib.mpg_step_begin(ctypes.byref(c), I(0), NULL) == MPG_EINVAL


# optimizer_type: the parser's is the Ray optimizer ('OffPolicyAsync'); this project has the single-process one only, for every learner
# obs_dim / act_dim: None in the parser, filled in from the env by the train script (train_script.py:794-811)
NOT_COMPARED = ('optimizer_type', 'obs_dim', 'act_dim')


def test_default_args_equal_the_reference_parser():
    from mpg_amd.config import default_args
    with open(os.path.join(GOLDEN, 'ndpg_parser_defaults.json')) as fh:
        ref = json.load(fh)
    ours = vars(default_args('NDPG'))
    assert ours['alg_name'] == 'NDPG' and ours['env_id'] == 'PathTracking-v0'
    both = sorted(k for k in ref if k in ours and k not in NOT_COMPARED)
    for k in ('explore_sigma', 'num_batch_reuse', 'delay_update', 'double_Q', 'sample_num_in_learner', 'target', 'buffer_type'):
        assert k in both
    wrong = {k: (ours[k], ref[k]) for k in both if ours[k] != ref[k]}
    assert not wrong, wrong
    assert ours['explore_sigma'] is None and ours['num_batch_reuse'] == 10 and ours['delay_update'] == 1 and ours['double_Q'] is False
    assert (ours['obs_dim'], ours['act_dim']) == (6, 2)
    k3 = vars(default_args('NDPG', num_future_data=3))
    assert k3['obs_dim'] == 9 and k3['obs_scale'] == ref['obs_scale'] + [1.] * 3          # train_script.py:521
