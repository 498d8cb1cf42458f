"""mpg_eval_rollout, mpg_eval_rollout_pendulum and mpg_eval_metrics at the drop-in boundary, without a GPU: both libraries export them
with the declared argument types, and every refusal comes back as MPG_EINVAL with a text of its own before any launch (every pointer is
FAKE: a launch would fault)."""
import ctypes
import os
import re

import pytest

from mpg_amd import _lib as L
from mpg_amd import ops
from tests import abi_harness as H
from tests.abi_harness import CSRC, ENGINES, FAKE, I, NULL, MPG_EINVAL, _with, built  # noqa: F401 (built: the module's autouse fixture)

PT, PEND, METRICS = 'mpg_eval_rollout', 'mpg_eval_rollout_pendulum', 'mpg_eval_metrics'


@pytest.mark.parametrize('engine', ENGINES)
def test_both_libraries_export_the_entry_points(engine):
    lib = ctypes.CDLL(L.ENGINES[engine])
    for name in (PT, PEND, METRICS):
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
    """the declarations of include/mpg_hip.h, argument by argument; the pendulum's is PathTracking's without done_intended_out"""
    assert _declared(PT) == ['const mpg_cfg_t* cfg', 'const float* policy_params', 'int n', 'int steps', 'float* state', 'float* obs_io',
                             'float* obs_traj', 'float* act_traj', 'float* rew_traj', 'uint8_t* done_out', 'uint8_t* done_intended_out',
                             'mpg_stream_t stream']
    assert _declared(PEND) == [a for a in _declared(PT) if a != 'uint8_t* done_intended_out']
    assert _declared(METRICS) == ['int env_kind', 'int n', 'int steps', 'int obs_dim', 'const float* obs_traj', 'const float* act_traj',
                                  'const float* rew_traj', 'double* per_episode', 'double* mean', 'mpg_stream_t stream']


def test_the_metric_counts_are_declared_once_and_mirrored():
    src = open(L.HEADER).read()
    pt = re.findall(r'#define\s+MPG_EVAL_METRICS_PATH_TRACKING\s+(\d+)', src)
    pend = re.findall(r'#define\s+MPG_EVAL_METRICS_PENDULUM\s+(\d+)', src)
    assert len(pt) == 1 and len(pend) == 1, (pt, pend)
    assert (int(pt[0]), int(pend[0])) == (8, 18) == (ops.EVAL_METRICS_PATH_TRACKING, ops.EVAL_METRICS_PENDULUM)
    assert len(ops.EVAL_METRIC_KEYS[0]) == 8 and len(ops.EVAL_METRIC_KEYS[1]) == 18
    # the kernel takes them from the header
    krn = open(os.path.join(CSRC, 'eval_kernels.hip')).read()
    assert 'MPG_EVAL_METRICS_PATH_TRACKING' in krn and 'MPG_EVAL_METRICS_PENDULUM' in krn


def test_the_metric_rows_are_the_references_key_list():
    """evaluator.py:161,180-181,202-205"""
    assert ops.EVAL_METRIC_KEYS[0] == ('episode_return', 'episode_len', 'delta_y_mse', 'delta_phi_mse', 'delta_v_mse',
                                       'stationary_rew_mean', 'steer_mse', 'acc_mse')
    assert ops.EVAL_METRIC_KEYS[1] == ('episode_return', 'episode_len', 'x_mean', 'x_var', 'theta_mean', 'theta_var', 'xdot_mean', 'xdot_var',
                                       'thetadot_mean', 'thetadot_var', 'x_mse', 'theta_mse', 'xdot_mse', 'thetadot_mse', 'x_mse_25',
                                       'theta_mse_25', 'xdot_mse_25', 'thetadot_mse_25')


def _pt():
    return ops.make_cfg('PathTracking-v0')


def _pend():
    return ops.make_cfg('InvertedPendulumConti-v0')


POINTERS = ('policy', 'state', 'obs_io', 'obs_traj', 'act_traj', 'rew_traj')
OK = dict(policy=FAKE, n=5, steps=200, state=FAKE, obs_io=FAKE, obs_traj=FAKE, act_traj=FAKE, rew_traj=FAKE, done=FAKE, done_i=FAKE)
STEPS = [(dict(steps=0), 'steps >= 1'), (dict(steps=-1), 'steps >= 1'), (dict(steps=1025), 'steps <= 1024')]

# ---- mpg_eval_rollout -----------------------------------------------------------------------------------------------------------
PT_REFUSALS = [
    # (cfg, what differs from OK, the text of the refusal)
    (lambda: ops.make_cfg('InvertedDoublePendulum-v2'), {}, 'MuJoCo'),
    (_pend, {}, 'path-tracking env only'),
    (lambda: _with(_pt(), env_kind=3), {}, 'path-tracking env only'),
    (lambda: _with(_pt(), obs_dim=5), {}, 'obs_dim 6 .. 16 only'),
    (lambda: _with(_pt(), obs_dim=17), {}, 'obs_dim 6 .. 16 only'),
    (lambda: _with(_pt(), act_dim=1), {}, 'act_dim 2 only'),
    (_pt, dict(n=0), 'no agents'),
    (_pt, dict(n=-3), 'no agents'),
] + [(_pt, d, t) for d, t in STEPS] + [(_pt, {k: NULL}, 'null pointer') for k in POINTERS] + [
    (lambda: ops.make_cfg('PathTracking-v0', policy_out_activation='tanh', action_range=1.0), {}, 'tanh policy with an action range'),
    # the done flags may be null: the refusal further down the list is what answers
    (lambda: ops.make_cfg('PathTracking-v0', policy_out_activation='tanh', action_range=1.0), dict(done=NULL, done_i=NULL),
     'tanh policy with an action range'),
    (lambda: ops.make_cfg('PathTracking-v0', policy_out_activation='tanh', action_range=1.0), dict(done_i=NULL),
     'tanh policy with an action range'),
]

# ---- mpg_eval_rollout_pendulum --------------------------------------------------------------------------------------------------
PEND_REFUSALS = [
    (lambda: ops.make_cfg('InvertedDoublePendulum-v2'), {}, 'MuJoCo'),
    (_pt, {}, 'pendulum env only'),
    (lambda: _with(_pend(), env_kind=3), {}, 'pendulum env only'),
    (lambda: _with(_pend(), obs_dim=6), {}, 'obs_dim 4 only'),
    (lambda: _with(_pend(), obs_dim=3), {}, 'obs_dim 4 only'),
    (lambda: _with(_pend(), act_dim=2), {}, 'act_dim 1 only'),
    (_pend, dict(n=0), 'no agents'),
    (_pend, dict(n=-3), 'no agents'),
] + [(_pend, d, t) for d, t in STEPS] + [(_pend, {k: NULL}, 'null pointer') for k in POINTERS] + [
    (lambda: ops.make_cfg('InvertedPendulumConti-v0', policy_out_activation='tanh', action_range=3.0), {}, 'tanh policy with an action range'),
    (lambda: ops.make_cfg('InvertedPendulumConti-v0', policy_out_activation='tanh', action_range=3.0), dict(done=NULL),
     'tanh policy with an action range'),
]


def _call(lib, name, cfg_ref, a):
    tail = (a['done'], a['done_i'], NULL) if name == PT else (a['done'], NULL)
    return getattr(lib, name)(cfg_ref, a['policy'], I(a['n']), I(a['steps']), a['state'], a['obs_io'], a['obs_traj'], a['act_traj'],
                              a['rew_traj'], *tail)


def _calls(name):
    return lambda lib, cfg_ref, a: _call(lib, name, cfg_ref, a)


test_path_tracking_refusals = H.refusal_test(PT, PT_REFUSALS, OK, _calls(PT))
test_pendulum_refusals = H.refusal_test(PEND, PEND_REFUSALS, OK, _calls(PEND))


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('name', [PT, PEND])
def test_a_null_configuration_is_refused(engine, name):
    H.null_configuration_refused(engine, name, _calls(name), OK)


@pytest.mark.parametrize('name, src', [(PT, 'env_path_tracking.hip'), (PEND, 'env_cart_pole.hip'), (METRICS, 'eval_kernels.hip')])
def test_every_refusal_has_a_text_of_its_own(name, src):
    H.refusal_texts_are_unique(name, src, 6 if name == METRICS else 10)


# ---- mpg_eval_metrics -----------------------------------------------------------------------------------------------------------
M_OK = dict(kind=0, n=5, steps=200, od=6, obs=FAKE, act=FAKE, rew=FAKE, pe=FAKE, mean=FAKE)
M_REFUSALS = [
    (dict(kind=2), 'no evaluation metrics'),
    (dict(kind=-1), 'no evaluation metrics'),
    (dict(kind=3), 'no evaluation metrics'),
    (dict(n=0), 'no episodes'),
    (dict(n=-5), 'no episodes'),
    (dict(steps=0), 'steps >= 1'),
    (dict(steps=-1), 'steps >= 1'),
    (dict(od=5), 'obs_dim 6 .. 16 on PathTracking'),
    (dict(od=17), 'obs_dim 6 .. 16 on PathTracking'),
    (dict(od=4), 'obs_dim 6 .. 16 on PathTracking'),
    (dict(kind=1, od=6), 'obs_dim 4 on the pendulum'),
    (dict(kind=1, od=3), 'obs_dim 4 on the pendulum'),
] + [({k: NULL}, 'null pointer') for k in ('obs', 'act', 'rew', 'pe', 'mean')] + [
    (dict(kind=1, od=4, mean=NULL), 'null pointer'),
]


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('case', range(len(M_REFUSALS)),
                         ids=['%02d-%s' % (i, re.sub(r'[^a-z0-9]+', '_', c[1].lower())) for i, c in enumerate(M_REFUSALS)])
def test_metrics_refusals(engine, case):
    diff, text = M_REFUSALS[case]
    with L.engine(engine):
        lib = L.lib()
        a = dict(M_OK)
        a.update(diff)
        rc = lib.mpg_eval_metrics(I(a['kind']), I(a['n']), I(a['steps']), I(a['od']), a['obs'], a['act'], a['rew'], a['pe'], a['mean'], NULL)
        msg = lib.mpg_last_error().decode()
        assert rc == MPG_EINVAL, (rc, msg)
        assert msg.startswith(METRICS + ':') and text in msg, msg


# ---- the neighbours, ops and the evaluator --------------------------------------------------------------------------------------
def test_new_names_beside_the_existing_rollouts_not_a_widening_of_them():
    """the same arguments, old entry point and new: mpg_env_rollout still refuses 32 steps where mpg_eval_rollout refuses none up to
    1024 (here: the first thing wrong behind the step count, a null trajectory), and each env's pair refuses the other env's cfg under
    its own name"""
    lib = L.lib()
    cfg = _pt()
    rc = lib.mpg_env_rollout(ctypes.byref(cfg), FAKE, I(40), I(32), FAKE, FAKE, FAKE, FAKE, NULL)
    assert rc == MPG_EINVAL and '1 <= n < 32' in lib.mpg_last_error().decode()
    rc = lib.mpg_eval_rollout(ctypes.byref(cfg), FAKE, I(40), I(32), FAKE, FAKE, NULL, FAKE, FAKE, NULL, NULL, NULL)
    assert rc == MPG_EINVAL and lib.mpg_last_error().decode() == PT + ': null pointer'
    rc = lib.mpg_env_rollout_pendulum(ctypes.byref(cfg), FAKE, I(40), I(25), FAKE, FAKE, FAKE, FAKE, NULL)
    assert rc == MPG_EINVAL and lib.mpg_last_error().decode().startswith('mpg_env_rollout_pendulum: pendulum env only')
    rc = lib.mpg_eval_rollout_pendulum(ctypes.byref(cfg), FAKE, I(40), I(25), FAKE, FAKE, FAKE, FAKE, FAKE, NULL, NULL)
    assert rc == MPG_EINVAL and lib.mpg_last_error().decode().startswith(PEND + ': pendulum env only')


def test_a_refusal_reaches_python_as_mpg_error():
    """L.call - what the ops wrappers send their arguments through - turns a refusal into MpgError with the library's text; the
    wrappers themselves take device tensors and are invoked in tests/test_eval_rollout_gpu.py::test_ops_wrappers_raise_mpg_error"""
    cfg = _pend()
    with pytest.raises(L.MpgError, match=PT + ': path-tracking env only'):
        L.call(PT, ctypes.byref(cfg), FAKE, I(5), I(200), FAKE, FAKE, FAKE, FAKE, FAKE, NULL, NULL, NULL)
    with pytest.raises(L.MpgError, match=PEND + ': steps <= 1024'):
        L.call(PEND, ctypes.byref(cfg), FAKE, I(5), I(1025), FAKE, FAKE, FAKE, FAKE, FAKE, NULL, NULL)
    with pytest.raises(L.MpgError, match=METRICS + ': steps >= 1'):
        L.call(METRICS, I(0), I(5), I(0), I(6), FAKE, FAKE, FAKE, FAKE, FAKE, NULL)
    assert callable(ops.eval_rollout) and callable(ops.eval_metrics)


def test_the_evaluator_has_both_episode_forms_and_the_launch_bound():
    """(that the flag is off unless the args ask for it is read from a built evaluator: tests/test_eval_rollout_gpu.py)"""
    from mpg_amd.evaluator import Evaluator, MAX_ONE_LAUNCH_STEPS
    assert MAX_ONE_LAUNCH_STEPS == 1024
    assert callable(Evaluator.run_n_episodes) and callable(Evaluator.run_n_episodes_parallel)
