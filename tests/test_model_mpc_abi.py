"""mpg_model_mpc_cost_grad and mpg_model_mpc_solve at the drop-in boundary, without a GPU: both libraries export them with the declared
argument types, and every refusal comes back as MPG_EINVAL with the entry's name and a text of its own before any launch, the outputs
untouched (the buffers are HOST arrays with a pattern in them: a launch would fault, a refusal never dereferences them)."""
import ctypes
import math
import os
import re

import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops
from tests import abi_harness as H
from tests.abi_harness import ENGINES, F, I, NULL, MPG_EINVAL, _with, built  # noqa: F401 (built: the module's autouse fixture)

COST, SOLVE = 'mpg_model_mpc_cost_grad', 'mpg_model_mpc_solve'
PT_ID, PD_ID, DP_ID = 'PathTracking-v0', 'InvertedPendulumConti-v0', 'InvertedDoublePendulum-v2'
PATTERN = 0x5A
NAMES = ('obs0', 'u', 'eps', 'cost', 'grad', 'obs_traj', 'rew_traj', 'pgnorm', 'info')


def _define(name):
    v = re.findall(r'#define\s+%s\s+(\d+)' % name, open(L.HEADER).read())
    assert len(v) == 1, name
    return int(v[0])


CAPS = {k: _define('MPG_MODEL_MPC_MAX_ITERS_' + n) for k, n in ((0, 'PATH_TRACKING'), (1, 'PENDULUM'), (2, 'DOUBLE_PENDULUM'))}


class Buffers(object):
    """host arrays behind every pointer argument, filled with a pattern"""

    def __init__(self):
        self.raw = {k: (ctypes.c_ubyte * 4096)(*([PATTERN] * 4096)) for k in NAMES}

    def p(self, k):
        return ctypes.cast(self.raw[k], ctypes.c_void_p)

    def untouched(self):
        return all(bytes(v) == bytes([PATTERN]) * 4096 for v in self.raw.values())


BUF = Buffers()


@pytest.mark.parametrize('engine', ENGINES)
def test_both_libraries_export_the_entry_points(engine):
    lib = ctypes.CDLL(L.ENGINES[engine])
    for name in (COST, SOLVE):
        assert name in L.declared_symbols()
        assert hasattr(lib, name)
        assert L.declared_return_types()[name] == 'int'
    assert lib.mpg_abi_version() == 10           # functions were added: no layout or signature changed
    assert L.ABI_VERSION == 10


def _declared(name):
    src = re.sub(r'/\*.*?\*/', '', open(L.HEADER).read(), flags=re.S)
    m = re.search(r'\bint\s+%s\s*\((.*?)\)\s*;' % name, src, flags=re.S)
    assert m, name
    return [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')]


def test_declared_argument_types():
    assert _declared(COST) == ['const mpg_cfg_t* cfg', 'int rows', 'int horizon', 'const float* obs0', 'const float* u', 'const float* eps',
                               'float* cost', 'float* grad', 'float* obs_traj', 'float* rew_traj', 'mpg_stream_t stream']
    assert _declared(SOLVE) == ['const mpg_cfg_t* cfg', 'int rows', 'int horizon', 'int iters', 'float tol', 'const float* obs0',
                                'const float* eps', 'float* u_io', 'float* cost_out', 'float* pgnorm_out', 'int* info', 'mpg_stream_t stream']


def test_the_caps_are_defines_the_code_uses_and_python_mirrors():
    src = open(os.path.join(H.CSRC, 'model_mpc.hip')).read()
    for n in ('PATH_TRACKING', 'PENDULUM', 'DOUBLE_PENDULUM'):
        assert 'MPG_MODEL_MPC_MAX_ITERS_' + n in src
    assert all(1 <= c <= _define('MPG_MPC_MAX_ITERS') for c in CAPS.values())
    from mpg_amd import mpc
    assert mpc.MODEL_MAX_ITERS == CAPS
    # the solver's constants are mpg_mpc_solve's: the one loop
    assert 'mpc::solve(' in src and 'MPG_MPC_SPG_M' in src


def _pt():
    return ops.make_cfg(PT_ID)


def _pt16():
    return ops.make_cfg(PT_ID, obs_dim=16, obs_scale=[1.] * 16)


def _pd():
    return ops.make_cfg(PD_ID)


def _dp():
    return ops.make_cfg(DP_ID)


def _tanh_range(env_id, r):
    return lambda: ops.make_cfg(env_id, policy_out_activation='tanh', action_range=r)


CFGS = (_pt, _pt16, _pd, _dp)
CFG_REFUSALS = [
    (lambda: _with(_pt(), env_kind=3), {}, 'unknown env kind 3'),
    (lambda: _with(_dp(), env_kind=-1), {}, 'unknown env kind -1'),
    (lambda: _with(_pt(), obs_dim=5), {}, 'the path-tracking model has obs_dim 6 .. 16 (got 5)'),
    (lambda: _with(_pt(), obs_dim=17), {}, 'the path-tracking model has obs_dim 6 .. 16 (got 17)'),
    (lambda: _with(_pd(), obs_dim=6), {}, 'the pendulum model has obs_dim 4 (got 6)'),
    (lambda: _with(_dp(), obs_dim=6), {}, 'the double-pendulum model has obs_dim 11 (got 6)'),
    (lambda: _with(_pt(), act_dim=1), {}, 'the path-tracking model has act_dim 2 (got 1)'),
    (lambda: _with(_pd(), act_dim=2), {}, 'the pendulum model has act_dim 1 (got 2)'),
    (lambda: _with(_dp(), act_dim=2), {}, 'the double-pendulum model has act_dim 1 (got 2)'),
    (_tanh_range(PT_ID, 1.0), {}, 'tanh policy with an action range'),
    (_tanh_range(PD_ID, 3.0), {}, 'tanh policy with an action range'),
    (_tanh_range(DP_ID, 1.0), {}, 'tanh policy with an action range'),
]
SHARED = CFG_REFUSALS + [(c, d, t) for c in CFGS for d, t in (
    (dict(rows=0), 'no rows'), (dict(rows=-2), 'no rows'), (dict(horizon=0), 'horizon >= 1'), (dict(horizon=-1), 'horizon >= 1'),
    (dict(horizon=32), 'horizon <= 31'), (dict(horizon=1 << 20), 'horizon <= 31'))]
C_OK = dict(rows=3, horizon=25)
C_REFUSALS = SHARED + [(c, {k: None}, 'null pointer') for c in CFGS for k in ('obs0', 'u', 'cost')] + [
    # the nullable ones may be null: what answers is the next thing wrong
    (_dp, dict(eps=None, grad=None, obs_traj=None, rew_traj=None, cost=None), 'null pointer'),
    (_tanh_range(DP_ID, 1.0), dict(eps=None, grad=None), 'tanh policy with an action range')]
S_OK = dict(rows=3, horizon=25, iters=100, tol=0.)
S_REFUSALS = SHARED + [(c, d, t) for c in CFGS for d, t in (
    (dict(iters=-1), 'iters >= 0'), (dict(tol=-1e-3), 'tol negative or NaN'), (dict(tol=math.nan), 'tol negative or NaN'),
    (dict(tol=-math.inf), 'tol negative or NaN'))] + \
    [(c, dict(iters=CAPS[k] + 1), 'iters <= %d for env kind %d (got %d)' % (CAPS[k], k, CAPS[k] + 1)) for c, k in ((_pt, 0), (_pd, 1), (_dp, 2))] + \
    [(c, dict(iters=1 << 30), 'iters <= ') for c in CFGS] + \
    [(c, {k: None}, 'null pointer') for c in CFGS for k in ('obs0', 'u', 'cost', 'pgnorm', 'info')] + [
    (_dp, dict(eps=None, info=None), 'null pointer'),
    (_tanh_range(PD_ID, 3.0), dict(eps=None), 'tanh policy with an action range')]


def _p(a, k):
    return NULL if (k in a and a[k] is None) else BUF.p(k)


def _call_cost(lib, cfg_ref, a):
    rc = lib.mpg_model_mpc_cost_grad(cfg_ref, I(a['rows']), I(a['horizon']), _p(a, 'obs0'), _p(a, 'u'), _p(a, 'eps'), _p(a, 'cost'),
                                     _p(a, 'grad'), _p(a, 'obs_traj'), _p(a, 'rew_traj'), NULL)
    assert BUF.untouched()
    return rc


def _call_solve(lib, cfg_ref, a):
    rc = lib.mpg_model_mpc_solve(cfg_ref, I(a['rows']), I(a['horizon']), I(a['iters']), F(a['tol']), _p(a, 'obs0'), _p(a, 'eps'), _p(a, 'u'),
                                 _p(a, 'cost'), _p(a, 'pgnorm'), _p(a, 'info'), NULL)
    assert BUF.untouched()
    return rc


test_cost_grad_refusals = H.refusal_test(COST, C_REFUSALS, C_OK, _call_cost)
test_solve_refusals = H.refusal_test(SOLVE, S_REFUSALS, S_OK, _call_solve)


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('name, call, ok', [(COST, _call_cost, C_OK), (SOLVE, _call_solve, S_OK)])
def test_a_null_configuration_is_refused(engine, name, call, ok):
    H.null_configuration_refused(engine, name, call, ok)


@pytest.mark.parametrize('name, at_least', [(COST, 9), (SOLVE, 12)])
def test_every_refusal_has_a_text_of_its_own(name, at_least):
    H.refusal_texts_are_unique(name, 'model_mpc.hip', at_least)


def test_the_caps_at_their_value_pass_the_iteration_check():
    """iters = the kind's cap is not what is refused: the null pointer behind it answers"""
    lib = L.lib()
    for make, k in ((_pt, 0), (_pd, 1), (_dp, 2)):
        cfg = make()
        assert _call_solve(lib, ctypes.byref(cfg), dict(S_OK, iters=CAPS[k], info=None)) == MPG_EINVAL
        assert lib.mpg_last_error().decode() == SOLVE + ': null pointer'


def test_the_first_thing_wrong_answers():
    """several things wrong at once: the refusals come in the order of the header's list"""
    lib = L.lib()
    cfg = _with(_dp(), policy_out_act=ops.make_cfg(DP_ID, policy_out_activation='tanh', action_range=1.0).policy_out_act, action_range=1.0)
    order = [(dict(rows=0, horizon=40, iters=-1, tol=-1., info=None), 'no rows'),
             (dict(rows=1, horizon=40, iters=-1, tol=-1., info=None), 'horizon <= 31'),
             (dict(rows=1, horizon=31, iters=-1, tol=-1., info=None), 'iters >= 0'),
             (dict(rows=1, horizon=31, iters=1, tol=-1., info=None), 'tol negative or NaN'),
             (dict(rows=1, horizon=31, iters=1, tol=0., info=None), 'null pointer'),
             (dict(rows=1, horizon=31, iters=1, tol=0.), 'tanh policy with an action range')]
    for a, text in order:
        assert _call_solve(lib, ctypes.byref(cfg), a) == MPG_EINVAL
        assert text in lib.mpg_last_error().decode(), (text, lib.mpg_last_error().decode())
    cfg.obs_dim = 12
    assert _call_solve(lib, ctypes.byref(cfg), order[0][0]) == MPG_EINVAL
    assert 'obs_dim 11 (got 12)' in lib.mpg_last_error().decode()


def test_a_refusal_reaches_python_as_mpg_error():
    cfg = _dp()
    with pytest.raises(L.MpgError, match=SOLVE + ': iters <= %d' % CAPS[2]):
        L.call(SOLVE, ctypes.byref(cfg), I(4), I(10), I(CAPS[2] + 1), F(0.), BUF.p('obs0'), NULL, BUF.p('u'), BUF.p('cost'), BUF.p('pgnorm'),
               BUF.p('info'), NULL)
    with pytest.raises(L.MpgError, match=COST + ': horizon <= 31'):
        L.call(COST, ctypes.byref(cfg), I(4), I(32), BUF.p('obs0'), BUF.p('u'), NULL, BUF.p('cost'), NULL, NULL, NULL, NULL)
    assert BUF.untouched()


def test_the_wrappers_check_their_shapes_before_the_library():
    from mpg_amd import mpc
    cfg = _dp()
    obs = torch.zeros(5, 11)
    with pytest.raises(ValueError, match=r'model_mpc_cost_grad: obs0 \(5, 6\) and u \(5, 10, 1\) are not \[rows, 11\] and \[rows, horizon, 1\]'):
        mpc.model_mpc_cost_grad(cfg, torch.zeros(5, 6), torch.zeros(5, 10, 1))
    with pytest.raises(ValueError, match='model_mpc_cost_grad: obs0'):
        mpc.model_mpc_cost_grad(cfg, obs, torch.zeros(5, 10, 2))
    with pytest.raises(ValueError, match=r'model_mpc_cost_grad: eps has shape \(5, 10\), the model noise of this call is \(10, 5\)'):
        mpc.model_mpc_cost_grad(cfg, obs, torch.zeros(5, 10, 1), eps=torch.zeros(5, 10))
    with pytest.raises(ValueError, match='model_mpc_solve: obs0'):
        mpc.model_mpc_solve(cfg, obs, torch.zeros(4, 10, 1))
    with pytest.raises(ValueError, match='model_mpc_solve: a start point u_init or a horizon'):
        mpc.model_mpc_solve(cfg, obs)


def test_the_product_module_imports_nothing_from_the_oracle():
    root = os.path.join(os.path.dirname(L.HEADER), '..')
    for f in ('mpc.py', 'evaluator.py'):
        src = open(os.path.join(root, 'mpg_amd', f)).read()
        assert not re.search(r'^\s*(import|from)\s+(oracle|tests)\b', src, flags=re.M)
        assert 'model_mpc_oracle' not in src
    from mpg_amd import evaluator, mpc
    for name in ('ModelMPC', 'run_model_mpc', 'model_mpc_cost_grad', 'model_mpc_solve'):
        assert callable(getattr(mpc, name))
    for name in ('reset_init_obs', 'cost_function', 'cost_and_gradient', 'solve'):
        assert callable(getattr(mpc.ModelMPC, name))
    assert callable(evaluator.ModelEvaluator.gap_to_mpc)
