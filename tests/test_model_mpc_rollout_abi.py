"""mpg_model_mpc_rollout at the drop-in boundary, without a GPU: both libraries export it with the declared argument types, the bounds are
macros the code uses and Python mirrors, and every refusal comes back as MPG_EINVAL with the entry's name and a text of its own before
any launch, the outputs untouched (the buffers are HOST arrays with a pattern in them: a launch would fault, a refusal never
dereferences them).  The Python wrappers' own refusals beside them."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops
from tests import abi_harness as H
from tests.abi_harness import ENGINES, F, I, NULL, MPG_EINVAL, _with, built  # noqa: F401 (built: the module's autouse fixture)
from tests.test_model_mpc_abi import CAPS, CFG_REFUSALS, CFGS, DP_ID, PD_ID, _define, _dp, _pd, _pt, _tanh_range

NAME = 'mpg_model_mpc_rollout'
PATTERN = 0x5A
REQUIRED = ('obs_io', 'u_io', 'obs_traj', 'plan_traj', 'rew_traj')
NULLABLE = ('eps', 'cost_traj', 'pgnorm_traj', 'info_traj')
KINDS = ((0, 'PATH_TRACKING'), (1, 'PENDULUM'), (2, 'DOUBLE_PENDULUM'))
WORK = {k: _define('MPG_MODEL_MPC_ROLLOUT_MAX_WORK_' + n) for k, n in KINDS}
MAX_STEPS = _define('MPG_MODEL_MPC_ROLLOUT_MAX_STEPS')


class Buffers(object):
    """host arrays behind every pointer argument, filled with a pattern"""

    def __init__(self):
        self.raw = {k: (ctypes.c_ubyte * 4096)(*([PATTERN] * 4096)) for k in REQUIRED + NULLABLE}

    def p(self, k):
        return ctypes.cast(self.raw[k], ctypes.c_void_p)

    def untouched(self):
        return all(bytes(v) == bytes([PATTERN]) * 4096 for v in self.raw.values())


BUF = Buffers()


@pytest.mark.parametrize('engine', ENGINES)
def test_both_libraries_export_the_entry_point(engine):
    lib = ctypes.CDLL(L.ENGINES[engine])
    assert NAME in L.declared_symbols()
    assert hasattr(lib, NAME)
    assert L.declared_return_types()[NAME] == 'int'
    assert lib.mpg_abi_version() == 10           # a function was added: no layout or signature changed
    assert L.ABI_VERSION == 10


def test_declared_argument_types():
    src = re.sub(r'/\*.*?\*/', '', open(L.HEADER).read(), flags=re.S)
    m = re.search(r'\bint\s+%s\s*\((.*?)\)\s*;' % NAME, src, flags=re.S)
    assert m
    assert [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')] == [
        'const mpg_cfg_t* cfg', 'int n', 'int steps', 'int horizon', 'int iters', 'float tol', 'int warm_start', 'float* obs_io', 'float* u_io',
        'const float* eps', 'float* obs_traj', 'float* plan_traj', 'float* rew_traj', 'float* cost_traj', 'float* pgnorm_traj', 'int* info_traj',
        'mpg_stream_t stream']


def test_the_bounds_are_defines_the_code_uses_and_python_mirrors():
    assert MAX_STEPS == 1024
    assert WORK == {0: 2048, 1: 2048, 2: 400}
    src = open(os.path.join(H.CSRC, 'model_mpc.hip')).read()
    assert 'MPG_MODEL_MPC_ROLLOUT_MAX_STEPS' in src
    for _, n in KINDS:
        assert 'MPG_MODEL_MPC_ROLLOUT_MAX_WORK_' + n in src
    from mpg_amd import mpc
    assert mpc.MODEL_MAX_ROLLOUT_WORK == WORK and mpc.MODEL_MAX_ROLLOUT_STEPS == MAX_STEPS
    # a cap holds at least one solve of the kind's longest: chunks of one step are always possible
    assert all(WORK[k] >= CAPS[k] for k in WORK)
    # the solve is the one loop and the plant's step the unit's own forward pass
    body = src[src.index('k_model_mpc_rollout('):src.index('// launch(ENV{})')]
    assert 'mpc::solve(Problem<ENV>{' in body and 'plant_step<ENV>(' in body
    assert 'forward<ENV>(1, ' in open(os.path.join(H.CSRC, 'model_mpc.h')).read()


OK = dict(n=3, steps=4, horizon=25, iters=100, tol=0., warm_start=0)
REFUSALS = CFG_REFUSALS + [(c, d, t) for c in CFGS for d, t in (
    (dict(n=0), 'no agents'), (dict(n=-2), 'no agents'), (dict(steps=0), 'steps >= 1'), (dict(steps=-3), 'steps >= 1'),
    (dict(steps=MAX_STEPS + 1, iters=1), 'steps <= 1024'), (dict(steps=1 << 30, iters=0), 'steps <= 1024'),
    (dict(horizon=0), 'horizon >= 1'), (dict(horizon=-1), 'horizon >= 1'), (dict(horizon=32), 'horizon <= 31'),
    (dict(horizon=1 << 20), 'horizon <= 31'), (dict(iters=-1), 'iters >= 0'), (dict(iters=1 << 30), 'iters <= '),
    (dict(tol=-1e-3), 'tol negative or NaN'), (dict(tol=math.nan), 'tol negative or NaN'), (dict(tol=-math.inf), 'tol negative or NaN'),
    (dict(warm_start=2), 'warm_start is 0 or 1'), (dict(warm_start=-1), 'warm_start is 0 or 1'))] + \
    [(c, dict(steps=1, iters=CAPS[k] + 1), 'iters <= %d for env kind %d (got %d)' % (CAPS[k], k, CAPS[k] + 1)) for c, k in ((_pt, 0), (_pd, 1), (_dp, 2))] + \
    [(c, dict(steps=s, iters=i), 'steps * iters = %d solver iterations in one launch, at most %d for env kind %d' % (s * i, WORK[k], k))
     for c, k in ((_pt, 0), (_pd, 1), (_dp, 2)) for s, i in ((WORK[k] // 100 + 1, 100), (MAX_STEPS, CAPS[k]), (3, CAPS[k]))] + \
    [(c, {k: None}, 'null pointer') for c in CFGS for k in REQUIRED] + [
    # the nullable ones may be null, each on its own and all at once: what answers is the next thing wrong
    (_dp, dict(eps=None, cost_traj=None, pgnorm_traj=None, info_traj=None, rew_traj=None), 'null pointer'),
    (_pt, dict(eps=None, tol=-1.), 'tol negative or NaN'), (_pd, dict(cost_traj=None, tol=-1.), 'tol negative or NaN'),
    (_dp, dict(pgnorm_traj=None, tol=-1.), 'tol negative or NaN'), (_pt, dict(info_traj=None, tol=-1.), 'tol negative or NaN'),
    (_tanh_range(PD_ID, 3.0), dict(eps=None, info_traj=None), 'tanh policy with an action range')]


def _p(a, k):
    return NULL if (k in a and a[k] is None) else BUF.p(k)


def _call(lib, cfg_ref, a):
    rc = lib.mpg_model_mpc_rollout(cfg_ref, I(a['n']), I(a['steps']), I(a['horizon']), I(a['iters']), F(a['tol']), I(a['warm_start']),
                                   _p(a, 'obs_io'), _p(a, 'u_io'), _p(a, 'eps'), _p(a, 'obs_traj'), _p(a, 'plan_traj'), _p(a, 'rew_traj'),
                                   _p(a, 'cost_traj'), _p(a, 'pgnorm_traj'), _p(a, 'info_traj'), NULL)
    assert BUF.untouched()
    return rc


test_refusals = H.refusal_test(NAME, REFUSALS, OK, _call)


@pytest.mark.parametrize('engine', ENGINES)
def test_a_null_configuration_is_refused(engine):
    H.null_configuration_refused(engine, NAME, _call, OK)


def test_every_refusal_has_a_text_of_its_own():
    H.refusal_texts_are_unique(NAME, 'model_mpc.hip', 16)


def test_the_work_cap_is_a_bound_on_the_product_alone():
    """the cap passes every refusal (the next thing wrong answers), one more iteration does not"""
    lib = L.lib()
    for make, k in ((_pt, 0), (_pd, 1), (_dp, 2)):
        cfg = make()
        for steps, iters in ((WORK[k] // CAPS[k], CAPS[k]), (MAX_STEPS, WORK[k] // MAX_STEPS), (WORK[k] // 8, 8), (MAX_STEPS, 0)):
            assert steps * iters <= WORK[k] and steps >= 1
            assert _call(lib, ctypes.byref(cfg), dict(OK, steps=steps, iters=iters, tol=-1.)) == MPG_EINVAL
            assert 'tol negative or NaN' in lib.mpg_last_error().decode()
        for steps, iters in ((WORK[k] // 8 + 1, 8), (MAX_STEPS, WORK[k] // MAX_STEPS + 1)):
            assert steps * iters > WORK[k]
            assert _call(lib, ctypes.byref(cfg), dict(OK, steps=steps, iters=iters, tol=-1.)) == MPG_EINVAL
            assert 'steps * iters' in lib.mpg_last_error().decode()


def test_the_first_thing_wrong_answers():
    """several things wrong at once: the refusals come in the order of the header's list"""
    lib = L.lib()
    cfg = _with(_dp(), policy_out_act=ops.make_cfg(DP_ID, policy_out_activation='tanh', action_range=1.0).policy_out_act, action_range=1.0)
    wrong = dict(n=0, steps=0, horizon=40, iters=-1, tol=-1., warm_start=5, obs_io=None)
    order = [({}, 'no agents'), (dict(n=1), 'steps >= 1'), (dict(n=1, steps=2000), 'steps <= 1024'), (dict(n=1, steps=9), 'horizon <= 31'),
             (dict(n=1, steps=9, horizon=0), 'horizon >= 1'), (dict(n=1, steps=9, horizon=31), 'iters >= 0'),
             (dict(n=1, steps=9, horizon=31, iters=401), 'iters <= 400'), (dict(n=1, steps=9, horizon=31, iters=100), 'steps * iters = 900'),
             (dict(n=1, steps=4, horizon=31, iters=100), 'tol negative or NaN'), (dict(n=1, steps=4, horizon=31, iters=100, tol=0.), 'warm_start is 0 or 1'),
             (dict(n=1, steps=4, horizon=31, iters=100, tol=0., warm_start=1), 'null pointer'),
             (dict(n=1, steps=4, horizon=31, iters=100, tol=0., warm_start=1, obs_io=0), 'tanh policy with an action range')]
    for diff, text in order:
        assert _call(lib, ctypes.byref(cfg), dict(wrong, **diff)) == MPG_EINVAL
        assert text in lib.mpg_last_error().decode(), (text, lib.mpg_last_error().decode())
    cfg.obs_dim = 12
    assert _call(lib, ctypes.byref(cfg), wrong) == MPG_EINVAL
    assert 'obs_dim 11 (got 12)' in lib.mpg_last_error().decode()


def test_a_refusal_reaches_python_as_mpg_error():
    cfg = _dp()
    with pytest.raises(L.MpgError, match=NAME + ': steps \\* iters = 500'):
        L.call(NAME, ctypes.byref(cfg), I(4), I(5), I(10), I(100), F(0.), I(0), BUF.p('obs_io'), BUF.p('u_io'), NULL, BUF.p('obs_traj'),
               BUF.p('plan_traj'), BUF.p('rew_traj'), NULL, NULL, NULL, NULL)
    assert BUF.untouched()


def test_the_wrappers_check_their_shapes_before_the_library():
    from mpg_amd import mpc
    cfg = _dp()
    obs = torch.zeros(5, 11)
    with pytest.raises(ValueError, match=r'model_mpc_rollout: obs0 \(5, 6\) and u \(5, 10, 1\) are not \[rows, 11\] and \[rows, horizon, 1\]'):
        mpc.model_mpc_rollout(cfg, torch.zeros(5, 6), torch.zeros(5, 10, 1), 3)
    with pytest.raises(ValueError, match='model_mpc_rollout: obs0'):
        mpc.model_mpc_rollout(cfg, obs, torch.zeros(4, 10, 1), 3)
    with pytest.raises(ValueError, match=r'model_mpc_rollout: eps has shape \(5, 3\), the model noise of this call is \(3, 5\)'):
        mpc.model_mpc_rollout(cfg, obs, torch.zeros(5, 10, 1), 3, eps=torch.zeros(5, 3))
    for one_launch in (False, True):
        with pytest.raises(ValueError, match=r'run_model_mpc: eps has shape \(5, 3\), the model noise of this call is \(3, 5\)'):
            mpc.run_model_mpc(cfg, obs, 3, 10, one_launch=one_launch, eps=torch.zeros(5, 3))
        for steps in (0, -2):           # no record of no steps, in either form: a named refusal, not torch's about an empty list
            with pytest.raises(ValueError, match=r'run_model_mpc: steps >= 1 \(got %d\)' % steps):
                mpc.run_model_mpc(cfg, obs, steps, 10, one_launch=one_launch)
    # (the library's refusals through the wrappers need device tensors: tests/test_model_mpc_rollout_gpu.py)


def test_the_product_modules_have_the_new_names_and_keep_the_old_defaults():
    from mpg_amd import evaluator, mpc
    sig = inspect.signature(mpc.model_mpc_rollout).parameters
    assert [p for p in sig] == ['cfg', 'obs', 'u', 'steps', 'iters', 'tol', 'warm_start', 'eps']
    assert (sig['iters'].default, sig['tol'].default, sig['warm_start'].default, sig['eps'].default) == (200, 0., False, None)
    sig = inspect.signature(mpc.run_model_mpc).parameters
    assert [p for p in sig] == ['env_id_or_cfg', 'init_obs', 'steps', 'horizon', 'iters', 'tol', 'warm_start', 'one_launch', 'eps']
    assert (sig['iters'].default, sig['tol'].default, sig['warm_start'].default, sig['one_launch'].default, sig['eps'].default) == (200, 0., False, False, None)
    sig = inspect.signature(evaluator.ModelEvaluator.gap_to_mpc_closed_loop).parameters
    assert [p for p in sig] == ['self', 'init_obs', 'steps', 'horizon', 'iters', 'tol', 'warm_start', 'eps']
    assert (sig['iters'].default, sig['tol'].default, sig['warm_start'].default) == (200, 1e-3, True)
    assert callable(mpc.model_rollout_chunk)
    for f in ('mpc.py', 'evaluator.py'):
        src = open(os.path.join(os.path.dirname(L.HEADER), '..', 'mpg_amd', f)).read()
        assert not re.search(r'^\s*(import|from)\s+(oracle|tests)\b', src, flags=re.M) and 'model_mpc_rollout_oracle' not in src
