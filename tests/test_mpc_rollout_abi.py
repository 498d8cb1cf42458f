"""mpg_mpc_rollout at the drop-in boundary and mpc_rl_summary, without a GPU: both libraries export the entry point with the declared
argument types, and every refusal comes back as MPG_EINVAL with a text of its own before any launch, the outputs untouched (the buffers
are HOST arrays with a pattern in them: a launch would fault, a refusal never dereferences them)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from mpg_amd import _lib as L

NAME = 'mpg_mpc_rollout'
NULL = ctypes.c_void_p(0)
I, F = ctypes.c_int, ctypes.c_float
MPG_EINVAL = -1000
ENGINES = sorted(L.ENGINES)
ROOT = os.path.join(os.path.dirname(L.HEADER), '..')
SRC = os.path.join(ROOT, 'mpg_amd', 'csrc', 'env_path_tracking.hip')
PATTERN = 0x5A
REQUIRED = ('state', 'obs_io', 'u_io', 'obs_traj', 'plan_traj', 'rew_traj')
NULLABLE = ('cost_traj', 'pgnorm_traj', 'info_traj', 'done_out', 'done_intended_out')


@pytest.fixture(scope='module', autouse=True)
def built():
    from mpg_amd import build as B
    return B.build(verbose=False)


@pytest.mark.parametrize('engine', ENGINES)
def test_both_libraries_export_the_entry_point(engine):
    lib = ctypes.CDLL(L.ENGINES[engine])
    assert NAME in L.declared_symbols()
    assert hasattr(lib, NAME)
    assert L.declared_return_types()[NAME] == 'int'
    assert lib.mpg_abi_version() == 10           # a function was added: no layout or signature changed


def test_declared_argument_types_and_bounds():
    hdr = open(L.HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    m = re.search(r'\bint\s+%s\s*\((.*?)\)\s*;' % NAME, src, flags=re.S)
    assert m
    assert [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')] == [
        'int n', 'int steps', 'int horizon', 'int iters', 'float tol', 'int warm_start', 'float* state', 'float* obs_io', 'float* u_io',
        'float* obs_traj', 'float* plan_traj', 'float* rew_traj', 'float* cost_traj', 'float* pgnorm_traj', 'int* info_traj',
        'uint8_t* done_out', 'uint8_t* done_intended_out', 'mpg_stream_t stream']
    assert re.findall(r'#define\s+MPG_MPC_ROLLOUT_MAX_STEPS\s+(\S+)', hdr) == ['1024']
    assert re.findall(r'#define\s+MPG_MPC_ROLLOUT_MAX_WORK\s+(\S+)', hdr) == ['2048']
    from mpg_amd import mpc
    assert (mpc.MAX_ROLLOUT_STEPS, mpc.MAX_ROLLOUT_WORK) == (1024, 2048)


class Buffers(object):
    """host arrays behind every pointer argument, filled with a pattern"""

    def __init__(self):
        self.raw = {k: (ctypes.c_ubyte * 4096)(*([PATTERN] * 4096)) for k in REQUIRED + NULLABLE}

    def p(self, k):
        return ctypes.cast(self.raw[k], ctypes.c_void_p)

    def untouched(self):
        return all(bytes(v) == bytes([PATTERN]) * 4096 for v in self.raw.values())


OK = dict(n=3, steps=4, horizon=25, iters=200, tol=0., warm_start=0)
REFUSALS = [(dict(n=0), 'no agents'), (dict(n=-2), 'no agents'), (dict(steps=0), 'steps >= 1'), (dict(steps=-3), 'steps >= 1'),
            (dict(steps=1025, iters=1), 'steps <= 1024'), (dict(steps=1 << 30, iters=0), 'steps <= 1024'),
            (dict(horizon=0), 'horizon >= 1'), (dict(horizon=-1), 'horizon >= 1'), (dict(horizon=32), 'horizon <= 31'),
            (dict(horizon=1 << 20), 'horizon <= 31'), (dict(iters=-1), 'iters >= 0'), (dict(iters=1001), 'iters <= 1000'),
            (dict(steps=11, iters=200), 'steps * iters = 2200'), (dict(steps=3, iters=1000), 'steps * iters = 3000'),
            (dict(steps=1024, iters=1000), 'steps * iters = 1024000'), (dict(tol=-1e-3), 'tol negative or NaN'),
            (dict(tol=math.nan), 'tol negative or NaN'), (dict(tol=-math.inf), 'tol negative or NaN'), (dict(warm_start=2), 'warm_start is 0 or 1'),
            (dict(warm_start=-1), 'warm_start is 0 or 1')] + [({k: None}, 'null pointer') for k in REQUIRED]


def _call(lib, a, buf):
    def p(k):
        return NULL if (k in a and a[k] is None) else buf.p(k)
    return lib.mpg_mpc_rollout(I(a['n']), I(a['steps']), I(a['horizon']), I(a['iters']), F(a['tol']), I(a['warm_start']),
                               *([p(k) for k in REQUIRED + NULLABLE] + [NULL]))


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('case', range(len(REFUSALS)), ids=['%02d-%s' % (i, re.sub(r'[^a-z0-9]+', '_', c[1].lower())) for i, c in enumerate(REFUSALS)])
def test_refusals(engine, case):
    diff, text = REFUSALS[case]
    with L.engine(engine):
        lib = L.lib()
        a = dict(OK)
        a.update(diff)
        buf = Buffers()
        rc = _call(lib, a, buf)
        msg = lib.mpg_last_error().decode()
        assert rc == MPG_EINVAL, (rc, msg)
        assert msg.startswith(NAME + ':') and text in msg, msg
        assert buf.untouched()


def test_the_work_cap_is_a_bound_on_the_product_alone():
    """2048 iterations pass every refusal (the next thing wrong answers), 2049 and more do not"""
    lib = L.lib()
    buf = Buffers()
    for steps, iters in ((2, 1000), (1024, 2), (8, 256)):
        assert steps * iters <= 2048
        assert _call(lib, dict(OK, steps=steps, iters=iters, tol=-1.), buf) == MPG_EINVAL
        assert 'tol negative or NaN' in lib.mpg_last_error().decode()
    for steps, iters in ((3, 683), (1024, 3)):
        assert steps * iters > 2048
        assert _call(lib, dict(OK, steps=steps, iters=iters, tol=-1.), buf) == MPG_EINVAL
        assert 'steps * iters' in lib.mpg_last_error().decode()
    assert buf.untouched()


def test_the_first_thing_wrong_answers():
    """several things wrong at once: the refusals come in the order of the header's list"""
    lib = L.lib()
    buf = Buffers()
    order = [(dict(n=0, steps=0, horizon=40, iters=-1, tol=-1., warm_start=5, state=None), 'no agents'),
             (dict(steps=0, horizon=40, iters=-1, tol=-1., warm_start=5, state=None), 'steps >= 1'),
             (dict(horizon=40, iters=-1, tol=-1., warm_start=5, state=None), 'horizon <= 31'),
             (dict(iters=-1, tol=-1., warm_start=5, state=None), 'iters >= 0'),
             (dict(steps=100, tol=-1., warm_start=5, state=None), 'steps * iters'),
             (dict(tol=-1., warm_start=5, state=None), 'tol negative or NaN'),
             (dict(warm_start=5, state=None), 'warm_start is 0 or 1'),
             (dict(state=None), 'null pointer')]
    for diff, text in order:
        assert _call(lib, dict(OK, **diff), buf) == MPG_EINVAL
        assert text in lib.mpg_last_error().decode(), (text, lib.mpg_last_error().decode())
    assert buf.untouched()


def test_every_refusal_has_a_text_of_its_own():
    src = open(SRC).read()
    body = src[src.index('extern "C" int %s(' % NAME):]
    body = body[:body.index('hipLaunchKernelGGL')]
    texts = re.findall(r'MPG_REQUIRE\(.*?"(%s: [^"]*)"' % NAME, body, flags=re.S)
    assert len(texts) == 11 and len(set(texts)) == len(texts), texts


def test_a_refusal_reaches_python_as_mpg_error():
    buf = Buffers()
    with pytest.raises(L.MpgError, match=NAME + ': steps \\* iters = 2200'):
        L.call(NAME, I(4), I(11), I(25), I(200), F(0.), I(0), *([buf.p(k) for k in REQUIRED + NULLABLE] + [NULL]))
    assert buf.untouched()


def test_the_product_module_has_the_new_names_and_keeps_the_old_defaults():
    import inspect
    from mpg_amd import mpc
    for name in ('mpc_rollout', 'mpc_rl_summary', 'run_mpc'):
        assert callable(getattr(mpc, name))
    sig = inspect.signature(mpc.run_mpc).parameters
    assert (sig['one_launch'].default, sig['warm_start'].default, sig['tol'].default) == (False, False, 0.)
    assert [p for p in sig][:7] == ['policy', 'num_agent', 'steps', 'horizon', 'seed', 'iters', 'device']
    sig = inspect.signature(mpc.mpc_rollout).parameters
    assert [p for p in sig] == ['env', 'u', 'steps', 'horizon', 'iters', 'tol', 'warm_start']
    assert (sig['iters'].default, sig['tol'].default, sig['warm_start'].default) == (200, 0., False)


def test_mpc_rl_summary_against_a_numpy_restatement():
    """a hand-made record of 7 steps and 3 agents against mpc/mpc_ipopt.py:303-311 written out in numpy, agent by agent - without the
    - 20 of :286-287: this project's observations hold v_x - 20 already"""
    from mpg_amd import mpc
    rng = np.random.default_rng(4)
    steps, n = 7, 3
    rec = {'mpc_obs': rng.normal(0, 2, (steps, n, 6)), 'rl_obs': rng.normal(0, 2, (steps, n, 6)), 'mpc_rew': -rng.uniform(0, 3, (steps, n)),
           'rl_rew': -rng.uniform(0, 3, (steps, n)), 'mpc_action': rng.uniform(-1, 1, (steps, n, 5, 2))}
    rec = {k: v.astype(np.float32) for k, v in rec.items()}
    rec['mpc_rew'][0] = rec['rl_rew'][0] = 0.
    got = mpc.mpc_rl_summary({k: torch.from_numpy(v) for k, v in rec.items()})
    assert sorted(got) == sorted('%s_%s' % (w, k) for w in ('mpc', 'rl') for k in ('delta_y_mse', 'delta_v_mse', 'delta_phi_mse', 'rew_sum'))
    for who in ('mpc', 'rl'):
        for a in range(n):
            obs = rec[who + '_obs'][:, a].astype(np.float64)
            want = {'delta_y_mse': np.sqrt(np.mean(np.square(obs[:, 3]))), 'delta_v_mse': np.sqrt(np.mean(np.square(obs[:, 0]))),
                    'delta_phi_mse': np.sqrt(np.mean(np.square(obs[:, 4]))), 'rew_sum': np.sum(rec[who + '_rew'][:, a].astype(np.float64))}
            for k, v in want.items():
                t = got['%s_%s' % (who, k)]
                assert t.shape == (n,)
                np.testing.assert_allclose(float(t[a]), v, rtol=1e-12, atol=0)
