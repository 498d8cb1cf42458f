"""mpg_env_rollout_pendulum and mpg_nstep_targets_clipped at the drop-in boundary, without a GPU: both libraries export them with the
declared argument types, and every refusal comes back as MPG_EINVAL with a text of its own before any launch (every pointer is FAKE: a
launch would fault)."""
import ctypes
import os
import re

import pytest

from mpg_amd import _lib as L
from mpg_amd import ops
from tests import abi_harness as H
from tests.abi_harness import CSRC, ENGINES, F, FAKE, I, NULL, MPG_EINVAL, _with, built  # noqa: F401 (built: the module's autouse fixture)

ROLLOUT, CLIPPED = 'mpg_env_rollout_pendulum', 'mpg_nstep_targets_clipped'
SZ = ctypes.c_size_t


@pytest.mark.parametrize('engine', ENGINES)
def test_both_libraries_export_the_entry_points(engine):
    lib = ctypes.CDLL(L.ENGINES[engine])
    for name in (ROLLOUT, CLIPPED):
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
    """the declarations of include/mpg_hip.h, argument by argument: mpg_env_rollout's in its order; mpg_nstep_targets' with the two
    bounds in front of y"""
    assert _declared(ROLLOUT) == ['const mpg_cfg_t* cfg', 'const float* policy_params', 'int rows', 'int n', 'const float* obs0',
                                  'const float* act0', 'float* rewards', 'float* last_obs', 'mpg_stream_t stream']
    assert _declared(ROLLOUT) == _declared('mpg_env_rollout')
    plain = _declared('mpg_nstep_targets')
    assert _declared(CLIPPED) == ['const mpg_cfg_t* cfg', 'const float* policy_t', 'const float* q1t', 'int rows', 'int n',
                                  'const float* rewards', 'const float* last_obs', 'float q_lo', 'float q_hi', 'float* y', 'void* ws',
                                  'size_t ws_bytes', 'mpg_stream_t stream']
    assert _declared(CLIPPED) == plain[:7] + ['float q_lo', 'float q_hi'] + plain[7:]


def test_the_clip_constants_are_declared_once_and_mirrored():
    src = open(L.HEADER).read()
    lo = re.findall(r'#define\s+MPG_PENDULUM_NSTEP_Q_LO\s+\(?(-?[0-9.]+)f\)?', src)
    hi = re.findall(r'#define\s+MPG_PENDULUM_NSTEP_Q_HI\s+\(?(-?[0-9.]+)f\)?', src)
    assert len(lo) == 1 and len(hi) == 1, (lo, hi)
    assert (float(lo[0]), float(hi[0])) == (-0.5, 0.0) == tuple(ops.PENDULUM_NSTEP_Q_CLIP)
    assert 'mpg_learner.py:163-164' in src
    # the driver takes them from the header
    drv = open(os.path.join(CSRC, 'train_step.cpp')).read()
    assert 'MPG_PENDULUM_NSTEP_Q_LO, MPG_PENDULUM_NSTEP_Q_HI' in drv and '-0.5f' not in drv


def _cfg():
    return ops.make_cfg('InvertedPendulumConti-v0')


# ---- mpg_env_rollout_pendulum ---------------------------------------------------------------------------------------------------
OK = dict(policy=FAKE, rows=40, n=25, obs0=FAKE, act0=FAKE, rewards=FAKE, last_obs=FAKE)
REFUSALS = [
    # (cfg, what differs from OK, the text of the refusal)
    (lambda: ops.make_cfg('InvertedDoublePendulum-v2'), {}, 'MuJoCo'),
    (lambda: ops.make_cfg('PathTracking-v0'), {}, 'pendulum env only'),
    (lambda: _with(_cfg(), env_kind=3), {}, 'pendulum env only'),
    (lambda: _with(_cfg(), obs_dim=6), {}, 'obs_dim 4 only'),
    (lambda: _with(_cfg(), obs_dim=3), {}, 'obs_dim 4 only'),
    (lambda: _with(_cfg(), act_dim=2), {}, 'act_dim 1 only'),
    (_cfg, dict(n=0), 'n >= 1'),
    (_cfg, dict(n=-25), 'n >= 1'),
    (_cfg, dict(n=1025), 'n <= 1024'),
    (_cfg, dict(rows=0), 'no rows'),
    (_cfg, dict(rows=-1), 'no rows'),
] + [(_cfg, {k: NULL}, 'null pointer') for k in ('policy', 'obs0', 'act0', 'rewards', 'last_obs')] + [
    (lambda: ops.make_cfg('InvertedPendulumConti-v0', policy_out_activation='tanh', action_range=3.0), {}, 'tanh policy with an action range'),
]


def _rollout(lib, cfg_ref, a):
    return getattr(lib, ROLLOUT)(cfg_ref, a['policy'], I(a['rows']), I(a['n']), a['obs0'], a['act0'], a['rewards'], a['last_obs'], NULL)


test_rollout_refusals = H.refusal_test(ROLLOUT, REFUSALS, OK, _rollout)


@pytest.mark.parametrize('engine', ENGINES)
def test_rollout_refuses_a_null_configuration(engine):
    H.null_configuration_refused(engine, ROLLOUT, _rollout, OK)


def test_every_rollout_refusal_has_a_text_of_its_own():
    H.refusal_texts_are_unique(ROLLOUT, 'env_cart_pole.hip', 10)


def test_the_path_tracking_entry_points_answer_the_pendulum_as_they_did():
    """new names, not a widening: mpg_env_rollout still refuses a pendulum cfg"""
    lib = L.lib()
    cfg = _cfg()
    rc = lib.mpg_env_rollout(ctypes.byref(cfg), FAKE, I(40), I(25), FAKE, FAKE, FAKE, FAKE, NULL)
    assert rc == MPG_EINVAL and 'path-tracking env only' in lib.mpg_last_error().decode()


# ---- mpg_nstep_targets_clipped --------------------------------------------------------------------------------------------------
TOK = dict(policy_t=FAKE, q1t=FAKE, rows=64, n=25, rewards=FAKE, last_obs=FAKE, lo=-0.5, hi=0.0, y=FAKE, ws=FAKE, ws_bytes=1 << 30)
INF, NAN, BIG = float('inf'), float('nan'), 3.4028234664e38
T_REFUSALS = [
    # mpg_nstep_targets' own: one text ("bad argument"), as that entry point answers them
    (lambda: _with(_cfg(), obs_dim=0), {}, 'bad argument'),
    (lambda: ops.make_cfg('InvertedPendulumConti-v0', policy_out_activation='tanh', action_range=3.0), {}, 'bad argument'),
    (_cfg, dict(rows=0), 'bad argument'),
    (_cfg, dict(n=0), 'bad argument'),
] + [(_cfg, {k: NULL}, 'bad argument') for k in ('policy_t', 'q1t', 'rewards', 'last_obs', 'y', 'ws')] + [
    # the bounds
    (_cfg, dict(lo=-INF), 'must be finite'),
    (_cfg, dict(hi=INF), 'must be finite'),
    (_cfg, dict(lo=NAN), 'must be finite'),
    (_cfg, dict(hi=NAN), 'must be finite'),
    (_cfg, dict(lo=0.5, hi=0.0), 'empty clip interval'),
    (_cfg, dict(lo=BIG, hi=-BIG), 'empty clip interval'),
]


def _clipped(lib, cfg_ref, a):
    return getattr(lib, CLIPPED)(cfg_ref, a['policy_t'], a['q1t'], I(a['rows']), I(a['n']), a['rewards'], a['last_obs'], F(a['lo']),
                                 F(a['hi']), a['y'], a['ws'], SZ(a['ws_bytes']), NULL)


test_clipped_target_refusals = H.refusal_test(CLIPPED, T_REFUSALS, TOK, _clipped)


@pytest.mark.parametrize('engine', ENGINES)
def test_clipped_target_refuses_a_null_configuration_and_a_short_workspace(engine):
    with L.engine(engine):
        lib = L.lib()
        assert _clipped(lib, NULL, dict(TOK)) == MPG_EINVAL
        assert lib.mpg_last_error().decode().startswith(CLIPPED + ':')
        # the workspace is mpg_nstep_targets': one byte short of the same query is MPG_EWORKSPACE under this entry point's name
        cfg = _cfg()
        lib.mpg_q_targets_workspace_bytes.restype = ctypes.c_size_t
        need = lib.mpg_q_targets_workspace_bytes(ctypes.byref(cfg), I(64))
        assert need > 0
        rc = _clipped(lib, ctypes.byref(cfg), dict(TOK, ws_bytes=need - 1))
        msg = lib.mpg_last_error().decode()
        assert rc not in (0, MPG_EINVAL) and msg.startswith(CLIPPED + ':') and str(need) in msg, (rc, msg)
        rc2 = lib.mpg_nstep_targets(ctypes.byref(cfg), FAKE, FAKE, I(64), I(25), FAKE, FAKE, FAKE, FAKE, SZ(need - 1), NULL)
        assert rc2 == rc and lib.mpg_last_error().decode().startswith('mpg_nstep_targets:')


# ---- ops ------------------------------------------------------------------------------------------------------------------------
def test_the_wrappers_call_path_raises_mpg_error():
    """L.call - what ops.env_rollout_pendulum and ops.nstep_targets(.., clip=) send their arguments through - turns a refusal into
    MpgError with the library's text.  The wrappers themselves take device tensors and the current stream (ops._f32, L.ptr, L.stream),
    so they are invoked where a device is: tests/test_env_rollout_pendulum_gpu.py::test_ops_wrappers_raise_mpg_error."""
    import inspect
    cfg = ops.make_cfg('PathTracking-v0')
    with pytest.raises(L.MpgError, match=ROLLOUT + ': pendulum env only'):
        L.call(ROLLOUT, ctypes.byref(cfg), FAKE, I(40), I(25), FAKE, FAKE, FAKE, FAKE, NULL)
    cfg = _cfg()
    with pytest.raises(L.MpgError, match=CLIPPED + ': empty clip interval'):
        L.call(CLIPPED, ctypes.byref(cfg), FAKE, FAKE, I(64), I(25), FAKE, FAKE, F(0.5), F(0.0), FAKE, FAKE, SZ(1 << 30), NULL)
    # (the pendulum's wrapper is ops.env_rollout held to this entry point, whatever the cfg's env kind)
    assert "entry='%s'" % ROLLOUT in inspect.getsource(ops.env_rollout_pendulum)
    assert 'L.call(entry or ' in inspect.getsource(ops.env_rollout)
    assert "L.call('%s'" % CLIPPED in inspect.getsource(ops.nstep_targets)
    # the default leaves today's call untouched
    assert inspect.signature(ops.nstep_targets).parameters['clip'].default is None
