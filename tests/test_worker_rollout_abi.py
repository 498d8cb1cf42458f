"""mpg_worker_rollout at the drop-in boundary, without a GPU: both libraries export it with the declared argument types, and every
refusal comes back as MPG_EINVAL with a text of its own before any launch (every pointer is FAKE: a launch would fault)."""
import ctypes
import re

import pytest

from mpg_amd import _lib as L
from mpg_amd import ops
from tests import abi_harness as H
from tests.abi_harness import ENGINES, F, FAKE, I, NULL, U64, _with, built  # noqa: F401 (built: the module's autouse fixture)


@pytest.mark.parametrize('engine', ENGINES)
def test_both_libraries_export_the_entry_point(engine):
    assert 'mpg_worker_rollout' in L.declared_symbols()
    lib = ctypes.CDLL(L.ENGINES[engine])
    assert hasattr(lib, 'mpg_worker_rollout')
    assert lib.mpg_abi_version() == 10           # a function was added: no layout or signature changed
    assert L.declared_return_types()['mpg_worker_rollout'] == 'int'


def test_declared_argument_types():
    """the declaration of include/mpg_hip.h, argument by argument: mpg_worker_step's without the draw, `iters` after n"""
    src = re.sub(r'/\*.*?\*/', '', open(L.HEADER).read(), flags=re.S)
    m = re.search(r'\bint\s+mpg_worker_rollout\s*\((.*?)\)\s*;', src, flags=re.S)
    assert m
    args = [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')]
    assert args == ['const mpg_cfg_t* cfg', 'const float* policy_params', 'int n', 'int iters', 'float* state', 'float* obs_io',
                    'float explore_sigma', 'uint64_t noise_seed', 'uint64_t noise_ctr', 'float* act_out', 'int capacity', 'int next_idx',
                    'float* ring_obs', 'float* ring_act', 'float* ring_rew', 'float* ring_obs2', 'uint8_t* ring_done', 'uint64_t env_seed',
                    'uint64_t env_ctr', 'uint8_t* done_out', 'mpg_stream_t stream']


def _cfg(obs_dim=6):
    return ops.make_cfg('PathTracking-v0', obs_dim=obs_dim)


OK = dict(policy=FAKE, n=8, iters=64, state=FAKE, obs_io=FAKE, act_out=FAKE, capacity=512, next_idx=0, ring_obs=FAKE, ring_act=FAKE,
          ring_rew=FAKE, ring_obs2=FAKE, ring_done=FAKE, done_out=FAKE)
REFUSALS = [
    # (cfg, what differs from OK, the text of the refusal)
    (lambda: ops.make_cfg('InvertedPendulumConti-v0'), {}, 'path-tracking env only'),
    (lambda: ops.make_cfg('InvertedDoublePendulum-v2'), {}, 'MuJoCo'),
    (lambda: _with(_cfg(), obs_dim=5), {}, 'obs_dim 6 .. 16'),
    (lambda: _with(_cfg(), obs_dim=17), {}, 'obs_dim 6 .. 16'),
    (lambda: _with(_cfg(), act_dim=1), {}, 'act_dim 2 only'),
    (lambda: ops.make_cfg('PathTracking-v0', policy_out_activation='tanh', action_range=1.0), {}, 'tanh policy with an action range'),
] + [(_cfg, {k: NULL}, 'null pointer') for k in ('policy', 'state', 'obs_io', 'act_out', 'ring_obs', 'ring_act', 'ring_rew', 'ring_obs2',
                                                  'ring_done')] + [
    (_cfg, dict(n=0), 'bad ring'),
    (_cfg, dict(n=8, iters=1, capacity=7), 'bad ring'),
    (_cfg, dict(next_idx=-1), 'bad ring'),
    (_cfg, dict(next_idx=512), 'bad ring'),
    (_cfg, dict(iters=0), 'iters >= 1'),
    (_cfg, dict(iters=-3), 'iters >= 1'),
    (_cfg, dict(iters=1025, capacity=1 << 20), 'iters <= 1024'),
    (_cfg, dict(iters=64, capacity=511), 'do not fit the ring'),
    (_cfg, dict(n=1 << 22, iters=1024, capacity=(1 << 31) - 1), 'do not fit the ring'),     # iters * n = 2^32: no 32-bit product
]


def _call(lib, cfg_ref, a):
    return lib.mpg_worker_rollout(cfg_ref, a['policy'], I(a['n']), I(a['iters']), a['state'], a['obs_io'], F(0.1), U64(1), U64(0), a['act_out'],
                                  I(a['capacity']), I(a['next_idx']), a['ring_obs'], a['ring_act'], a['ring_rew'], a['ring_obs2'],
                                  a['ring_done'], U64(2), U64(0), a['done_out'], NULL)


test_refusals = H.refusal_test('mpg_worker_rollout', REFUSALS, OK, _call)


@pytest.mark.parametrize('engine', ENGINES)
def test_refuses_a_null_configuration(engine):
    H.null_configuration_refused(engine, 'mpg_worker_rollout', _call, OK)


def test_every_refusal_has_a_text_of_its_own():
    H.refusal_texts_are_unique('mpg_worker_rollout', 'env_path_tracking.hip', 11)


def test_python_refuses_a_stochastic_policy_and_another_env():
    """OffPolicyWorker._sample_one_launch raises ValueError with a text of its own before it touches the device"""
    import types
    from mpg_amd.worker import OffPolicyWorker
    w = OffPolicyWorker.__new__(OffPolicyWorker)
    w.num_agent, w.device = 8, 'cpu'
    w.policy_with_value = types.SimpleNamespace(deterministic_policy=False)
    w.env = types.SimpleNamespace(kind=0)
    with pytest.raises(ValueError, match='deterministic policy only'):
        w._sample_one_launch(4)
    w.policy_with_value = types.SimpleNamespace(deterministic_policy=True)
    w.env = types.SimpleNamespace(kind=1)
    with pytest.raises(ValueError, match='PathTracking-v0 only'):
        w._sample_one_launch(4)
