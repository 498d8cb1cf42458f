"""mpg_worker_sample_rollout_pendulum at the drop-in boundary, without a GPU: both libraries export it with the declared argument types,
and every refusal comes back as MPG_EINVAL with a text of its own before any launch (every pointer is FAKE: a launch would fault)."""
import ctypes
import re

import pytest

from mpg_amd import _lib as L
from mpg_amd import ops
from tests import abi_harness as H
from tests.abi_harness import ENGINES, F, FAKE, I, NULL, U64, MPG_EINVAL, _with, built  # noqa: F401 (built: the module's autouse fixture)

NAME = 'mpg_worker_sample_rollout_pendulum'
PEND = 'InvertedPendulumConti-v0'


@pytest.mark.parametrize('engine', ENGINES)
def test_both_libraries_export_the_entry_point(engine):
    assert NAME in L.declared_symbols()
    lib = ctypes.CDLL(L.ENGINES[engine])
    assert hasattr(lib, NAME)
    assert lib.mpg_abi_version() == 10           # a function was added: no layout or signature changed
    assert L.declared_return_types()[NAME] == 'int'


def test_declared_argument_types():
    """the declaration of include/mpg_hip.h, argument by argument: mpg_worker_rollout_pendulum's without explore_sigma, the draw's key
    and counter in the place of the exploration noise's"""
    src = re.sub(r'/\*.*?\*/', '', open(L.HEADER).read(), flags=re.S)
    args = {}
    for name in (NAME, 'mpg_worker_rollout_pendulum'):
        m = re.search(r'\bint\s+%s\s*\((.*?)\)\s*;' % name, src, flags=re.S)
        assert m, name
        args[name] = [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')]
    assert args[NAME] == ['const mpg_cfg_t* cfg', 'const float* policy_params', 'int n', 'int iters', 'float* state', 'float* obs_io',
                          'uint64_t sample_seed', 'uint64_t sample_ctr', 'float* act_out', 'int capacity', 'int next_idx',
                          'float* ring_obs', 'float* ring_act', 'float* ring_rew', 'float* ring_obs2', 'uint8_t* ring_done',
                          'uint64_t env_seed', 'uint64_t env_ctr', 'uint8_t* done_out', 'mpg_stream_t stream']
    sibling = [a.replace('noise_', 'sample_') for a in args['mpg_worker_rollout_pendulum'] if a != 'float explore_sigma']
    assert args[NAME] == sibling


def _cfg():
    """the pendulum under an action range over a linear output: what the squashed head is built for (make_cfg's default range: 3)"""
    c = ops.make_cfg(PEND)
    assert c.env_kind == 1 and c.action_range == 3.0
    return c


OK = dict(policy=FAKE, n=8, iters=64, state=FAKE, obs_io=FAKE, act_out=FAKE, capacity=512, next_idx=0, ring_obs=FAKE, ring_act=FAKE,
          ring_rew=FAKE, ring_obs2=FAKE, ring_done=FAKE, done_out=FAKE)
REFUSALS = [
    # (cfg, what differs from OK, the text of the refusal)
    (lambda: ops.make_cfg('InvertedDoublePendulum-v2'), {}, 'MuJoCo'),
    (lambda: ops.make_cfg('PathTracking-v0'), {}, 'pendulum env only'),
    (lambda: _with(ops.make_cfg('PathTracking-v0'), action_range=1.5), {}, 'pendulum env only'),     # the head serves it, the launch does not
    (lambda: _with(_cfg(), env_kind=3), {}, 'pendulum env only'),
    (lambda: _with(_cfg(), act_dim=2), {}, 'the inverted pendulum (act_dim 1) only'),
    (lambda: _with(_cfg(), action_range=0.0), {}, 'positive, finite action range'),
    (lambda: _with(_cfg(), action_range=-3.0), {}, 'positive, finite action range'),
    (lambda: _with(_cfg(), action_range=float('inf')), {}, 'positive, finite action range'),
    (lambda: _with(_cfg(), action_range=float('nan')), {}, 'positive, finite action range'),
    (lambda: ops.make_cfg(PEND, policy_out_activation='tanh', action_range=3.0), {}, 'tanh output activation under an action range'),
    (lambda: _with(_cfg(), obs_dim=6), {}, 'unsupported observation width 6'),
    (lambda: _with(_cfg(), obs_dim=3), {}, 'unsupported observation width 3'),
] + [(_cfg, {k: NULL}, 'null pointer') for k in ('policy', 'state', 'obs_io', 'act_out', 'ring_obs', 'ring_act', 'ring_rew', 'ring_obs2',
                                                  'ring_done')] + [
    (_cfg, dict(n=0), 'bad ring'),
    (_cfg, dict(n=-4), 'bad ring'),
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
    return getattr(lib, NAME)(cfg_ref, a['policy'], I(a['n']), I(a['iters']), a['state'], a['obs_io'], U64(1), U64(0), a['act_out'],
                              I(a['capacity']), I(a['next_idx']), a['ring_obs'], a['ring_act'], a['ring_rew'], a['ring_obs2'],
                              a['ring_done'], U64(2), U64(0), a['done_out'], NULL)


test_refusals = H.refusal_test(NAME, REFUSALS, OK, _call)


@pytest.mark.parametrize('engine', ENGINES)
def test_refuses_a_null_configuration(engine):
    H.null_configuration_refused(engine, NAME, _call, OK)


@pytest.mark.parametrize('engine', ENGINES)
def test_a_null_done_out_is_no_refusal_of_its_own(engine):
    """done_out is the one nullable pointer: with it null the NEXT refusal in line answers (nothing is launched here either)"""
    with L.engine(engine):
        lib = L.lib()
        cfg = _cfg()
        a = dict(OK, done_out=NULL, iters=0)
        assert _call(lib, ctypes.byref(cfg), a) == MPG_EINVAL
        assert 'iters >= 1' in lib.mpg_last_error().decode()


def test_every_refusal_has_a_text_of_its_own():
    """(the entry point's own texts and those of gauss::squash_refusal, which it calls)"""
    H.refusal_texts_are_unique(NAME, 'env_cart_pole.hip', 8, head_at_least=7)


def test_the_other_entry_points_answer_as_before():
    """a new name, not a widening: mpg_worker_rollout_pendulum is the deterministic policy's (a squashed cfg is a ranged deterministic cfg
    to it: nothing to refuse but the ring), and mpg_worker_sample_step still refuses the pendulum and an action range"""
    lib = L.lib()
    cfg = _cfg()
    rc = lib.mpg_worker_rollout_pendulum(ctypes.byref(cfg), FAKE, I(8), I(0), FAKE, FAKE, F(0.1), U64(1), U64(0), FAKE, I(512), I(0), FAKE,
                                         FAKE, FAKE, FAKE, FAKE, U64(2), U64(0), FAKE, NULL)
    msg = lib.mpg_last_error().decode()
    assert rc == MPG_EINVAL and msg.startswith('mpg_worker_rollout_pendulum:') and 'iters >= 1' in msg, msg
    for c in (cfg, _with(ops.make_cfg('PathTracking-v0'), action_range=1.5)):
        rc = lib.mpg_worker_sample_step(ctypes.byref(c), FAKE, I(8), FAKE, FAKE, U64(1), U64(0), FAKE, FAKE, I(512), I(0), FAKE, FAKE, FAKE,
                                        FAKE, FAKE, U64(2), U64(0), FAKE, NULL)
        msg = lib.mpg_last_error().decode()
        assert rc == MPG_EINVAL and msg.startswith('mpg_worker_sample_step:') and 'Gaussian head without an action range only' in msg, msg


def test_python_refusals():
    """OffPolicyWorker._sample_one_launch_stochastic_pendulum raises ValueError with a text of its own before it touches the device
    (the worker here has no device objects at all), and the two deterministic methods keep their refusals"""
    import types
    from mpg_amd.worker import OffPolicyWorker
    w = OffPolicyWorker.__new__(OffPolicyWorker)
    w.num_agent, w.device, w.explore_sigma = 1, 'cpu', None
    w.env = types.SimpleNamespace(kind=1)
    w.policy_with_value = types.SimpleNamespace(deterministic_policy=False, squashed_head=False)
    with pytest.raises(ValueError, match='tanh-squashed head only'):
        w._sample_one_launch_stochastic_pendulum(4)
    w.policy_with_value = types.SimpleNamespace(deterministic_policy=False, squashed_head=True)
    for sigma in (0.1, 0.0):
        w.explore_sigma = sigma
        with pytest.raises(ValueError, match='takes no explore_sigma'):
            w._sample_one_launch_stochastic_pendulum(4)
    w.explore_sigma = None
    with pytest.raises(ValueError, match='at most 1024 iterations'):
        w._sample_one_launch_stochastic_pendulum(1025)
    w.env = types.SimpleNamespace(kind=0)
    with pytest.raises(ValueError, match='InvertedPendulumConti-v0 only'):
        w._sample_one_launch_stochastic_pendulum(4)
    w.env = types.SimpleNamespace(kind=1)
    w.policy_with_value = types.SimpleNamespace(deterministic_policy=True)
    with pytest.raises(ValueError, match='serves a stochastic policy'):
        w._sample_one_launch_stochastic_pendulum(4)
    # the deterministic policy's methods answer a stochastic policy as they did
    w.policy_with_value = types.SimpleNamespace(deterministic_policy=False, squashed_head=True)
    with pytest.raises(ValueError, match='deterministic policy only'):
        w._sample_one_launch_pendulum(4)
    with pytest.raises(ValueError, match='deterministic policy only'):
        w._sample_one_launch(4)


def test_sample_dispatches_on_the_policy_kind():
    """sample() with one_launch_sample on the pendulum: a stochastic policy goes to the new method, a deterministic one to
    _sample_one_launch_pendulum, and without the switch both stay on the loop"""
    import types
    from mpg_amd.worker import OffPolicyWorker
    took = []

    class Taken(Exception):
        pass

    class W(OffPolicyWorker):
        def _sample_loop(self, iters):
            took.append(('loop', iters))
            raise Taken

        def _sample_one_launch_pendulum(self, iters):
            took.append(('deterministic', iters))
            raise Taken

        def _sample_one_launch_stochastic_pendulum(self, iters):
            took.append(('stochastic', iters))
            raise Taken

    for one in (True, False):
        for det in (True, False):
            w = W.__new__(W)
            w.num_agent, w.batch_size = 8, 64
            w.args = types.SimpleNamespace(one_launch_sample=one)
            w.env = types.SimpleNamespace(kind=1)
            w.policy_with_value = types.SimpleNamespace(deterministic_policy=det)
            with pytest.raises(Taken):
                w.sample()
    assert took == [('deterministic', 8), ('stochastic', 8), ('loop', 8), ('loop', 8)]
