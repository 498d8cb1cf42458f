"""mpg_worker_sample_rollout at the drop-in boundary, without a GPU: both libraries export it with the declared argument types, and every
refusal comes back as MPG_EINVAL with a text of its own before any launch.  Every output pointer is a HOST buffer full of a poison
byte: a launch would fault on it, and a refusal leaves every byte as it was.  The Python side: OffPolicyWorker's refusals and the
dispatch of sample()."""
import ctypes
import re

import pytest

from mpg_amd import _lib as L
from mpg_amd import ops
from tests import abi_harness as H
from tests.abi_harness import ENGINES, F, FAKE, I, NULL, U64, MPG_EINVAL, _with, built  # noqa: F401 (built: the module's autouse fixture)

NAME = 'mpg_worker_sample_rollout'
POISON, NBYTES = 0xA5, 256
OUTPUTS = ('state', 'obs_io', 'act_out', 'ring_obs', 'ring_act', 'ring_rew', 'ring_obs2', 'ring_done', 'done_out')


@pytest.mark.parametrize('engine', ENGINES)
def test_both_libraries_export_the_entry_point(engine):
    assert NAME in L.declared_symbols()
    lib = ctypes.CDLL(L.ENGINES[engine])
    assert hasattr(lib, NAME)
    assert lib.mpg_abi_version() == 10           # a function was added: no layout or signature changed
    assert L.declared_return_types()[NAME] == 'int'


def test_declared_argument_types():
    """the declaration of include/mpg_hip.h, argument by argument: mpg_worker_rollout's without explore_sigma, the draw's key and counter
    in the place of the exploration noise's - which is mpg_worker_sample_rollout_pendulum's list"""
    src = re.sub(r'/\*.*?\*/', '', open(L.HEADER).read(), flags=re.S)
    args = {}
    for name in (NAME, 'mpg_worker_rollout', 'mpg_worker_sample_rollout_pendulum'):
        m = re.search(r'\bint\s+%s\s*\((.*?)\)\s*;' % name, src, flags=re.S)
        assert m, name
        args[name] = [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')]
    assert args[NAME] == ['const mpg_cfg_t* cfg', 'const float* policy_params', 'int n', 'int iters', 'float* state', 'float* obs_io',
                          'uint64_t sample_seed', 'uint64_t sample_ctr', 'float* act_out', 'int capacity', 'int next_idx',
                          'float* ring_obs', 'float* ring_act', 'float* ring_rew', 'float* ring_obs2', 'uint8_t* ring_done',
                          'uint64_t env_seed', 'uint64_t env_ctr', 'uint8_t* done_out', 'mpg_stream_t stream']
    assert args[NAME] == [a.replace('noise_', 'sample_') for a in args['mpg_worker_rollout'] if a != 'float explore_sigma']
    assert args[NAME] == args['mpg_worker_sample_rollout_pendulum']


def _cfg(obs_dim=6, **kw):
    """PathTracking under the Gaussian head; with action_range (and the linear output it asks for) the squashed one"""
    return ops.make_cfg('PathTracking-v0', obs_dim=obs_dim, **kw)


def _squashed(**kw):
    return _cfg(policy_out_activation='linear', action_range=1.5, **kw)


OK = dict(policy=FAKE, n=8, iters=64, capacity=512, next_idx=0)
REFUSALS = [
    # (cfg, what differs from OK, the text of the refusal)
    (lambda: ops.make_cfg('InvertedDoublePendulum-v2'), {}, 'MuJoCo'),
    (lambda: ops.make_cfg('InvertedPendulumConti-v0'), {}, 'path-tracking env only'),      # (its launch: ..._rollout_pendulum)
    (lambda: _with(_cfg(), env_kind=3), {}, 'path-tracking env only'),
    (lambda: _with(_cfg(), act_dim=1), {}, 'act_dim 2 only'),
    (lambda: _with(_squashed(), act_dim=1), {}, 'act_dim 2 only'),
    (lambda: _with(_cfg(), obs_dim=5), {}, 'obs_dim 6 .. 16'),
    (lambda: _with(_cfg(), obs_dim=17), {}, 'obs_dim 6 .. 16'),
    (lambda: _with(_squashed(), obs_dim=17), {}, 'obs_dim 6 .. 16'),
    (lambda: _cfg(policy_out_activation='tanh', action_range=1.5), {}, 'tanh output activation under an action range'),
    (lambda: _with(_squashed(), action_range=float('inf')), {}, 'positive, finite action range'),
] + [(make, {k: NULL}, 'null pointer') for make in (_cfg, _squashed)
     for k in ('policy', 'state', 'obs_io', 'act_out', 'ring_obs', 'ring_act', 'ring_rew', 'ring_obs2', 'ring_done')] + [
    (_cfg, dict(n=0), 'bad ring'),
    (_cfg, dict(n=-4), 'bad ring'),
    (_cfg, dict(n=8, iters=1, capacity=7), 'bad ring'),
    (_cfg, dict(next_idx=-1), 'bad ring'),
    (_squashed, dict(next_idx=512), 'bad ring'),
    (_cfg, dict(iters=0), 'iters >= 1'),
    (_squashed, dict(iters=-3), 'iters >= 1'),
    (_cfg, dict(iters=1025, capacity=1 << 20), 'iters <= 1024'),
    (_squashed, dict(iters=1025, capacity=1 << 20), 'iters <= 1024'),
    (_cfg, dict(iters=64, capacity=511), 'do not fit the ring'),
    (_squashed, dict(iters=64, capacity=511), 'do not fit the ring'),
    (lambda: _cfg(9), dict(n=1 << 22, iters=1024, capacity=(1 << 31) - 1), 'do not fit the ring'),     # iters * n = 2^32: no 32-bit product
]


def _buffers():
    return {k: (ctypes.c_ubyte * NBYTES)(*([POISON] * NBYTES)) for k in OUTPUTS}


def _call(lib, cfg_ref, a, bufs):
    p = {k: (a[k] if k in a else ctypes.cast(bufs[k], ctypes.c_void_p)) for k in OUTPUTS}
    return getattr(lib, NAME)(cfg_ref, a['policy'], I(a['n']), I(a['iters']), p['state'], p['obs_io'], U64(1), U64(0), p['act_out'],
                              I(a['capacity']), I(a['next_idx']), p['ring_obs'], p['ring_act'], p['ring_rew'], p['ring_obs2'],
                              p['ring_done'], U64(2), U64(0), p['done_out'], NULL)


def _untouched(bufs):
    return all(bytes(b) == bytes([POISON]) * NBYTES for b in bufs.values())


def _call_on_poison(lib, cfg_ref, a):
    """_call on fresh poison buffers, which the refusal has left as they were"""
    bufs = _buffers()
    rc = _call(lib, cfg_ref, a, bufs)
    assert _untouched(bufs)
    return rc


test_refusals = H.refusal_test(NAME, REFUSALS, OK, _call_on_poison)


@pytest.mark.parametrize('engine', ENGINES)
def test_refuses_a_null_configuration(engine):
    H.null_configuration_refused(engine, NAME, _call_on_poison, OK)


@pytest.mark.parametrize('engine', ENGINES)
def test_a_range_that_is_no_range_is_the_plain_head(engine):
    """action_range 0, negative or NaN is `no action range` to every entry point of the library (cfg->action_range > 0 decides): such a
    cfg is the Gaussian head's, tanh output included, and the NEXT refusal in line answers (nothing is launched here either).  So does
    a null done_out, the one nullable pointer."""
    with L.engine(engine):
        lib = L.lib()
        for r in (0.0, -1.5, float('nan')):
            cfg = _with(_cfg(), action_range=r)
            bufs = _buffers()
            assert _call(lib, ctypes.byref(cfg), dict(OK, iters=0, done_out=NULL), bufs) == MPG_EINVAL
            assert 'iters >= 1' in lib.mpg_last_error().decode()
            assert _untouched(bufs)


def test_every_refusal_has_a_text_of_its_own():
    """(the entry point's own texts and those of gauss::squash_refusal, which it calls under an action range)"""
    H.refusal_texts_are_unique(NAME, 'env_path_tracking.hip', 10, head_at_least=7)


def test_the_other_entry_points_answer_as_before():
    """a new name, not a widening: mpg_worker_sample_step still refuses an action range, mpg_worker_sample_rollout_pendulum still refuses
    PathTracking (with and without a range), and mpg_worker_rollout is the deterministic policy's as it was"""
    lib = L.lib()
    for c in (_squashed(), _with(_cfg(), action_range=1.5)):
        rc = lib.mpg_worker_sample_step(ctypes.byref(c), FAKE, I(8), FAKE, FAKE, U64(1), U64(0), FAKE, FAKE, I(512), I(0), FAKE, FAKE, FAKE,
                                        FAKE, FAKE, U64(2), U64(0), FAKE, NULL)
        msg = lib.mpg_last_error().decode()
        assert rc == MPG_EINVAL and msg.startswith('mpg_worker_sample_step:') and 'Gaussian head without an action range only' in msg, msg
    for c in (_cfg(), _squashed()):
        rc = lib.mpg_worker_sample_rollout_pendulum(ctypes.byref(c), FAKE, I(8), I(64), FAKE, FAKE, U64(1), U64(0), FAKE, I(512), I(0), FAKE,
                                                    FAKE, FAKE, FAKE, FAKE, U64(2), U64(0), FAKE, NULL)
        msg = lib.mpg_last_error().decode()
        assert rc == MPG_EINVAL and msg.startswith('mpg_worker_sample_rollout_pendulum:') and 'pendulum env only' in msg, msg
    c = _cfg()
    rc = lib.mpg_worker_rollout(ctypes.byref(c), FAKE, I(8), I(0), FAKE, FAKE, F(0.1), U64(1), U64(0), FAKE, I(512), I(0), FAKE, FAKE, FAKE,
                                FAKE, FAKE, U64(2), U64(0), FAKE, NULL)
    msg = lib.mpg_last_error().decode()
    assert rc == MPG_EINVAL and msg.startswith('mpg_worker_rollout:') and 'iters >= 1' in msg, msg
    pend = ops.make_cfg('InvertedPendulumConti-v0')
    rc = lib.mpg_worker_rollout(ctypes.byref(pend), FAKE, I(8), I(64), FAKE, FAKE, F(0.1), U64(1), U64(0), FAKE, I(512), I(0), FAKE, FAKE,
                                FAKE, FAKE, FAKE, U64(2), U64(0), FAKE, NULL)
    msg = lib.mpg_last_error().decode()
    assert rc == MPG_EINVAL and msg.startswith('mpg_worker_rollout:') and 'path-tracking env only' in msg, msg


def test_python_refusals():
    """OffPolicyWorker._sample_one_launch_stochastic raises ValueError with a text of its own before it touches the device (the worker
    here has no device objects at all), and the other methods keep their refusals"""
    import types
    from mpg_amd.worker import OffPolicyWorker
    w = OffPolicyWorker.__new__(OffPolicyWorker)
    w.num_agent, w.device, w.explore_sigma = 8, 'cpu', None
    w.env = types.SimpleNamespace(kind=0)
    w.policy_with_value = types.SimpleNamespace(deterministic_policy=True)
    with pytest.raises(ValueError, match='serves a stochastic policy'):
        w._sample_one_launch_stochastic(4)
    for squashed in (False, True):
        w.policy_with_value = types.SimpleNamespace(deterministic_policy=False, squashed_head=squashed)
        for sigma in (0.1, 0.0):
            w.explore_sigma = sigma
            with pytest.raises(ValueError, match='takes no explore_sigma'):
                w._sample_one_launch_stochastic(4)
        w.explore_sigma = None
        with pytest.raises(ValueError, match='at most 1024 iterations'):
            w._sample_one_launch_stochastic(1025)
        w.env = types.SimpleNamespace(kind=1)
        with pytest.raises(ValueError, match='PathTracking-v0 only'):
            w._sample_one_launch_stochastic(4)
        w.env = types.SimpleNamespace(kind=0)
        # the deterministic policy's method answers a stochastic policy as it did, and so does the pendulum's stochastic one another env
        with pytest.raises(ValueError, match='deterministic policy only'):
            w._sample_one_launch(4)
    with pytest.raises(ValueError, match='InvertedPendulumConti-v0 only'):
        w._sample_one_launch_stochastic_pendulum(4)
    texts = []
    for setup in (dict(det=True), dict(sigma=0.1), dict(kind=1), dict(iters=1025)):
        w.policy_with_value = types.SimpleNamespace(deterministic_policy=setup.get('det', False))
        w.explore_sigma = setup.get('sigma')
        w.env = types.SimpleNamespace(kind=setup.get('kind', 0))
        with pytest.raises(ValueError) as e:
            w._sample_one_launch_stochastic(setup.get('iters', 4))
        texts.append(str(e.value))
    assert len(set(texts)) == 4, texts


def test_sample_dispatches_on_the_switch_the_policy_kind_and_the_env():
    """sample() over (one_launch_sample, deterministic, env.kind): with the switch a stochastic policy on PathTracking goes to the new
    method, every other combination where it went before; without the switch all stay on the loop"""
    import types
    from mpg_amd.worker import OffPolicyWorker
    took = []

    class Taken(Exception):
        pass

    def taker(name):
        def f(self, iters):
            took.append((name, iters))
            raise Taken
        return f

    class W(OffPolicyWorker):
        _sample_loop = taker('loop')
        _sample_one_launch = taker('path-tracking deterministic')
        _sample_one_launch_stochastic = taker('path-tracking stochastic')
        _sample_one_launch_pendulum = taker('pendulum deterministic')
        _sample_one_launch_stochastic_pendulum = taker('pendulum stochastic')

    for one in (True, False):
        for kind in (0, 1):
            for det in (True, False):
                w = W.__new__(W)
                w.num_agent, w.batch_size = 8, 64
                w.args = types.SimpleNamespace(one_launch_sample=one)
                w.env = types.SimpleNamespace(kind=kind)
                w.policy_with_value = types.SimpleNamespace(deterministic_policy=det)
                with pytest.raises(Taken):
                    w.sample()
    assert took == [('path-tracking deterministic', 8), ('path-tracking stochastic', 8), ('pendulum deterministic', 8),
                    ('pendulum stochastic', 8)] + [('loop', 8)] * 4
