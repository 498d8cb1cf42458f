"""The native AMPC step (learner_version 8 of mpg_step_workspace_bytes / mpg_step_begin / mpg_step_end) at the drop-in boundary, without
a GPU, both libraries: the workspace query answers for version 8 (ws0 = 0, ws1 = mpg_ampc_pg's), every refusal comes back under the
caller's name with a text of its own BEFORE anything is enqueued or counted (every pointer is FAKE: a launch would fault), the ABI
version is unchanged, and the optimizer's native_ampc=True refuses what the driver does not serve."""
import ctypes
import types

import pytest

from mpg_amd import _lib as L
from mpg_amd import ops

NULL, FAKE = ctypes.c_void_p(0), ctypes.c_void_p(0x1000)
I, SZ = ctypes.c_int, ctypes.c_size_t
MPG_EINVAL, MPG_EWORKSPACE = -1000, -1001
PD, DP = 'InvertedPendulumConti-v0', 'InvertedDoublePendulum-v2'
# what version 8 reads (include/mpg_hip.h): the networks, the gradient buffer, the rollout's workspace, the worker's buffers, the ring,
# the minibatch
POINTERS = ('params', 'targets', 'grad', 'ws1', 'env_state', 'w_obs', 'w_act', 'w_done', 'ring_obs', 'ring_act', 'ring_rew', 'ring_obs2',
            'ring_done', 'idx', 'b_obs', 'b_act', 'b_rew', 'b_obs2', 'b_done')
COUNTERS = ('noise_ctr', 'env_ctr', 'replay_times', 'learner_counter', 'ring_next', 'ring_size')


@pytest.fixture(scope='module')
def built():
    from mpg_amd import build as B
    return B.build(verbose=False)


@pytest.fixture(params=sorted(L.ENGINES))
def engine(request, built):
    """both builds of the library (mpg_amd/_lib.py ENGINES)"""
    with L.engine(request.param):
        yield request.param


def _cfg(env='PathTracking-v0', obs_dim=6):
    if env != 'PathTracking-v0':
        return ops.make_cfg(env)
    return ops.make_cfg(env, obs_dim=obs_dim, obs_scale=[1.] * obs_dim, policy_out_activation='tanh')


def _ctx(lib, cfg=None, version=8, batch=256, M=1, n=25):
    """a complete version 8 context on FAKE pointers - WITHOUT ws0 (null, zero bytes: the version has no critic) - and counters that
    a step would move"""
    from mpg_amd.fused import TrainCtx
    c = TrainCtx()
    c.cfg = cfg if cfg is not None else _cfg()
    c.learner_version = version
    c.batch, c.n, c.M, c.n_select = batch, n, M, 1
    c.num_agent, c.sample_iters, c.sampling_interval, c.num_batch_reuse, c.world_size, c.ring_capacity = 8, 64, 10, 1, 1, 4096
    for k in POINTERS:
        setattr(c, k, FAKE.value)
    c.ws0, c.ws0_bytes = None, 0
    need = lib.mpg_ampc_pg_workspace_bytes(ctypes.byref(c.cfg), I(batch), I(M), I(n))
    c.ws1_bytes = need if need else 1 << 40
    c.noise_ctr, c.env_ctr, c.replay_times, c.learner_counter, c.ring_next, c.ring_size = 11, 12, 13, 14, 40, 400
    c.opt_steps[0] = 15
    return c


def counters(c):
    return tuple(int(getattr(c, k)) for k in COUNTERS) + (int(c.opt_steps[0]),)


def refused(lib, c, text, rc=MPG_EINVAL, name='mpg_step_begin', iteration=0):
    """the call is refused under its name with `text`, and no counter moved"""
    before = counters(c)
    if name == 'mpg_step_begin':
        got = lib.mpg_step_begin(ctypes.byref(c), I(iteration), NULL)
    else:
        w0, w1 = SZ(7), SZ(7)
        got = lib.mpg_step_workspace_bytes(ctypes.byref(c), ctypes.byref(w0), ctypes.byref(w1))
    msg = lib.mpg_last_error().decode()
    assert got == rc, (name, got, msg)
    assert msg.startswith(name + ':') and text in msg, msg
    assert counters(c) == before, (msg, before, counters(c))
    return msg


# ---- the workspace query -------------------------------------------------------------------------------------------------------------
CFGS = [('pt-6', lambda: _cfg(obs_dim=6)), ('pt-9', lambda: _cfg(obs_dim=9)), ('pt-16', lambda: _cfg(obs_dim=16)), ('pendulum', lambda: _cfg(PD))]


@pytest.mark.parametrize('shape', [(256, 1, 25), (24, 2, 10)], ids=['256x1-n25', '24x2-n10'])
@pytest.mark.parametrize('case', range(len(CFGS)), ids=[c[0] for c in CFGS])
def test_step_workspace_answers_for_version_8(engine, case, shape):
    lib = L.lib()
    assert lib.mpg_abi_version() == 10           # one more accepted value of an int: no symbol, no field, no layout changed
    batch, M, n = shape
    c = _ctx(lib, CFGS[case][1](), batch=batch, M=M, n=n)
    w0, w1 = SZ(7), SZ(7)
    assert lib.mpg_step_workspace_bytes(ctypes.byref(c), ctypes.byref(w0), ctypes.byref(w1)) == 0, lib.mpg_last_error().decode()
    assert w0.value == 0
    assert w1.value == lib.mpg_ampc_pg_workspace_bytes(ctypes.byref(c.cfg), I(batch), I(M), I(n)) > 0
    for v in (6, 9):                             # not assigned: refused as before
        c.learner_version = v
        refused(lib, c, 'unknown learner_version %d' % v, name='mpg_step_workspace_bytes')


def _wide():
    c = _cfg()
    c.obs_dim = 17
    return c


# (what, context arguments, the words that tell the refusal from the others)
SHAPE_REFUSALS = [('n-0', dict(n=0), '0 < n < 32 (got 0)'), ('n-32', dict(n=32), '0 < n < 32 (got 32)'),
                  ('batch-24-M-1', dict(batch=24), 'batch*M % 16 == 0 (got 24)'), ('M-0', dict(M=0), 'M must be positive (got 0)'),
                  ('obs_dim-17', dict(cfg=_wide), 'unsupported cfg')]


@pytest.mark.parametrize('name', ['mpg_step_workspace_bytes', 'mpg_step_begin'])
@pytest.mark.parametrize('case', range(len(SHAPE_REFUSALS)), ids=[c[0] for c in SHAPE_REFUSALS])
def test_what_mpg_ampc_pg_would_refuse_is_refused_up_front(engine, case, name):
    lib = L.lib()
    _, kw, text = SHAPE_REFUSALS[case]
    kw = {k: (v() if callable(v) else v) for k, v in kw.items()}
    msg = refused(lib, _ctx(lib, **kw), text, name=name)
    assert 'learner_version 8' in msg


# ---- mpg_step_begin ------------------------------------------------------------------------------------------------------------------
def test_step_begin_refuses_reuse_priorities_and_the_mujoco_env(engine):
    lib = L.lib()
    c = _ctx(lib)
    c.num_batch_reuse = 2
    refused(lib, c, 'num_batch_reuse must be 1 (got 2)')
    c = _ctx(lib)
    c.prioritized = 1
    refused(lib, c, 'prioritized replay buffer is not served')
    c = _ctx(lib, _cfg(DP), batch=48, n=10)
    assert c.ws1_bytes < 1 << 40                 # mpg_ampc_pg itself serves this MODEL: the refusal is the driver's, for the real env
    refused(lib, c, 'MuJoCo')
    for k in ('num_agent', 'batch', 'sampling_interval', 'ring_capacity', 'world_size'):
        c = _ctx(lib)
        setattr(c, k, 0)
        refused(lib, c, 'incomplete context')
    for v in (6, 9, 0):                          # ctx_ok keeps refusing what is not assigned
        refused(lib, _ctx(lib, version=v), 'incomplete context')
    with pytest.raises(L.MpgError, match='mpg_step_begin'):
        c = _ctx(lib, n=32)
        L.check(lib.mpg_step_begin(ctypes.byref(c), I(0), NULL), 'mpg_step_begin')


@pytest.mark.parametrize('pointer', POINTERS)
def test_step_begin_names_the_missing_pointer(engine, pointer):
    lib = L.lib()
    c = _ctx(lib)
    setattr(c, pointer, None)
    msg = refused(lib, c, 'null pointer: %s' % pointer)
    assert msg.endswith(pointer)                 # (ring_obs is not taken for ring_obs2)


def test_step_begin_workspace_too_small(engine):
    lib = L.lib()
    c = _ctx(lib)
    need = int(c.ws1_bytes)
    c.ws1_bytes = need - 1
    refused(lib, c, '%d < %d' % (need - 1, need), rc=MPG_EWORKSPACE)


def test_a_null_ws0_is_not_refused(engine):
    """every refusal above was made on a context whose ws0 is null with zero bytes.  Here the same context passes ALL of them: with an
    empty ring on an iteration that does not sample, the first thing left to object to is the ring - still before anything is enqueued
    or counted"""
    lib = L.lib()
    c = _ctx(lib)
    assert not c.ws0 and c.ws0_bytes == 0
    c.ring_size = 0
    refused(lib, c, 'empty replay ring', iteration=1)


def test_step_end_and_the_sac_entry_points(engine):
    lib = L.lib()
    c = _ctx(lib)                                # norms, nonfinite, adam_m, adam_v, clip_scratch are null
    before = counters(c)
    assert lib.mpg_step_end(ctypes.byref(c), I(0), NULL) == MPG_EINVAL
    assert lib.mpg_last_error().decode().startswith('mpg_step_end: incomplete context') and counters(c) == before
    assert lib.mpg_sac_step_begin(ctypes.byref(c), ctypes.c_float(0.03), I(0), NULL) == MPG_EINVAL
    assert 'learner_version 7 (SAC) only (got 8)' in lib.mpg_last_error().decode() and counters(c) == before


# ---- the optimizer's keyword: an explicit request never falls back silently (raised before anything is sampled) -----------------------
def _bare(cls, **attrs):
    """an instance without its constructor: the refusal looks at types and at the learner's n, M and batch_size only"""
    x = object.__new__(cls)
    for k, v in attrs.items():
        setattr(x, k, v)
    return x


def test_native_ampc_refuses_what_the_driver_does_not_serve():
    from mpg_amd.buffer import PrioritizedReplayBuffer, ReplayBuffer
    from mpg_amd.learners import AMPCLearner, TD3Learner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer as Opt
    worker = types.SimpleNamespace(explore_sigma=None)
    normal, priority = types.SimpleNamespace(buffer_type='normal'), types.SimpleNamespace(buffer_type='priority')
    ampc = lambda n=25, M=1, B=256: _bare(AMPCLearner, n=n, M=M, batch_size=B)
    with pytest.raises(ValueError, match='^native_ampc=True: .*TD3Learner'):
        Opt(worker, _bare(TD3Learner), _bare(ReplayBuffer), None, normal, native_ampc=True)
    with pytest.raises(ValueError, match='^native_ampc=True: .*prioritized'):
        Opt(worker, ampc(), _bare(PrioritizedReplayBuffer), None, priority, native_ampc=True)
    with pytest.raises(ValueError, match='^native_ampc=True: .*prioritized'):
        Opt(worker, ampc(), _bare(ReplayBuffer), None, priority, native_ampc=True)
    with pytest.raises(ValueError, match='^native_ampc=True: .*n = 32'):
        Opt(worker, ampc(n=32), _bare(ReplayBuffer), None, normal, native_ampc=True)
    with pytest.raises(ValueError, match='^native_ampc=True: .*n = 0'):
        Opt(worker, ampc(n=0), _bare(ReplayBuffer), None, normal, native_ampc=True)
    with pytest.raises(ValueError, match='^native_ampc=True: .*= 24 is not a multiple of 16'):
        Opt(worker, ampc(B=24), _bare(ReplayBuffer), None, normal, native_ampc=True)
    with pytest.raises(ValueError, match='^native_ampc=True: .*= 24 is not a multiple of 16'):
        Opt(worker, ampc(B=8, M=3), _bare(ReplayBuffer), None, normal, native_ampc=True)
    with pytest.raises(ValueError, match='^native_ampc=True: .*both set'):
        Opt(worker, ampc(), _bare(ReplayBuffer), None, normal, native_sac=True, native_ampc=True)
