"""The native SAC step (mpg_sac_step_begin, learner_version 7) and the one-launch stochastic worker step (mpg_worker_sample_step) at the
drop-in boundary, without a GPU: both libraries export them, the ABI version is unchanged, every refusal comes back as MPG_EINVAL with
the entry point's name before any launch (every pointer is FAKE: a launch would fault), the workspace query answers for version 7, and
the optimizer's native_sac=True refuses what the driver does not serve."""
import ctypes
import types

import pytest

from mpg_amd import _lib as L
from mpg_amd import ops

NULL, FAKE = ctypes.c_void_p(0), ctypes.c_void_p(0x1000)
I, F, SZ, U64 = ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_uint64
MPG_EINVAL = -1000
NEW = ('mpg_worker_sample_step', 'mpg_sac_step_begin')
ENGINES = sorted(L.ENGINES)


@pytest.fixture(scope='module')
def built():
    from mpg_amd import build as B
    return B.build(verbose=False)


@pytest.mark.parametrize('engine', ENGINES)
def test_both_libraries_export_the_two_symbols(built, engine):
    assert set(NEW) <= set(L.declared_symbols())
    lib = ctypes.CDLL(L.ENGINES[engine])
    assert not [n for n in NEW if not hasattr(lib, n)]
    assert lib.mpg_abi_version() == 10           # two functions and one accepted value of an int were added: no layout changed


def _cfg(obs_dim=6, **kw):
    c = ops.make_cfg('PathTracking-v0', obs_dim=obs_dim, policy_out_activation='linear')
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def refused(lib, name, rc, text):
    msg = lib.mpg_last_error().decode()
    assert rc == MPG_EINVAL, (name, rc, msg)
    assert msg.startswith(name + ':') and text in msg, msg


# ---- mpg_worker_sample_step ------------------------------------------------------------------------------------------------------
W_POINTERS = ('policy', 'state', 'obs_io', 'act_out', 'ring_obs', 'ring_act', 'ring_rew', 'ring_obs2', 'ring_done')


def worker_call(lib, cfg_ref, n=8, capacity=64, next_idx=60, logp=FAKE, done=FAKE, **null):
    p = {k: (NULL if null.get(k) else FAKE) for k in W_POINTERS}
    return lib.mpg_worker_sample_step(cfg_ref, p['policy'], I(n), p['state'], p['obs_io'], U64(1), U64(2), p['act_out'], logp, I(capacity),
                                      I(next_idx), p['ring_obs'], p['ring_act'], p['ring_rew'], p['ring_obs2'], p['ring_done'], U64(3), U64(4),
                                      done, NULL)


@pytest.mark.parametrize('engine', ENGINES)
def test_worker_sample_step_null_pointers_and_n(engine):
    name = 'mpg_worker_sample_step'
    with L.engine(engine):
        lib = L.lib()
        cfg = _cfg()
        for k in W_POINTERS:
            refused(lib, name, worker_call(lib, ctypes.byref(cfg), **{k: True}), 'null pointer')
        refused(lib, name, worker_call(lib, NULL), 'null pointer')
        for n in (0, -3):
            refused(lib, name, worker_call(lib, ctypes.byref(cfg), n=n), 'rows')
        with pytest.raises(L.MpgError, match=name):
            L.check(worker_call(lib, ctypes.byref(cfg), n=0), name)


def _with_obs(n):
    c = _cfg()
    c.obs_dim = n
    return c


HEAD = 'Gaussian head without an action range only'
W_CFG_REFUSALS = [('pendulum', lambda: ops.make_cfg('InvertedPendulumConti-v0'), HEAD),
                  ('double-pendulum', lambda: ops.make_cfg('InvertedDoublePendulum-v2'), 'MuJoCo'),
                  ('act_dim-1', lambda: _cfg(act_dim=1), HEAD),
                  ('env_kind-1', lambda: _cfg(env_kind=1), HEAD),
                  ('action_range', lambda: _cfg(action_range=1.0), HEAD),
                  ('obs_dim-17', lambda: _with_obs(17), 'observation width'),
                  ('obs_dim-5', lambda: _with_obs(5), 'observation width')]


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('case', range(len(W_CFG_REFUSALS)), ids=[c[0] for c in W_CFG_REFUSALS])
def test_worker_sample_step_configurations_refused(engine, case):
    _, make, text = W_CFG_REFUSALS[case]
    with L.engine(engine):
        lib = L.lib()
        cfg = make()
        refused(lib, 'mpg_worker_sample_step', worker_call(lib, ctypes.byref(cfg)), text)


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('ring', [dict(capacity=7), dict(capacity=0), dict(next_idx=-1), dict(next_idx=64), dict(next_idx=1000)],
                         ids=['capacity-below-n', 'capacity-0', 'next-negative', 'next-at-capacity', 'next-beyond'])
def test_worker_sample_step_ring_refused(engine, ring):
    """the ring checks of mpg_worker_step: capacity >= n, 0 <= next_idx < capacity"""
    with L.engine(engine):
        lib = L.lib()
        cfg = _cfg()
        refused(lib, 'mpg_worker_sample_step', worker_call(lib, ctypes.byref(cfg), **ring), 'ring')


# ---- the driver --------------------------------------------------------------------------------------------------------------------
def _ctx(version=7, complete=True):
    from mpg_amd.fused import TrainCtx
    c = TrainCtx()
    c.cfg = _cfg()
    c.learner_version = version
    c.batch, c.n, c.M, c.n_select = 256, 1, 1, 1
    if complete:
        c.num_agent, c.sample_iters, c.sampling_interval, c.num_batch_reuse, c.world_size, c.ring_capacity = 8, 64, 10, 1, 1, 4096
        for k in ('params', 'targets', 'grad', 'ws0', 'ws1', 'scratch'):
            setattr(c, k, FAKE.value)
    return c


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('obs_dim', [6, 9, 16])
def test_step_workspace_answers_for_version_7(engine, obs_dim):
    with L.engine(engine):
        lib = L.lib()
        c = _ctx(complete=False)
        c.cfg = _cfg(obs_dim=obs_dim)
        cfg = ctypes.byref(c.cfg)
        w0, w1 = SZ(0), SZ(0)
        assert lib.mpg_step_workspace_bytes(ctypes.byref(c), ctypes.byref(w0), ctypes.byref(w1)) == 0
        assert w0.value == max(lib.mpg_sac_targets_workspace_bytes(cfg, I(256)), lib.mpg_q_loss_grad_workspace_bytes(cfg, I(256))) > 0
        assert w1.value == lib.mpg_sac_policy_grad_workspace_bytes(cfg, I(256)) > 0
        c.learner_version = 6                    # not assigned: refused as before
        assert lib.mpg_step_workspace_bytes(ctypes.byref(c), ctypes.byref(w0), ctypes.byref(w1)) == MPG_EINVAL
        assert 'mpg_step_workspace_bytes' in lib.mpg_last_error().decode()
        c.learner_version = 7
        c.cfg.action_range = 1.0                 # what the Gaussian-head queries refuse, the step's query refuses
        assert lib.mpg_step_workspace_bytes(ctypes.byref(c), ctypes.byref(w0), ctypes.byref(w1)) == MPG_EINVAL


@pytest.mark.parametrize('engine', ENGINES)
def test_step_begin_names_the_sac_entry_point(engine):
    with L.engine(engine):
        lib = L.lib()
        for complete in (True, False):
            c = _ctx(complete=complete)
            refused(lib, 'mpg_step_begin', lib.mpg_step_begin(ctypes.byref(c), I(0), NULL), 'mpg_sac_step_begin')
        c = _ctx(version=6)
        assert lib.mpg_step_begin(ctypes.byref(c), I(0), NULL) == MPG_EINVAL
        assert 'mpg_sac_step_begin' not in lib.mpg_last_error().decode()


@pytest.mark.parametrize('engine', ENGINES)
def test_sac_step_begin_refusals(engine):
    name = 'mpg_sac_step_begin'
    with L.engine(engine):
        lib = L.lib()
        begin = lambda c, alpha=0.03: lib.mpg_sac_step_begin(ctypes.byref(c), F(alpha), I(0), NULL)
        refused(lib, name, lib.mpg_sac_step_begin(NULL, F(0.03), I(0), NULL), 'null context')
        for v in (1, 2, 3, 4, 5, 6, 8, 0, -1):
            refused(lib, name, begin(_ctx(version=v)), 'learner_version 7')
        refused(lib, name, begin(_ctx(complete=False)), 'incomplete context')
        for k in ('params', 'targets', 'grad', 'ws0', 'ws1', 'scratch'):
            c = _ctx()
            setattr(c, k, None)
            refused(lib, name, begin(c), 'incomplete context')
        for k in ('num_agent', 'batch', 'sampling_interval', 'num_batch_reuse', 'ring_capacity', 'world_size'):
            c = _ctx()
            setattr(c, k, 0)
            refused(lib, name, begin(c), 'incomplete context')
        c = _ctx()
        c.prioritized = 1
        refused(lib, name, begin(c), 'prioritized')
        c = _ctx()
        c.explore_sigma = 0.1
        refused(lib, name, begin(c), 'explore_sigma')
        for alpha in (-0.03, float('inf'), float('nan')):
            refused(lib, name, begin(_ctx(), alpha), 'alpha')
        c = _ctx()
        c.cfg = ops.make_cfg('InvertedDoublePendulum-v2')
        refused(lib, name, begin(c), 'MuJoCo')
        with pytest.raises(L.MpgError, match=name):
            L.check(begin(_ctx(version=4)), name)


# ---- the optimizer's keyword: an explicit request never falls back silently (raised before anything is sampled) -----------------------
def _bare(cls):
    """an instance without its constructor: the refusal looks at types and at worker.explore_sigma only"""
    return object.__new__(cls)


def test_native_sac_refuses_what_the_driver_does_not_serve():
    from mpg_amd.buffer import PrioritizedReplayBuffer, ReplayBuffer
    from mpg_amd.learners import SACLearner, TD3Learner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer as Opt
    worker = types.SimpleNamespace(explore_sigma=None)
    normal, priority = types.SimpleNamespace(buffer_type='normal'), types.SimpleNamespace(buffer_type='priority')
    with pytest.raises(ValueError, match='native_sac=True.*TD3Learner'):
        Opt(worker, _bare(TD3Learner), _bare(ReplayBuffer), None, normal, native_sac=True)
    with pytest.raises(ValueError, match='native_sac=True.*prioritized'):
        Opt(worker, _bare(SACLearner), _bare(PrioritizedReplayBuffer), None, priority, native_sac=True)
    with pytest.raises(ValueError, match='native_sac=True.*prioritized'):
        Opt(worker, _bare(SACLearner), _bare(ReplayBuffer), None, priority, native_sac=True)
    with pytest.raises(ValueError, match='native_sac=True.*explore_sigma'):
        Opt(types.SimpleNamespace(explore_sigma=0.1), _bare(SACLearner), _bare(ReplayBuffer), None, normal, native_sac=True)
