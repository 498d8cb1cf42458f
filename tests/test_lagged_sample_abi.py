"""The lagged worker sample (mpg_lagged_sample_t; mpg_step_begin_lagged, mpg_sac_step_begin_lagged, mpg_sac_auto_step_begin_lagged,
mpg_lagged_sample_drain) at the drop-in boundary, without a GPU, both libraries: the symbols are declared and exported, the ABI version and
the context's layout are what they were, every refusal comes back under the entry point's name with a text of its own BEFORE anything is
enqueued or counted (every pointer is FAKE: a launch would fault), and the optimizer's sample_lag keyword refuses at construction."""
import ctypes
import re
import types

import pytest

from mpg_amd import _lib as L
from mpg_amd import ops

NULL, FAKE = ctypes.c_void_p(0), ctypes.c_void_p(0x1000)
I, F = ctypes.c_int, ctypes.c_float
MPG_EINVAL = -1000
DP = 'InvertedDoublePendulum-v2'
BEGINS = ('mpg_step_begin_lagged', 'mpg_sac_step_begin_lagged', 'mpg_sac_auto_step_begin_lagged')
NEW = BEGINS + ('mpg_lagged_sample_drain',)
COUNTERS = ('noise_ctr', 'env_ctr', 'replay_times', 'learner_counter', 'ring_next', 'ring_size')
STAGING = ('s_obs', 's_act', 's_rew', 's_obs2', 's_done')


@pytest.fixture(scope='module')
def built():
    from mpg_amd import build as B
    return B.build(verbose=False)


@pytest.fixture(params=sorted(L.ENGINES))
def engine(request, built):
    """both builds of the library (mpg_amd/_lib.py ENGINES)"""
    with L.engine(request.param):
        yield request.param


# ---- declarations -------------------------------------------------------------------------------------------------------------------
def _declared(name):
    src = re.sub(r'/\*.*?\*/', '', open(L.HEADER).read(), flags=re.S)
    m = re.search(r'\bint\s+%s\s*\((.*?)\)\s*;' % name, src, flags=re.S)
    assert m, name
    return [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')]


def test_symbols_are_declared_and_exported(engine):
    assert set(NEW) <= set(L.declared_symbols())
    lib = ctypes.CDLL(L.ENGINES[engine])
    assert not [n for n in NEW if not hasattr(lib, n)]
    assert all(L.declared_return_types()[n] == 'int' for n in NEW)
    assert lib.mpg_abi_version() == 10           # four functions and one caller-owned struct were added: no layout or signature changed


def test_declared_argument_types_and_layouts():
    """each lagged begin is its plain begin with the object ahead of the iteration; the context's mirror has the size it had (768 bytes:
    measured on the commit before this struct existed) and the object's mirror follows the header field by field"""
    from mpg_amd.fused import LaggedSample, TrainCtx
    g = 'mpg_lagged_sample_t* lagged'
    for name, plain in zip(BEGINS, ('mpg_step_begin', 'mpg_sac_step_begin', 'mpg_sac_auto_step_begin')):
        args = _declared(plain)
        assert _declared(name) == args[:-2] + [g] + args[-2:], name
    assert _declared('mpg_lagged_sample_drain') == ['mpg_train_ctx_t* ctx', g, 'mpg_stream_t stream']
    assert ctypes.sizeof(TrainCtx) == 768
    assert [f[0] for f in LaggedSample._fields_] == ['lag', 'side', 'forked', 'done', 'policy'] + list(STAGING) + ['pending', 'due']
    assert ctypes.sizeof(LaggedSample) == 8 + 9 * 8 + 8
    hdr = re.sub(r'/\*.*?\*/', '', open(L.HEADER).read(), flags=re.S)
    body = re.search(r'typedef struct \{([^}]*)\} mpg_lagged_sample_t;', hdr).group(1)
    assert re.findall(r'[*\s](\w+)\s*[,;]', body) == [f[0] for f in LaggedSample._fields_]


# ---- contexts on FAKE pointers ------------------------------------------------------------------------------------------------------
def _ctx(version, env='PathTracking-v0'):
    """a complete context of `version` (4: TD3, 7: SAC, 8: AMPC) whose every pointer is FAKE, with counters that a step would move"""
    from mpg_amd.fused import TrainCtx
    c = TrainCtx()
    act = 'linear' if version == 7 else 'tanh'
    c.cfg = ops.make_cfg(env) if env != 'PathTracking-v0' else ops.make_cfg(env, obs_dim=6, obs_scale=[1.] * 6, policy_out_activation=act)
    c.learner_version = version
    c.batch, c.n, c.M, c.n_select = 256, 25, 1, 1
    c.num_agent, c.sample_iters, c.sampling_interval, c.num_batch_reuse, c.world_size, c.ring_capacity = 8, 64, 10, 1, 1, 4096
    c.delay_update = 2
    for name, kind in type(c)._fields_:
        if kind is ctypes.c_void_p:
            setattr(c, name, FAKE.value)
    c.critics_ready_event = None
    c.ws0_bytes = c.ws1_bytes = 1 << 40
    c.noise_ctr, c.env_ctr, c.replay_times, c.learner_counter, c.ring_next, c.ring_size = 11, 12, 13, 14, 40, 400
    c.opt_steps[0] = 15
    return c


def _lagged(lag=3, side=False):
    from mpg_amd.fused import LaggedSample
    g = LaggedSample()
    g.lag = lag
    for k in ('policy',) + STAGING:
        setattr(g, k, FAKE.value)
    if side:
        g.side, g.forked, g.done = 0x2000, 0x3000, 0x4000
    g.pending, g.due = 0, 7
    return g


def _alpha(state=FAKE.value, target_entropy=-2.0):
    a = ops.SacAlphaStruct()
    a.state, a.target_entropy = state, target_entropy
    return a


VERSION = {'mpg_step_begin_lagged': 4, 'mpg_sac_step_begin_lagged': 7, 'mpg_sac_auto_step_begin_lagged': 7, 'mpg_lagged_sample_drain': 4}


def _call(lib, name, c, g, iteration=0, alpha=0.03, a=None, stream=NULL):
    cref = ctypes.byref(c) if c is not None else None
    gref = ctypes.byref(g) if g is not None else None
    if name == 'mpg_step_begin_lagged':
        return lib.mpg_step_begin_lagged(cref, gref, I(iteration), stream)
    if name == 'mpg_sac_step_begin_lagged':
        return lib.mpg_sac_step_begin_lagged(cref, F(alpha), gref, I(iteration), stream)
    if name == 'mpg_sac_auto_step_begin_lagged':
        a = a if a is not None else _alpha()
        return lib.mpg_sac_auto_step_begin_lagged(cref, ctypes.byref(a) if a != 'null' else None, gref, I(iteration), stream)
    return lib.mpg_lagged_sample_drain(cref, gref, stream)


def state(c, g):
    return (tuple(int(getattr(c, k)) for k in COUNTERS) + (int(c.opt_steps[0]),) if c is not None else ()) + \
        ((g.pending, g.due) if g is not None else ())


def refused(lib, name, c, g, text, **kw):
    """the call is refused under its name with `text`; no counter of the context and no host field of the object moved"""
    before = state(c, g)
    got = _call(lib, name, c, g, **kw)
    msg = lib.mpg_last_error().decode()
    assert got == MPG_EINVAL, (name, got, msg)
    assert msg.startswith(name + ':') and text in msg, msg
    assert state(c, g) == before, (msg, before, state(c, g))
    return msg


# ---- the lagged form's own refusals, on every entry point ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', NEW)
def test_a_null_object_is_refused(engine, name):
    refused(L.lib(), name, _ctx(VERSION[name]), None, 'null lagged-sample object')


@pytest.mark.parametrize('name', NEW)
@pytest.mark.parametrize('lag', [0, -1, 11])
def test_a_lag_outside_the_interval_is_refused(engine, name, lag):
    msg = refused(L.lib(), name, _ctx(VERSION[name]), _lagged(lag=lag), 'lag out of range')
    assert 'sampling_interval = 10' in msg and '(got %d)' % lag in msg


@pytest.mark.parametrize('name', NEW)
def test_the_ends_of_the_lag_range_pass(engine, name):
    """lag = 1 and lag = sampling_interval pass every refusal: with an empty ring on an iteration that does not sample, the first thing
    left for a begin to object to is the ring - still before anything is enqueued or counted; the drain has nothing pending and returns"""
    lib = L.lib()
    for lag in (1, 10):
        c, g = _ctx(VERSION[name]), _lagged(lag=lag)
        c.ring_size = 0
        if name == 'mpg_lagged_sample_drain':
            before = state(c, g)
            assert _call(lib, name, c, g) == 0, lib.mpg_last_error().decode()
            assert state(c, g) == before
        else:
            refused(lib, name, c, g, 'empty replay ring', iteration=1)


@pytest.mark.parametrize('name', NEW)
@pytest.mark.parametrize('field', STAGING)
def test_missing_staging_rows_are_refused(engine, name, field):
    g = _lagged()
    setattr(g, field, None)
    refused(L.lib(), name, _ctx(VERSION[name]), g, 'missing staging rows')


@pytest.mark.parametrize('name', NEW)
def test_a_missing_policy_copy_is_refused(engine, name):
    g = _lagged()
    g.policy = None
    refused(L.lib(), name, _ctx(VERSION[name]), g, 'missing policy copy')


@pytest.mark.parametrize('name', NEW)
def test_a_kernel_timer_with_a_side_stream_is_refused(engine, name):
    lib = L.lib()
    c = _ctx(VERSION[name])
    c.cfg.prof = FAKE.value
    refused(lib, name, c, _lagged(side=True), 'kernel timer (cfg.prof)')
    # ... and is the side stream's alone: on one stream (side null, or the step's own) the timer is no objection
    for g, stream in ((_lagged(), NULL), (_lagged(side=True), ctypes.c_void_p(0x2000))):
        c.ring_size = 0
        if name != 'mpg_lagged_sample_drain':
            refused(lib, name, c, g, 'empty replay ring', iteration=1, stream=stream)


@pytest.mark.parametrize('name', NEW)
@pytest.mark.parametrize('event', ['forked', 'done'])
def test_a_side_stream_without_its_events_is_refused(engine, name, event):
    g = _lagged(side=True)
    setattr(g, event, None)
    refused(L.lib(), name, _ctx(VERSION[name]), g, 'needs both events')


@pytest.mark.parametrize('name', NEW)
def test_more_than_one_rank_is_refused(engine, name):
    c = _ctx(VERSION[name])
    c.world_size = 2
    refused(L.lib(), name, c, _lagged(), 'world_size > 1 is not served with a lagged sample (got 2)')


@pytest.mark.parametrize('name', NEW)
def test_a_ring_smaller_than_one_sample_and_no_iterations_are_refused(engine, name):
    lib = L.lib()
    c = _ctx(VERSION[name])
    c.ring_capacity = 8 * 64 - 1
    refused(lib, name, c, _lagged(), 'ring smaller than one sample')
    c = _ctx(VERSION[name])
    c.sample_iters = 0
    refused(lib, name, c, _lagged(), 'sample_iters = 0')


@pytest.mark.parametrize('name', BEGINS)
def test_a_sample_still_pending_at_a_sampling_iteration_is_refused(engine, name):
    g = _lagged(lag=3)
    g.pending, g.due = 64, 13
    refused(L.lib(), name, _ctx(VERSION[name]), g, 'still pending', iteration=10)


# ---- everything the plain begin of the version refuses ------------------------------------------------------------------------------
def test_step_begin_lagged_refuses_what_mpg_step_begin_refuses(engine):
    lib, name = L.lib(), 'mpg_step_begin_lagged'
    refused(lib, name, None, _lagged(), 'incomplete context')
    refused(lib, name, _ctx(7), _lagged(), 'learner_version 7 (SAC) takes its temperature as an argument')
    for v in (0, 6, 9):
        refused(lib, name, _ctx(v), _lagged(), 'incomplete context')
    for k, v in (('num_agent', 0), ('batch', 0), ('sampling_interval', 0), ('ring_capacity', 0), ('params', None), ('grad', None),
                 ('ws1', None), ('scratch', None)):
        c = _ctx(4)
        setattr(c, k, v)
        refused(lib, name, c, _lagged(), 'incomplete context')
    refused(lib, name, _ctx(3, DP), _lagged(), 'MuJoCo')
    # version 8 keeps its own words
    c = _ctx(8)
    c.n = 32
    assert 'learner_version 8' in refused(lib, name, c, _lagged(), '0 < n < 32 (got 32)')
    c = _ctx(8)
    c.w_obs = None
    refused(lib, name, c, _lagged(), 'null pointer: w_obs')


@pytest.mark.parametrize('name', BEGINS[1:])
def test_sac_begins_lagged_refuse_what_their_plain_begins_refuse(engine, name):
    lib = L.lib()
    refused(lib, name, None, _lagged(), 'null context')
    refused(lib, name, _ctx(4), _lagged(), 'learner_version 7 (SAC) only (got 4)')
    c = _ctx(7)
    c.scratch = None
    refused(lib, name, c, _lagged(), 'incomplete context')
    c = _ctx(7)
    c.prioritized = 1
    refused(lib, name, c, _lagged(), 'prioritized replay buffer is not served')
    c = _ctx(7)
    c.explore_sigma = 0.1
    refused(lib, name, c, _lagged(), 'explore_sigma on top of the stochastic policy is not served')
    if name == 'mpg_sac_step_begin_lagged':
        for alpha in (-0.1, float('inf'), float('nan')):
            refused(lib, name, _ctx(7), _lagged(), 'alpha must be finite and not negative', alpha=alpha)
    else:
        refused(lib, name, _ctx(7), _lagged(), 'null temperature struct', a='null')
        refused(lib, name, _ctx(7), _lagged(), 'null temperature state', a=_alpha(state=None))
        refused(lib, name, _ctx(7), _lagged(), 'target_entropy must be finite', a=_alpha(target_entropy=float('nan')))


def test_the_drain_refuses_an_incomplete_context(engine):
    lib = L.lib()
    refused(lib, 'mpg_lagged_sample_drain', None, _lagged(), 'incomplete context')
    c = _ctx(4)
    c.params = None
    refused(lib, 'mpg_lagged_sample_drain', c, _lagged(), 'incomplete context')


# ---- the optimizer's keyword ----------------------------------------------------------------------------------------------------------
def test_sample_lag_is_refused_at_construction(monkeypatch):
    """before anything is sampled or looked at: the worker, learner and buffer here are bare objects that could not take a step"""
    from mpg_amd import dist as D
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer as Opt
    bare = types.SimpleNamespace()
    for lag in (0, -1, 11, 1.5, True):
        with pytest.raises(ValueError, match=r'^sample_lag must be an integer within 1 \.\. sampling_interval = 10'):
            Opt(bare, bare, bare, None, bare, sample_lag=lag)
    with pytest.raises(ValueError, match=r'^sample_lag must be .* sampling_interval = 3 \(got 4\)'):
        Opt(bare, bare, bare, None, bare, sampling_interval=3, sample_lag=4)
    monkeypatch.setattr(D, 'world_size', lambda: 2)
    with pytest.raises(ValueError, match=r'^sample_lag is not served with world_size > 1 \(got 2\)'):
        Opt(bare, bare, bare, None, bare, sample_lag=1)
