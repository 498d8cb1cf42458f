"""The AMPC entry point and the policy-only stack at the drop-in boundary, without a GPU: both libraries export the symbols, the
workspace query answers 0 for every request the entry point refuses and grows with rows, M and n, every refusal comes back as
MPG_EINVAL with its own text before any launch (every pointer is FAKE: a launch would fault), PolicyWithQs(policy_only=True) builds
on the host, and AMPCLearner names what it needs."""
import ctypes

import pytest

from mpg_amd import _lib as L
from mpg_amd import ops

NULL, FAKE = ctypes.c_void_p(0), ctypes.c_void_p(0x1000)
I, F, U64, SZ = ctypes.c_int, ctypes.c_float, ctypes.c_uint64, ctypes.c_size_t
MPG_EINVAL, MPG_EWORKSPACE = -1000, -1001
NEW = ('mpg_ampc_pg', 'mpg_ampc_pg_workspace_bytes')
ENGINES = sorted(L.ENGINES)
CFGS = {
    'path-tracking': lambda: ops.make_cfg('PathTracking-v0'),
    'path-tracking-K3': lambda: ops.make_cfg('PathTracking-v0', obs_dim=9),
    'pendulum': lambda: ops.make_cfg('InvertedPendulumConti-v0'),
    'double-pendulum': lambda: ops.make_cfg('InvertedDoublePendulum-v2'),
}


@pytest.fixture(scope='module')
def built():
    from mpg_amd import build as B
    return B.build(verbose=False)


@pytest.mark.parametrize('engine', ENGINES)
def test_both_libraries_export_the_new_entry_points(built, engine):
    assert set(NEW) <= set(L.declared_symbols())
    lib = ctypes.CDLL(L.ENGINES[engine])
    assert not [n for n in NEW if not hasattr(lib, n)]
    assert lib.mpg_abi_version() == 10           # functions were added: no layout or signature changed
    assert L.declared_return_types()['mpg_ampc_pg_workspace_bytes'] == 'size_t'


def _query(lib, cfg, rows, M, n):
    return lib.mpg_ampc_pg_workspace_bytes(ctypes.byref(cfg), I(rows), I(M), I(n))


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('kind', sorted(CFGS))
def test_workspace_query(engine, kind):
    with L.engine(engine):
        lib, cfg = L.lib(), CFGS[kind]()
        base = _query(lib, cfg, 64, 1, 10)
        assert base > 0
        assert _query(lib, cfg, 128, 1, 10) > base and _query(lib, cfg, 64, 2, 10) > base and _query(lib, cfg, 64, 1, 11) > base
        assert _query(lib, cfg, 32, 2, 10) > 0 and _query(lib, cfg, 24, 2, 10) > 0          # rows*M a multiple of 16; rows need not be
        # no critic in it: below the critic path's workspace for the same rollout
        assert _query(lib, cfg, 4096, 1, 25) < lib.mpg_rollout_pg_workspace_bytes(ctypes.byref(cfg), I(4096), I(1), I(25), I(1), I(1))
        for rows, M, n in ((24, 1, 10), (8, 3, 10), (0, 1, 10), (-16, 1, 10), (64, 0, 10), (64, 1, 0), (64, 1, 32), (64, 1, -1)):
            assert _query(lib, cfg, rows, M, n) == 0, (rows, M, n)
        assert lib.mpg_ampc_pg_workspace_bytes(NULL, I(64), I(1), I(10)) == 0


def test_workspace_query_refuses_a_mismatched_cfg():
    lib = L.lib()
    for bad in (dict(obs_dim=5), dict(obs_dim=17), dict(act_dim=1), dict(env_kind=1), dict(env_kind=2)):
        cfg = ops.make_cfg('PathTracking-v0')
        for k, v in bad.items():
            setattr(cfg, k, v)
        assert _query(lib, cfg, 64, 1, 10) == 0, bad
    assert _query(lib, ops.make_cfg('PathTracking-v0', policy_out_activation='tanh', action_range=1.0), 64, 1, 10) == 0


def _call(lib, cfg, policy=FAKE, rows=64, M=1, n=10, obs0=FAKE, eps=NULL, ret_sum=FAKE, ret_sqsum=FAKE, grad=FAKE, ws=FAKE, nbytes=1 << 40):
    ref = NULL if cfg is None else ctypes.byref(cfg)
    return lib.mpg_ampc_pg(ref, policy, I(rows), I(M), I(n), obs0, eps, U64(1), U64(0), F(1. / 64), ret_sum, ret_sqsum, grad, ws, SZ(nbytes), NULL)


REFUSALS = [
    (dict(rows=24), 'rows*M % 16 == 0 (got 24)'),
    (dict(rows=8, M=3), 'rows*M % 16 == 0 (got 24)'),
    (dict(n=0), '0 < n < 32 (got 0)'),
    (dict(n=32), '0 < n < 32 (got 32)'),
    (dict(rows=0), 'no rows'),
    (dict(M=0), 'no rows'),
    (dict(policy=NULL), 'null pointer'),
    (dict(obs0=NULL), 'null pointer'),
    (dict(ret_sum=NULL), 'null pointer'),
    (dict(ret_sqsum=NULL), 'null pointer'),
    (dict(grad=NULL), 'null pointer'),
    (dict(ws=NULL), 'null pointer'),
]


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('case', range(len(REFUSALS)), ids=['%02d-%s' % (i, '-'.join(c[0])) for i, c in enumerate(REFUSALS)])
def test_refusals_have_their_own_texts(engine, case):
    kw, text = REFUSALS[case]
    with L.engine(engine):
        lib = L.lib()
        rc = _call(lib, ops.make_cfg('PathTracking-v0'), **kw)
        msg = lib.mpg_last_error().decode()
        assert rc == MPG_EINVAL, (rc, msg)
        assert msg.startswith('mpg_ampc_pg:') and text in msg, msg


@pytest.mark.parametrize('engine', ENGINES)
def test_refuses_a_null_or_unsupported_configuration_and_a_short_workspace(engine):
    with L.engine(engine):
        lib = L.lib()
        assert _call(lib, None) == MPG_EINVAL and lib.mpg_last_error().decode().startswith('mpg_ampc_pg: unsupported cfg')
        tr = ops.make_cfg('PathTracking-v0', policy_out_activation='tanh', action_range=1.0)
        assert _call(lib, tr) == MPG_EINVAL and lib.mpg_last_error().decode().startswith('mpg_ampc_pg: unsupported cfg')
        cfg = ops.make_cfg('PathTracking-v0')
        need = _query(lib, cfg, 64, 1, 10)
        rc = _call(lib, cfg, nbytes=need - 1)
        msg = lib.mpg_last_error().decode()
        assert rc == MPG_EWORKSPACE and msg.startswith('mpg_ampc_pg:') and '%d < %d' % (need - 1, need) in msg, (rc, msg)
        with pytest.raises(L.MpgError, match='mpg_ampc_pg'):
            L.call('mpg_ampc_pg', ctypes.byref(cfg), FAKE, I(64), I(1), I(0), FAKE, NULL, U64(1), U64(0), F(1. / 64), FAKE, FAKE, FAKE, FAKE,
                   SZ(1 << 40), NULL)


# ---- the Python layer (nothing here touches a device) ---------------------------------------------------------------------------
def test_policy_only_stack_builds_on_the_host():
    from mpg_amd.config import default_args
    from mpg_amd.policy import PolicyWithQs
    pw = PolicyWithQs(**vars(default_args('AMPC')), device='cpu')            # tau, delay_update, alpha None; double_Q, target False
    assert pw.names == ['policy'] and pw.policy_only
    assert pw.sizes == [ops.net_size(6, 4)] and int(pw.offsets[-1]) == pw.params.numel()
    w = pw.get_weights()
    assert len(w) == 1 and [tuple(a.shape) for a in w[0]] == [(6, 256), (256,), (256, 256), (256,), (256, 4), (4,)]
    w[0][1] += 1.0                                                          # copies: the live parameters do not move ...
    assert float(pw.net('policy')[6 * 256:7 * 256].abs().max()) == 0.0
    pw.set_weights(w)                                                       # ... until the list is handed back
    assert float(pw.net('policy')[6 * 256:7 * 256].min()) == 1.0
    assert list(pw.opt_steps) == ['policy'] and list(pw.state_dict()['names']) == ['policy']
    with pytest.raises(AssertionError, match='one model'):
        pw.set_weights(w + w)
    k3 = PolicyWithQs(**vars(default_args('AMPC', num_future_data=3)), device='cpu')
    assert k3.names == ['policy'] and k3.sizes == [ops.net_size(9, 4)]


def test_the_scope_assertion_still_fires_without_policy_only():
    from mpg_amd.config import default_args
    from mpg_amd.policy import PolicyWithQs
    for alg in ('MPG-v2', 'NDPG', 'TD3'):
        with pytest.raises(AssertionError, match='hot-path scope'):
            PolicyWithQs(**vars(default_args(alg, target=False)), device='cpu')
    with pytest.raises(AssertionError, match='hot-path scope'):
        PolicyWithQs(**vars(default_args('AMPC', policy_only=False)), device='cpu')


def test_learner_refuses_a_stack_with_critics_by_name():
    from mpg_amd.config import default_args
    from mpg_amd.learners import AMPCLearner
    from mpg_amd.policy import PolicyWithQs
    with pytest.raises(ValueError, match='policy_only=True'):
        AMPCLearner(PolicyWithQs, default_args('AMPC', policy_only=False, target=True, tau=0.005, delay_update=1), device='cpu')
    with pytest.raises(ValueError, match='AMPCLearner'):
        AMPCLearner(PolicyWithQs, default_args('NADP'), device='cpu')
    ln = AMPCLearner(PolicyWithQs, default_args('AMPC', M=2, num_rollout_list_for_policy_update=[10]), device='cpu')
    assert (ln.M, ln.n, ln.num_batch_reuse) == (2, 10, 1) and ln.policy_with_value.names == ['policy']
    assert ln.flat.numel() == ops.net_size(6, 4) + 16 and ln.norms.numel() == 1

