"""The Gaussian-head entry points (mpg_policy_sample, mpg_sac_targets, mpg_sac_policy_grad and their workspace queries) at the drop-in
boundary, without a GPU: both libraries export them, the ABI version is unchanged, and every refusal comes back with its code and its
text before any launch (every pointer is FAKE: a launch would fault)."""
import ctypes

import pytest

from mpg_amd import _lib as L
from mpg_amd import ops

NULL, FAKE = ctypes.c_void_p(0), ctypes.c_void_p(0x1000)
I, F, SZ = ctypes.c_int, ctypes.c_float, ctypes.c_size_t
MPG_EINVAL, MPG_EWORKSPACE = -1000, -1001
ENTRY = ('mpg_policy_sample', 'mpg_sac_targets', 'mpg_sac_policy_grad')
NEW = ENTRY + tuple(n + '_workspace_bytes' for n in ENTRY)
ENGINES = sorted(L.ENGINES)
BIG = 1 << 40


@pytest.fixture(scope='module')
def built():
    from mpg_amd import build as B
    return B.build(verbose=False)


@pytest.mark.parametrize('engine', ENGINES)
def test_both_libraries_export_the_six_symbols(built, engine):
    assert set(NEW) <= set(L.declared_symbols())
    lib = ctypes.CDLL(L.ENGINES[engine])
    assert not [n for n in NEW if not hasattr(lib, n)]
    assert lib.mpg_abi_version() == 10           # functions were added: no layout or signature changed


def _cfg(obs_dim=6, **kw):
    c = ops.make_cfg('PathTracking-v0', obs_dim=obs_dim, policy_out_activation='linear')
    for k, v in kw.items():
        setattr(c, k, v)
    return c


# the pointer arguments of each entry point by name, in call order, and how the call is made from them
POINTERS = {'mpg_policy_sample': ('policy', 'obs', 'eps', 'act_out', 'logp_out', 'ws'),
            'mpg_sac_targets': ('policy', 'q1t', 'q2t', 'rew', 'obs_tp1', 'eps', 'y', 'ws'),
            'mpg_sac_policy_grad': ('policy', 'q1', 'q2', 'obs', 'eps', 'qmin_sum', 'qmin_sqsum', 'logp_sum', 'grad', 'ws')}


def invoke(lib, name, cfg_ref, p, rows=64, alpha=0.03, ws_bytes=BIG):
    if name == 'mpg_policy_sample':
        return lib.mpg_policy_sample(cfg_ref, p['policy'], I(rows), p['obs'], p['eps'], p['act_out'], p['logp_out'], NULL, p['ws'],
                                     SZ(ws_bytes), NULL)
    if name == 'mpg_sac_targets':
        return lib.mpg_sac_targets(cfg_ref, p['policy'], p['q1t'], p['q2t'], I(rows), p['rew'], p['obs_tp1'], p['eps'], F(alpha), p['y'],
                                   p['ws'], SZ(ws_bytes), NULL)
    return lib.mpg_sac_policy_grad(cfg_ref, p['policy'], p['q1'], p['q2'], I(rows), p['obs'], p['eps'], F(alpha), F(1.0 / 64),
                                   p['qmin_sum'], p['qmin_sqsum'], p['logp_sum'], p['grad'], p['ws'], SZ(ws_bytes), NULL)


def refused(lib, name, rc, text, code=MPG_EINVAL):
    msg = lib.mpg_last_error().decode()
    assert rc == code, (name, rc, msg)
    assert msg.startswith(name + ':') and text in msg, msg


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('name', ENTRY)
def test_null_pointers_and_rows(engine, name):
    with L.engine(engine):
        lib = L.lib()
        cfg = _cfg()
        ok = {k: FAKE for k in POINTERS[name]}
        for k in POINTERS[name]:
            refused(lib, name, invoke(lib, name, ctypes.byref(cfg), dict(ok, **{k: NULL})), 'null pointer')
        refused(lib, name, invoke(lib, name, NULL, ok), 'null pointer')
        for rows in (0, -3):
            refused(lib, name, invoke(lib, name, ctypes.byref(cfg), ok, rows=rows), 'rows')
        with pytest.raises(L.MpgError, match=name):
            L.check(invoke(lib, name, ctypes.byref(cfg), ok, rows=0), name)


HEAD = 'Gaussian head without an action range only'
CFG_REFUSALS = [('pendulum', lambda: ops.make_cfg('InvertedPendulumConti-v0'), HEAD),
                ('double-pendulum', lambda: ops.make_cfg('InvertedDoublePendulum-v2'), HEAD),
                ('act_dim-1', lambda: _cfg(act_dim=1), HEAD),
                ('env_kind-1', lambda: _cfg(env_kind=1), HEAD),
                ('action_range', lambda: _cfg(action_range=1.0), HEAD),
                ('obs_dim-17', lambda: _with_obs(17), 'observation width'),
                ('obs_dim-5', lambda: _with_obs(5), 'observation width')]


def _with_obs(n):
    c = _cfg()
    c.obs_dim = n
    return c


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('name', ENTRY)
@pytest.mark.parametrize('case', range(len(CFG_REFUSALS)), ids=[c[0] for c in CFG_REFUSALS])
def test_configurations_refused(engine, name, case):
    _, make, text = CFG_REFUSALS[case]
    with L.engine(engine):
        lib = L.lib()
        cfg = make()
        refused(lib, name, invoke(lib, name, ctypes.byref(cfg), {k: FAKE for k in POINTERS[name]}), text)
        assert getattr(lib, name + '_workspace_bytes')(ctypes.byref(cfg), I(64)) == 0


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('name', ENTRY[1:])
@pytest.mark.parametrize('alpha', [-0.03, float('inf'), float('nan')])
def test_alpha_refused(engine, name, alpha):
    with L.engine(engine):
        lib = L.lib()
        cfg = _cfg()
        refused(lib, name, invoke(lib, name, ctypes.byref(cfg), {k: FAKE for k in POINTERS[name]}, alpha=alpha), 'alpha')


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('name', ENTRY)
@pytest.mark.parametrize('obs_dim', [6, 9, 16])
def test_workspace(engine, name, obs_dim):
    """the query answers, refuses what the entry point refuses, and a buffer one byte short is refused with both sizes"""
    with L.engine(engine):
        lib = L.lib()
        cfg = _cfg(obs_dim=obs_dim)
        query = getattr(lib, name + '_workspace_bytes')
        need = query(ctypes.byref(cfg), I(4096))
        assert need > 0
        assert query(ctypes.byref(cfg), I(0)) == 0 and query(NULL, I(4096)) == 0
        assert query(ctypes.byref(cfg), I(8192)) > need
        rc = invoke(lib, name, ctypes.byref(cfg), {k: FAKE for k in POINTERS[name]}, rows=4096, ws_bytes=need - 1)
        refused(lib, name, rc, '%d < %d' % (need - 1, need), code=MPG_EWORKSPACE)
    if name == 'mpg_sac_policy_grad':
        with L.engine(engine):
            # the TD3 entry point's arrays plus the logits, log-densities and the four-column output gradient
            assert need > L.lib().mpg_td3_policy_grad_workspace_bytes(ctypes.byref(cfg), I(4096))


@pytest.mark.parametrize('engine', ENGINES)
def test_other_shapes_keep_their_refusal(engine):
    """the dispatch gained (6 .. 16, 4) only: any other width with four used outputs, and every shape refused before, still answers with
    the text it had (rows = 1 and fake pointers: the shape is refused before the launch)"""
    with L.engine(engine):
        lib = L.lib()
        for din, used in ((5, 4), (4, 4), (17, 4), (24, 4), (6, 3), (5, 2), (24, 2)):
            rc = lib.mpg_mlp_forward(FAKE, I(din), I(4), I(used), I(0), I(1), FAKE, NULL, I(0), FAKE, NULL, NULL)
            msg = lib.mpg_last_error().decode()
            assert rc == MPG_EINVAL and msg == 'unsupported network shape in=%d used-out=%d' % (din, used), (rc, msg)


# ---- the Python layer's refusals (raised before anything touches the device) ---------------------------------------------------
def test_policy_refuses_what_the_gaussian_head_does_not_serve():
    from mpg_amd.policy import PolicyWithQs
    base = dict(obs_dim=6, act_dim=2, deterministic_policy=False, policy_out_activation='linear', device='cpu')
    with pytest.raises(ValueError, match='learned temperature'):
        PolicyWithQs(alpha='auto', **base)
    with pytest.raises(ValueError, match='finite alpha'):
        PolicyWithQs(alpha=None, **base)
    with pytest.raises(ValueError, match='finite alpha'):
        PolicyWithQs(alpha=-0.1, **base)
    with pytest.raises(ValueError, match='action_range'):
        PolicyWithQs(alpha=0.03, action_range=1.0, **base)
    with pytest.raises(ValueError, match='act_dim 2'):
        PolicyWithQs(alpha=0.03, **dict(base, obs_dim=4, act_dim=1, env_id='InvertedPendulumConti-v0'))
    with pytest.raises(ValueError, match='act_dim 2'):
        PolicyWithQs(alpha=0.03, **dict(base, act_dim=1))


def test_learner_refusals():
    from mpg_amd.config import default_args
    from mpg_amd.learners import SACLearner
    from mpg_amd.policy import PolicyWithQs
    with pytest.raises(ValueError, match="alpha = 'auto'"):
        SACLearner(PolicyWithQs, default_args('SAC', alpha='auto'), device='cpu')
    with pytest.raises(ValueError, match='deterministic_policy=False'):
        SACLearner(PolicyWithQs, default_args('SAC', deterministic_policy=True), device='cpu')
    with pytest.raises(ValueError, match='PathTracking-v0 only'):
        SACLearner(PolicyWithQs, default_args('SAC', env_id='InvertedPendulumConti-v0'), device='cpu')
    with pytest.raises(ValueError, match='action_range'):
        SACLearner(PolicyWithQs, default_args('SAC', action_range=1.0), device='cpu')
