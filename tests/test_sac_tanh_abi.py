"""The squashed-head entry points (mpg_policy_sample_squashed, mpg_sac_targets_squashed, mpg_sac_policy_grad_squashed, the two _auto
forms and the three workspace queries) at the drop-in boundary, without a GPU: both libraries export them, the ABI version is
unchanged, every refusal comes back with its code and its own text before any launch (every pointer is FAKE: a launch would fault),
and the Python layer accepts the head on request only."""
import ctypes

import pytest

from mpg_amd import _lib as L
from mpg_amd import ops

NULL, FAKE = ctypes.c_void_p(0), ctypes.c_void_p(0x1000)
I, F, SZ = ctypes.c_int, ctypes.c_float, ctypes.c_size_t
MPG_EINVAL, MPG_EWORKSPACE = -1000, -1001
ENTRY = ('mpg_policy_sample_squashed', 'mpg_sac_targets_squashed', 'mpg_sac_policy_grad_squashed', 'mpg_sac_targets_squashed_auto',
         'mpg_sac_policy_grad_squashed_auto')
QUERY = {'mpg_policy_sample_squashed': 'mpg_policy_sample_squashed_workspace_bytes',
         'mpg_sac_targets_squashed': 'mpg_sac_targets_squashed_workspace_bytes',
         'mpg_sac_policy_grad_squashed': 'mpg_sac_policy_grad_squashed_workspace_bytes',
         'mpg_sac_targets_squashed_auto': 'mpg_sac_targets_squashed_workspace_bytes',
         'mpg_sac_policy_grad_squashed_auto': 'mpg_sac_policy_grad_squashed_workspace_bytes'}
NEW = ENTRY + tuple(sorted(set(QUERY.values())))
ENGINES = sorted(L.ENGINES)
BIG = 1 << 40


@pytest.fixture(scope='module')
def built():
    from mpg_amd import build as B
    return B.build(verbose=False)


@pytest.mark.parametrize('engine', ENGINES)
def test_both_libraries_export_the_eight_symbols(built, engine):
    assert len(NEW) == 8 and set(NEW) <= set(L.declared_symbols())
    lib = ctypes.CDLL(L.ENGINES[engine])
    assert not [n for n in NEW if not hasattr(lib, n)]
    assert lib.mpg_abi_version() == 10           # functions were added: no layout or signature changed


def pt_cfg(obs_dim=6, action_range=2.0, **kw):
    c = ops.make_cfg('PathTracking-v0', obs_dim=obs_dim, policy_out_activation='linear', action_range=action_range)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def pend_cfg(**kw):
    c = ops.make_cfg('InvertedPendulumConti-v0')        # linear output, action_range 3
    for k, v in kw.items():
        setattr(c, k, v)
    return c


ACCEPTED = [('pendulum', pend_cfg), ('pt-6', pt_cfg), ('pt-9', lambda: pt_cfg(9)), ('pt-16', lambda: pt_cfg(16))]

POINTERS = {'mpg_policy_sample_squashed': ('policy', 'obs', 'eps', 'act_out', 'logp_out', 'ws'),
            'mpg_sac_targets_squashed': ('policy', 'q1t', 'q2t', 'rew', 'obs_tp1', 'eps', 'y', 'ws'),
            'mpg_sac_policy_grad_squashed': ('policy', 'q1', 'q2', 'obs', 'eps', 'qmin_sum', 'qmin_sqsum', 'logp_sum', 'grad', 'ws'),
            'mpg_sac_targets_squashed_auto': ('policy', 'q1t', 'q2t', 'rew', 'obs_tp1', 'eps', 'log_alpha', 'y', 'ws'),
            'mpg_sac_policy_grad_squashed_auto': ('policy', 'q1', 'q2', 'obs', 'eps', 'log_alpha', 'eps_alpha', 'qmin_sum', 'qmin_sqsum',
                                                  'logp_sum', 'alpha_grad', 'grad', 'ws')}


def invoke(lib, name, cfg_ref, p, rows=64, alpha=0.03, ws_bytes=BIG, target_entropy=-2.0):
    if name == 'mpg_policy_sample_squashed':
        return lib.mpg_policy_sample_squashed(cfg_ref, p['policy'], I(rows), p['obs'], p['eps'], p['act_out'], p['logp_out'], NULL, p['ws'],
                                              SZ(ws_bytes), NULL)
    if name == 'mpg_sac_targets_squashed':
        return lib.mpg_sac_targets_squashed(cfg_ref, p['policy'], p['q1t'], p['q2t'], I(rows), p['rew'], p['obs_tp1'], p['eps'], F(alpha),
                                            p['y'], p['ws'], SZ(ws_bytes), NULL)
    if name == 'mpg_sac_policy_grad_squashed':
        return lib.mpg_sac_policy_grad_squashed(cfg_ref, p['policy'], p['q1'], p['q2'], I(rows), p['obs'], p['eps'], F(alpha), F(1.0 / 64),
                                                p['qmin_sum'], p['qmin_sqsum'], p['logp_sum'], p['grad'], p['ws'], SZ(ws_bytes), NULL)
    if name == 'mpg_sac_targets_squashed_auto':
        return lib.mpg_sac_targets_squashed_auto(cfg_ref, p['policy'], p['q1t'], p['q2t'], I(rows), p['rew'], p['obs_tp1'], p['eps'],
                                                 p['log_alpha'], p['y'], p['ws'], SZ(ws_bytes), NULL)
    return lib.mpg_sac_policy_grad_squashed_auto(cfg_ref, p['policy'], p['q1'], p['q2'], I(rows), p['obs'], p['eps'], p['log_alpha'],
                                                 p['eps_alpha'], F(target_entropy), F(1.0 / 64), p['qmin_sum'], p['qmin_sqsum'],
                                                 p['logp_sum'], p['alpha_grad'], p['grad'], p['ws'], SZ(ws_bytes), NULL)


def refused(lib, name, rc, text, code=MPG_EINVAL):
    msg = lib.mpg_last_error().decode()
    assert rc == code, (name, rc, msg)
    assert msg.startswith(name + ':') and text in msg, msg


def fakes(name):
    return {k: FAKE for k in POINTERS[name]}


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('name', ENTRY)
@pytest.mark.parametrize('case', range(len(ACCEPTED)), ids=[c[0] for c in ACCEPTED])
def test_null_pointers_and_rows(engine, name, case):
    with L.engine(engine):
        lib = L.lib()
        cfg = ACCEPTED[case][1]()
        for k in POINTERS[name]:
            refused(lib, name, invoke(lib, name, ctypes.byref(cfg), dict(fakes(name), **{k: NULL})), 'null pointer')
        refused(lib, name, invoke(lib, name, NULL, fakes(name)), 'null pointer')
        for rows in (0, -3):
            refused(lib, name, invoke(lib, name, ctypes.byref(cfg), fakes(name), rows=rows), 'rows must be positive')
        with pytest.raises(L.MpgError, match=name):
            L.check(invoke(lib, name, ctypes.byref(cfg), fakes(name), rows=0), name)


def _with_obs(c, n):
    c.obs_dim = n
    return c


# each refusal has a text of its own
CFG_REFUSALS = [('no-range', lambda: pt_cfg(action_range=0.0), 'needs a positive, finite action range'),
                ('negative-range', lambda: pt_cfg(action_range=-1.0), 'needs a positive, finite action range'),
                ('infinite-range', lambda: pend_cfg(action_range=float('inf')), 'needs a positive, finite action range'),
                ('nan-range', lambda: pend_cfg(action_range=float('nan')), 'needs a positive, finite action range'),
                ('tanh-output', lambda: pt_cfg(policy_out_act=ops.ACT_TANH), 'tanh output activation under an action range'),
                ('tanh-output-pendulum', lambda: pend_cfg(policy_out_act=ops.ACT_TANH), 'tanh output activation under an action range'),
                ('double-pendulum', lambda: ops.make_cfg('InvertedDoublePendulum-v2'), 'not built for the double pendulum'),
                ('act_dim-1-on-pt', lambda: pt_cfg(act_dim=1), 'PathTracking (act_dim 2) or the inverted pendulum (act_dim 1) only'),
                ('act_dim-2-on-pendulum', lambda: pend_cfg(act_dim=2), 'PathTracking (act_dim 2) or the inverted pendulum (act_dim 1) only'),
                ('env_kind-1-on-pt', lambda: pt_cfg(env_kind=1), 'PathTracking (act_dim 2) or the inverted pendulum (act_dim 1) only'),
                ('obs_dim-17', lambda: _with_obs(pt_cfg(), 17), 'unsupported observation width 17'),
                ('obs_dim-5', lambda: _with_obs(pt_cfg(), 5), 'unsupported observation width 5'),
                ('pendulum-obs_dim-6', lambda: _with_obs(pend_cfg(), 6), 'unsupported observation width 6')]


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('name', ENTRY)
@pytest.mark.parametrize('case', range(len(CFG_REFUSALS)), ids=[c[0] for c in CFG_REFUSALS])
def test_configurations_refused(engine, name, case):
    _, make, text = CFG_REFUSALS[case]
    with L.engine(engine):
        lib = L.lib()
        cfg = make()
        refused(lib, name, invoke(lib, name, ctypes.byref(cfg), fakes(name)), text)
        assert getattr(lib, QUERY[name])(ctypes.byref(cfg), I(64)) == 0


def test_the_refusal_texts_differ():
    texts = sorted(set(c[2].rstrip(' 0123456789') for c in CFG_REFUSALS))
    assert len(texts) == 5, texts


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('name', ('mpg_sac_targets_squashed', 'mpg_sac_policy_grad_squashed'))
@pytest.mark.parametrize('alpha', [-0.03, float('inf'), float('nan')])
def test_alpha_refused(engine, name, alpha):
    with L.engine(engine):
        lib = L.lib()
        for make in (pend_cfg, pt_cfg):
            cfg = make()
            refused(lib, name, invoke(lib, name, ctypes.byref(cfg), fakes(name), alpha=alpha), 'alpha must be finite and not negative')


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('te', [float('inf'), float('nan')])
def test_target_entropy_refused(engine, te):
    name = 'mpg_sac_policy_grad_squashed_auto'
    with L.engine(engine):
        lib = L.lib()
        cfg = pend_cfg()
        refused(lib, name, invoke(lib, name, ctypes.byref(cfg), fakes(name), target_entropy=te), 'target_entropy must be finite')


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('name', ENTRY)
@pytest.mark.parametrize('case', range(len(ACCEPTED)), ids=[c[0] for c in ACCEPTED])
def test_workspace(engine, name, case):
    """the query answers, refuses what the entry point refuses, and a buffer one byte short is refused with both sizes"""
    with L.engine(engine):
        lib = L.lib()
        cfg = ACCEPTED[case][1]()
        query = getattr(lib, QUERY[name])
        need = query(ctypes.byref(cfg), I(4096))
        assert need > 0
        assert query(ctypes.byref(cfg), I(0)) == 0 and query(NULL, I(4096)) == 0
        assert query(ctypes.byref(cfg), I(8192)) > need
        rc = invoke(lib, name, ctypes.byref(cfg), fakes(name), rows=4096, ws_bytes=need - 1)
        refused(lib, name, rc, '%d < %d' % (need - 1, need), code=MPG_EWORKSPACE)


@pytest.mark.parametrize('engine', ENGINES)
def test_the_plain_entry_points_keep_refusing_a_range(engine):
    """the squashed forms are siblings: mpg_policy_sample and the others answer a cfg with a range, or the pendulum, as before"""
    head = 'Gaussian head without an action range only'
    with L.engine(engine):
        lib = L.lib()
        for cfg in (pend_cfg(), pt_cfg()):
            rc = lib.mpg_policy_sample(ctypes.byref(cfg), FAKE, I(64), FAKE, FAKE, FAKE, FAKE, NULL, FAKE, SZ(BIG), NULL)
            refused(lib, 'mpg_policy_sample', rc, head)
            for q in ('mpg_policy_sample', 'mpg_sac_targets', 'mpg_sac_policy_grad'):
                assert getattr(lib, q + '_workspace_bytes')(ctypes.byref(cfg), I(64)) == 0
            # ... and a cfg WITHOUT a range is the plain forms' alone
            plain = pt_cfg(action_range=0.0)
            assert lib.mpg_policy_sample_workspace_bytes(ctypes.byref(plain), I(64)) > 0
            assert lib.mpg_policy_sample_squashed_workspace_bytes(ctypes.byref(plain), I(64)) == 0


@pytest.mark.parametrize('engine', ENGINES)
def test_the_dispatch_gained_four_by_two_only(engine):
    """(in 4, used-out 2) leaves the refused shapes; its neighbours keep their refusal and its text (fake pointers, rows = 1: the shape is
    refused before the launch)"""
    with L.engine(engine):
        lib = L.lib()
        for din, used in ((5, 2), (3, 2), (24, 2), (4, 3), (4, 4)):
            rc = lib.mpg_mlp_forward(FAKE, I(din), I(4), I(used), I(0), I(1), FAKE, NULL, I(0), FAKE, NULL, NULL)
            msg = lib.mpg_last_error().decode()
            assert rc == MPG_EINVAL and msg == 'unsupported network shape in=%d used-out=%d' % (din, used), (rc, msg)


# ---- the Python layer (raised before anything touches the device) ---------------------------------------------------------------
BASE = dict(deterministic_policy=False, policy_out_activation='linear', device='cpu', alpha=0.03)
PEND = dict(BASE, obs_dim=4, act_dim=1, env_id='InvertedPendulumConti-v0')
PT = dict(BASE, obs_dim=6, act_dim=2)


def test_policy_accepts_the_head_on_request():
    from mpg_amd.policy import PolicyWithQs
    for kw, R in ((PEND, 3.0), (PT, 2.0), (dict(PT, obs_dim=9), 1.0), (dict(PEND, alpha='auto', target_entropy=-2.), 3.0)):
        pw = PolicyWithQs(action_range=R, squashed_head=True, **kw)
        assert pw.squashed_head and not pw.deterministic_policy and pw.cfg.action_range == R
        assert pw.dims['policy'] == (kw['obs_dim'], 2 * kw['act_dim']) and pw.state_dict()['squashed_head'] is True
    # a deterministic policy has no head to squash: the flag is not looked at
    assert not PolicyWithQs(obs_dim=4, act_dim=1, env_id='InvertedPendulumConti-v0', action_range=3., policy_out_activation='linear',
                            squashed_head=True, device='cpu').squashed_head


def test_policy_refusals():
    from mpg_amd.policy import PolicyWithQs
    # without the keyword every refusal stays, with its text
    with pytest.raises(ValueError, match='is not built: its tanh-affine bijector changes the log-density'):
        PolicyWithQs(action_range=3.0, **PEND)
    with pytest.raises(ValueError, match='is not built: its tanh-affine bijector changes the log-density'):
        PolicyWithQs(action_range=1.0, squashed_head=False, **PT)
    with pytest.raises(ValueError, match='built for PathTracking-v0 with act_dim 2'):
        PolicyWithQs(**PEND)
    # with it: a text of its own for a missing range, and for what the head does not serve
    for R in (None, 0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='squashed_head=True needs a positive, finite action_range'):
            PolicyWithQs(action_range=R, squashed_head=True, **PT)
    with pytest.raises(ValueError, match='tanh.tanh'):
        PolicyWithQs(action_range=2.0, squashed_head=True, **dict(PT, policy_out_activation='tanh'))
    with pytest.raises(ValueError, match='the squashed head is built for'):
        PolicyWithQs(action_range=1.0, squashed_head=True, **dict(BASE, obs_dim=11, act_dim=1, env_id='InvertedDoublePendulum-v2'))
    with pytest.raises(ValueError, match='the squashed head is built for'):
        PolicyWithQs(action_range=1.0, squashed_head=True, **dict(PT, act_dim=1))
    with pytest.raises(ValueError, match='finite alpha'):
        PolicyWithQs(action_range=3.0, squashed_head=True, **dict(PEND, alpha=None))


def test_state_dict_carries_the_flag():
    from mpg_amd.policy import PolicyWithQs
    sq = PolicyWithQs(action_range=2.0, squashed_head=True, **PT)
    plain = PolicyWithQs(**PT)
    assert 'squashed_head' not in plain.state_dict()           # a plain stack keeps the keys it had
    sq.load_state_dict(sq.state_dict())
    with pytest.raises(ValueError, match='differ in the policy head'):
        plain.load_state_dict(sq.state_dict())
    with pytest.raises(ValueError, match='differ in the policy head'):
        sq.load_state_dict(plain.state_dict())


def test_learner_refusals_and_acceptances():
    from mpg_amd.config import default_args
    from mpg_amd.learners import SACLearner
    from mpg_amd.policy import PolicyWithQs
    pend = 'InvertedPendulumConti-v0'
    with pytest.raises(ValueError, match='PathTracking-v0 only'):
        SACLearner(PolicyWithQs, default_args('SAC', env_id=pend), device='cpu')
    with pytest.raises(ValueError, match='action_range'):
        SACLearner(PolicyWithQs, default_args('SAC', action_range=1.0), device='cpu')
    with pytest.raises(ValueError, match='squashed_head=True serves PathTracking-v0 and InvertedPendulumConti-v0'):
        SACLearner(PolicyWithQs, default_args('SAC', env_id='InvertedDoublePendulum-v2', squashed_head=True), device='cpu')
    with pytest.raises(ValueError, match='needs a positive, finite action_range'):
        SACLearner(PolicyWithQs, default_args('SAC', squashed_head=True), device='cpu')
    with pytest.raises(ValueError, match='deterministic_policy=False'):
        SACLearner(PolicyWithQs, default_args('SAC', env_id=pend, squashed_head=True, deterministic_policy=True), device='cpu')
    for kw in (dict(env_id=pend), dict(action_range=2.0), dict(env_id=pend, alpha='auto', target_entropy=-2.),
               dict(env_id=pend, buffer_type='priority')):
        ln = SACLearner(PolicyWithQs, default_args('SAC', squashed_head=True, **kw), device='cpu')
        assert ln.squashed and ln.policy_with_value.squashed_head
        assert ln.policy_with_value.names == ['Q1', 'Q2', 'policy']
    assert not SACLearner(PolicyWithQs, default_args('SAC'), device='cpu').squashed


def test_native_sac_refuses_a_squashed_stack():
    """SingleProcessOffPolicyOptimizer(native_sac=True) raises before anything is sampled: the worker here would fail at its first call"""
    from mpg_amd.config import default_args
    from mpg_amd.learners import SACLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    args = default_args('SAC', env_id='InvertedPendulumConti-v0', squashed_head=True)
    learner = SACLearner(PolicyWithQs, args, device='cpu')

    class Worker(object):
        explore_sigma = None
        policy_with_value = learner.policy_with_value

        def sample_with_count(self):
            raise AssertionError('sampled before the refusal')

    with pytest.raises(ValueError, match='native_sac=True: the tanh-squashed head'):
        SingleProcessOffPolicyOptimizer(Worker(), learner, object(), None, args, native_sac=True)
