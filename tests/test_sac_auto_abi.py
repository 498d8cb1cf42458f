"""The learned temperature of SAC (alpha = 'auto') at the drop-in boundary, without a GPU: both libraries export mpg_sac_targets_auto,
mpg_sac_policy_grad_auto and mpg_sac_alpha_update, the ABI version is unchanged, every refusal comes back with its code and its own
text before any launch (every pointer is FAKE: a launch would fault) and leaves the struct as it was; ops.py mirrors mpg_sac_alpha_t;
PolicyWithQs on the host lists, sets and saves the temperature, and a stack with a fixed temperature keeps its keys."""
import ctypes

import numpy as np
import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops

NULL, FAKE = ctypes.c_void_p(0), ctypes.c_void_p(0x1000)
I, F, SZ = ctypes.c_int, ctypes.c_float, ctypes.c_size_t
MPG_EINVAL, MPG_EWORKSPACE = -1000, -1001
ENTRY = ('mpg_sac_targets_auto', 'mpg_sac_policy_grad_auto')
NEW = ENTRY + ('mpg_sac_alpha_update', 'mpg_sac_auto_step_begin', 'mpg_sac_auto_step_end')
ENGINES = sorted(L.ENGINES)
BIG = 1 << 40
POINTERS = {'mpg_sac_targets_auto': ('policy', 'q1t', 'q2t', 'rew', 'obs_tp1', 'eps', 'log_alpha', 'y', 'ws'),
            'mpg_sac_policy_grad_auto': ('policy', 'q1', 'q2', 'obs', 'eps', 'log_alpha', 'eps_alpha', 'qmin_sum', 'qmin_sqsum', 'logp_sum',
                                         'alpha_grad', 'grad', 'ws')}
QUERY = {'mpg_sac_targets_auto': 'mpg_sac_targets_workspace_bytes', 'mpg_sac_policy_grad_auto': 'mpg_sac_policy_grad_workspace_bytes'}


@pytest.fixture(scope='module')
def built():
    from mpg_amd import build as B
    return B.build(verbose=False)


@pytest.mark.parametrize('engine', ENGINES)
def test_both_libraries_export_the_new_symbols(built, engine):
    assert set(NEW) <= set(L.declared_symbols())
    lib = ctypes.CDLL(L.ENGINES[engine])
    assert not [n for n in NEW if not hasattr(lib, n)]
    assert lib.mpg_abi_version() == 10           # functions and one struct were added: no layout or signature changed


def _cfg(obs_dim=6, **kw):
    c = ops.make_cfg('PathTracking-v0', obs_dim=obs_dim, policy_out_activation='linear')
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _with_obs(n):
    c = _cfg()
    c.obs_dim = n
    return c


def invoke(lib, name, cfg_ref, p, rows=64, target_entropy=-2.0, ws_bytes=BIG):
    if name == 'mpg_sac_targets_auto':
        return lib.mpg_sac_targets_auto(cfg_ref, p['policy'], p['q1t'], p['q2t'], I(rows), p['rew'], p['obs_tp1'], p['eps'], p['log_alpha'],
                                        p['y'], p['ws'], SZ(ws_bytes), NULL)
    return lib.mpg_sac_policy_grad_auto(cfg_ref, p['policy'], p['q1'], p['q2'], I(rows), p['obs'], p['eps'], p['log_alpha'], p['eps_alpha'],
                                        F(target_entropy), F(1.0 / 64), p['qmin_sum'], p['qmin_sqsum'], p['logp_sum'], p['alpha_grad'],
                                        p['grad'], p['ws'], SZ(ws_bytes), NULL)


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


HEAD = 'Gaussian head without an action range only'


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('name', ENTRY)
def test_configurations_refused(engine, name):
    with L.engine(engine):
        lib = L.lib()
        ok = {k: FAKE for k in POINTERS[name]}
        for make, text in ((lambda: ops.make_cfg('InvertedPendulumConti-v0'), HEAD), (lambda: _cfg(act_dim=1), HEAD),
                           (lambda: _cfg(env_kind=1), HEAD), (lambda: _cfg(action_range=1.0), HEAD),
                           (lambda: _with_obs(17), 'observation width'), (lambda: _with_obs(5), 'observation width')):
            cfg = make()
            refused(lib, name, invoke(lib, name, ctypes.byref(cfg), ok), text)


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('h', [float('nan'), float('inf'), -float('inf')])
def test_target_entropy_refused(engine, h):
    with L.engine(engine):
        lib = L.lib()
        cfg = _cfg()
        name = 'mpg_sac_policy_grad_auto'
        refused(lib, name, invoke(lib, name, ctypes.byref(cfg), {k: FAKE for k in POINTERS[name]}, target_entropy=h), 'target_entropy')


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('name', ENTRY)
@pytest.mark.parametrize('obs_dim', [6, 9])
def test_workspace_one_byte_short(engine, name, obs_dim):
    """the _auto entry points take the workspaces of the host-alpha ones: one byte short is refused with both sizes"""
    with L.engine(engine):
        lib = L.lib()
        cfg = _cfg(obs_dim=obs_dim)
        need = getattr(lib, QUERY[name])(ctypes.byref(cfg), I(4096))
        assert need > 0
        rc = invoke(lib, name, ctypes.byref(cfg), {k: FAKE for k in POINTERS[name]}, rows=4096, ws_bytes=need - 1)
        refused(lib, name, rc, '%d < %d' % (need - 1, need), code=MPG_EWORKSPACE)


def _desc(state=0x1000, opt_steps=3):
    d = ops.SacAlphaStruct()
    d.state, d.target_entropy, d.opt_steps = state, -2.0, opt_steps
    d.lr[0], d.lr[1], d.lr[2] = 8e-5, 100000, 8e-6
    return d


@pytest.mark.parametrize('engine', ENGINES)
def test_alpha_update_refusals(engine):
    """each refusal has its own text, nothing is launched and the step counter stays where it was"""
    name = 'mpg_sac_alpha_update'
    with L.engine(engine):
        lib = L.lib()

        def call(d, g=FAKE, clip=1.0, do_clip=1, do_adam=1, skip=NULL, n_skip=0):
            return lib.mpg_sac_alpha_update(ctypes.byref(d) if d is not None else NULL, g, F(clip), I(do_clip), I(do_adam), skip, I(n_skip), NULL)
        refused(lib, name, call(None), 'null temperature struct')
        d = _desc(state=None)
        refused(lib, name, call(d), 'null temperature state')
        d = _desc()
        refused(lib, name, call(d, g=NULL), 'null gradient')
        refused(lib, name, call(d, do_clip=0, do_adam=0), 'nothing to do')
        for clip in (0.0, -1.0, float('nan')):
            refused(lib, name, call(d, clip=clip), 'clip norm')
        refused(lib, name, call(d, n_skip=3), '3 skip flags')
        refused(lib, name, call(d, skip=FAKE, n_skip=-1), 'skip flags')
        assert d.opt_steps == 3
        # the last field of the mirror sits where the library reads it: the refusal quotes the counter
        d = _desc(opt_steps=-7)
        refused(lib, name, call(d), '(-7)')
        assert d.opt_steps == -7


def _ctx(**kw):
    """a context that passes every check of mpg_sac_step_begin (FAKE pointers: a launch would fault)"""
    from mpg_amd.fused import TrainCtx
    c = TrainCtx()
    c.cfg = _cfg()
    c.learner_version, c.num_agent, c.sample_iters, c.sampling_interval, c.batch, c.world_size = 7, 8, 1, 10, 64, 1
    c.num_batch_reuse, c.delay_update, c.ring_capacity, c.clip = 1, 2, 1024, 1.0
    for k in ('params', 'targets', 'grad', 'ws0', 'ws1', 'scratch', 'norms', 'nonfinite', 'adam_m', 'adam_v', 'clip_scratch'):
        setattr(c, k, 0x1000)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


@pytest.mark.parametrize('engine', ENGINES)
def test_native_auto_step_refusals(engine):
    """those of mpg_sac_step_begin under the new name, plus a null struct, a null state and a target_entropy that is not finite; nothing
    is enqueued and no counter moves (ring_size 0: the one check after the refusals would stop a context that passed them all)"""
    with L.engine(engine):
        lib = L.lib()
        begin, end = 'mpg_sac_auto_step_begin', 'mpg_sac_auto_step_end'
        d = _desc()
        ref = ctypes.byref(d)
        refused(lib, begin, lib.mpg_sac_auto_step_begin(NULL, ref, I(0), NULL), 'null context')
        for kw, text in ((dict(learner_version=4), 'learner_version 7 (SAC) only (got 4)'), (dict(scratch=None), 'incomplete context'),
                         (dict(params=None), 'incomplete context'), (dict(prioritized=1), 'prioritized replay buffer'),
                         (dict(explore_sigma=0.1), 'explore_sigma')):
            c = _ctx(**kw)
            refused(lib, begin, lib.mpg_sac_auto_step_begin(ctypes.byref(c), ref, I(0), NULL), text)
            assert c.replay_times == 0 and c.learner_counter == 0 and c.noise_ctr == 0
        c = _ctx()
        refused(lib, begin, lib.mpg_sac_auto_step_begin(ctypes.byref(c), NULL, I(0), NULL), 'null temperature struct')
        refused(lib, begin, lib.mpg_sac_auto_step_begin(ctypes.byref(c), ctypes.byref(_desc(state=None)), I(0), NULL), 'null temperature state')
        for h in (float('nan'), float('inf')):
            bad = _desc()
            bad.target_entropy = h
            refused(lib, begin, lib.mpg_sac_auto_step_begin(ctypes.byref(c), ctypes.byref(bad), I(0), NULL), 'target_entropy must be finite')
        c.cfg.env_kind = 2
        refused(lib, begin, lib.mpg_sac_auto_step_begin(ctypes.byref(c), ref, I(0), NULL), 'InvertedDoublePendulum-v2')
        c = _ctx()
        refused(lib, begin, lib.mpg_sac_auto_step_begin(ctypes.byref(c), ref, I(1), NULL), 'empty replay ring')      # (iteration 1: no sampling)
        assert c.replay_times == 0 and c.learner_counter == 0 and d.opt_steps == 3
        # the step's second half
        refused(lib, end, lib.mpg_sac_auto_step_end(NULL, ref, I(0), NULL), 'null context')
        refused(lib, end, lib.mpg_sac_auto_step_end(ctypes.byref(_ctx(learner_version=2)), ref, I(0), NULL), 'learner_version 7 (SAC) only (got 2)')
        refused(lib, end, lib.mpg_sac_auto_step_end(ctypes.byref(c), NULL, I(0), NULL), 'null temperature struct')
        refused(lib, end, lib.mpg_sac_auto_step_end(ctypes.byref(c), ctypes.byref(_desc(state=None)), I(0), NULL), 'null temperature state')
        refused(lib, end, lib.mpg_sac_auto_step_end(ctypes.byref(_ctx(norms=None)), ref, I(0), NULL), 'incomplete context')
        refused(lib, end, lib.mpg_sac_auto_step_end(ctypes.byref(_ctx(clip=0.0)), ref, I(0), NULL), 'clip norm')
        c = _ctx()
        assert d.opt_steps == 3 and list(c.opt_steps) == [0, 0, 0]
        # the fixed-temperature entry point keeps its texts
        rc = lib.mpg_sac_step_begin(ctypes.byref(_ctx(prioritized=1)), F(0.03), I(0), NULL)
        refused(lib, 'mpg_sac_step_begin', rc, 'a prioritized replay buffer is not served (prioritized = 1)')
        refused(lib, 'mpg_sac_step_begin', lib.mpg_sac_step_begin(ctypes.byref(_ctx()), F(-1.0), I(0), NULL), 'alpha must be finite and not negative')


def test_ops_mirrors_the_struct():
    """mpg_sac_alpha_t { float* state; float target_entropy; float lr[3]; long long opt_steps; } under the C layout rules"""
    S = ops.SacAlphaStruct
    assert [f[0] for f in S._fields_] == ['state', 'target_entropy', 'lr', 'opt_steps']
    assert (S.state.offset, S.target_entropy.offset, S.lr.offset, S.opt_steps.offset) == (0, 8, 12, 24)
    assert ctypes.sizeof(S) == 32 and ops.ALPHA_STATE_FLOATS == 8
    assert (ops.ALPHA_LOG, ops.ALPHA_M, ops.ALPHA_V, ops.ALPHA_SNAPSHOT, ops.ALPHA_LOSS, ops.ALPHA_NORM, ops.ALPHA_NONFINITE) == tuple(range(7))


# ---- the Python layer on the host ----------------------------------------------------------------------------------------------
BASE = dict(obs_dim=6, act_dim=2, deterministic_policy=False, policy_out_activation='linear', device='cpu')


def test_policy_with_learned_temperature_on_the_host():
    from mpg_amd.policy import PolicyWithQs
    pw = PolicyWithQs(alpha='auto', target_entropy=-2., alpha_lr_schedule=[3e-4, 1000, 1e-5], **BASE)
    assert pw.auto_alpha and pw.alpha == 'auto' and pw.target_entropy == -2.0 and pw.names == ['Q1', 'Q2', 'policy']
    assert pw.alpha_state.shape == (8,) and not pw.alpha_state.any() and pw.alpha_opt_steps == 0          # log_alpha starts at 0
    assert [pw.alpha_desc.lr[i] for i in range(3)] == [np.float32(3e-4), 1000.0, np.float32(1e-5)]
    # get_weights: [Q1, Q2, policy, [log_alpha], Q1_t, Q2_t, policy_t], the reference's order
    w = pw.get_weights()
    assert [len(x) for x in w] == [6, 6, 6, 1, 6, 6, 6] and w[3][0].shape == ()
    other = PolicyWithQs(alpha='auto', target_entropy=-2., init_seed=3, **BASE)
    assert not torch.equal(other.params, pw.params)
    w[3][0] = np.float32(np.log(0.2))
    other.set_weights(w)
    assert torch.equal(other.params, pw.params) and torch.equal(other.targets, pw.targets)
    assert other.log_alpha.item() == np.float32(np.log(0.2))
    back = other.get_weights()
    assert all(torch.equal(torch.as_tensor(a), torch.as_tensor(b)) for x, y in zip(back, w) for a, b in zip(x, y))
    # state_dict round trip: the block and the counter
    other.alpha_state[1:3] = torch.tensor([0.25, 0.5])
    other.alpha_desc.opt_steps = 11
    sd = other.state_dict()
    assert set(sd) == {'params', 'targets', 'm', 'v', 'opt_steps', 'names', 'alpha_state', 'alpha_opt_steps'}
    third = PolicyWithQs(alpha='auto', target_entropy=-2., init_seed=5, **BASE)
    third.load_state_dict(sd)
    assert torch.equal(third.alpha_state, other.alpha_state) and third.alpha_opt_steps == 11 and torch.equal(third.params, other.params)
    # a flat gradient without the temperature's entry is refused before any launch
    with pytest.raises(ValueError, match="temperature's gradient"):
        third.apply_gradients(0, torch.zeros(int(third.offsets[-1])))


def test_fixed_temperature_stack_keeps_its_keys_and_weights_list():
    from mpg_amd.policy import PolicyWithQs
    pw = PolicyWithQs(alpha=0.03, **BASE)
    assert not pw.auto_alpha and pw.alpha == 0.03 and not hasattr(pw, 'alpha_state')
    assert set(pw.state_dict()) == {'params', 'targets', 'm', 'v', 'opt_steps', 'names'}
    assert [len(x) for x in pw.get_weights()] == [6] * 6


def test_refusals_of_the_python_layer():
    from mpg_amd.config import default_args
    from mpg_amd.learners import SACLearner
    from mpg_amd.policy import PolicyWithQs
    for h in (None, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='target_entropy'):
            PolicyWithQs(alpha='auto', target_entropy=h, **BASE)
    with pytest.raises(ValueError, match="'auto'"):
        PolicyWithQs(alpha='learned', target_entropy=-2., **BASE)
    with pytest.raises(ValueError, match='target_entropy'):
        SACLearner(PolicyWithQs, default_args('SAC', alpha='auto'), device='cpu')
    ln = SACLearner(PolicyWithQs, default_args('SAC', alpha='auto', target_entropy=-2.), device='cpu')
    pw = ln.policy_with_value
    assert ln.auto_alpha and ln.alpha == 'auto' and ln.n_grad == int(pw.offsets[-1]) + 1 and ln.flat.numel() == ln.n_grad + 16
    assert [pw.alpha_desc.lr[i] for i in range(3)] == [np.float32(8e-5), 100000.0, np.float32(8e-6)]
