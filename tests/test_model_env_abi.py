"""mpg_model_env_reset, mpg_model_env_step, mpg_model_env_step_store_reset and mpg_worker_rollout_model at the drop-in boundary, without a
GPU: both libraries export them with the declared argument types, every refusal comes back as MPG_EINVAL under the entry point's own
name with a text of its own before any launch (every pointer is FAKE: a launch would fault), the two kinds that have a real env are
pointed to it, the ops wrappers check their arguments - and the real-env entry points keep refusing env kind 2."""
import ctypes
import re

import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops
from tests import abi_harness as H
from tests.abi_harness import ENGINES, F, FAKE, I, NULL, U64, MPG_EINVAL, _with, built  # noqa: F401 (built: the module's autouse fixture)

RESET, STEP, SSR, ROLL = 'mpg_model_env_reset', 'mpg_model_env_step', 'mpg_model_env_step_store_reset', 'mpg_worker_rollout_model'
PT_ID, PD_ID, DP_ID = 'PathTracking-v0', 'InvertedPendulumConti-v0', 'InvertedDoublePendulum-v2'
RING = ('ring_obs', 'ring_act', 'ring_rew', 'ring_obs2', 'ring_done')


@pytest.mark.parametrize('engine', ENGINES)
def test_both_libraries_export_the_entry_points(engine):
    lib = ctypes.CDLL(L.ENGINES[engine])
    for name in (RESET, STEP, SSR, ROLL):
        assert name in L.declared_symbols()
        assert hasattr(lib, name)
        assert L.declared_return_types()[name] == 'int'
    assert lib.mpg_abi_version() == 10           # functions were added: no layout or signature changed


def _declared(name):
    src = re.sub(r'/\*.*?\*/', '', open(L.HEADER).read(), flags=re.S)
    m = re.search(r'\bint\s+%s\s*\((.*?)\)\s*;' % name, src, flags=re.S)
    assert m, name
    return [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')]


RING_ARGS = ['int capacity', 'int next_idx', 'float* ring_obs', 'float* ring_act', 'float* ring_rew', 'float* ring_obs2', 'uint8_t* ring_done']


def test_declared_argument_types():
    assert _declared(RESET) == ['const mpg_cfg_t* cfg', 'int n', 'float* obs_io', 'int* age_io', 'const uint8_t* done_mask', 'uint64_t seed',
                                'uint64_t ctr', 'mpg_stream_t stream']
    assert _declared(STEP) == ['const mpg_cfg_t* cfg', 'int n', 'const float* obs', 'const float* act', 'int max_steps', 'int* age_io',
                               'float* obs_next', 'float* rew', 'uint8_t* done', 'mpg_stream_t stream']
    assert _declared(SSR) == ['const mpg_cfg_t* cfg', 'int n', 'float* obs_io', 'const float* act', 'int max_steps', 'int* age_io'] + RING_ARGS + \
        ['uint64_t seed', 'uint64_t ctr', 'uint8_t* done_out', 'mpg_stream_t stream']
    assert _declared(ROLL) == ['const mpg_cfg_t* cfg', 'const float* policy_params', 'int n', 'int iters', 'float* obs_io', 'int* age_io',
                               'int max_steps', 'float explore_sigma', 'uint64_t noise_seed', 'uint64_t noise_ctr', 'float* act_out'] + \
        RING_ARGS + ['uint64_t env_seed', 'uint64_t env_ctr', 'uint8_t* done_out', 'mpg_stream_t stream']


def _dp():
    return ops.make_cfg(DP_ID)


# what the cfg can get wrong, for every entry point
CFG_REFUSALS = [
    (lambda: ops.make_cfg(PT_ID), {}, 'env kind 0 has a real env (mpg_env_*'),
    (lambda: ops.make_cfg(PD_ID), {}, 'env kind 1 has a real env (mpg_env_*'),
    (lambda: _with(_dp(), env_kind=3), {}, 'unknown env kind 3'),
    (lambda: _with(_dp(), env_kind=-1), {}, 'unknown env kind -1'),
    (lambda: _with(_dp(), obs_dim=6), {}, 'the double-pendulum model env has obs_dim 11 (got 6)'),
    (lambda: _with(_dp(), obs_dim=12), {}, 'the double-pendulum model env has obs_dim 11 (got 12)'),
    (lambda: _with(_dp(), act_dim=2), {}, 'the double-pendulum model env has act_dim 1 (got 2)'),
    (lambda: ops.make_cfg(DP_ID, policy_out_activation='tanh', action_range=1.0), {}, 'tanh policy with an action range'),
]


def _sizes(nullable, pointers, ring):
    out = [(_dp, {k: NULL}, 'null pointer') for k in pointers]
    out += [(_dp, dict({k: NULL for k in nullable}, **{pointers[-1]: NULL}), 'null pointer')]      # a nullable one answers with the next thing wrong
    out += [(_dp, dict(n=v), 'no agents (n %d)' % v) for v in (0, -3)]
    if ring:
        out += [(_dp, dict(capacity=4), "the ring's capacity 4 is below n 5"),
                (_dp, dict(next_idx=-1), 'next_idx -1 outside [0, capacity 6000)'),
                (_dp, dict(next_idx=6000), 'next_idx 6000 outside [0, capacity 6000)')]
    return out


MAX_STEPS = [(_dp, dict(max_steps=-1), 'max_steps >= 0, 0 for no episode limit (got -1)')]

R_OK = dict(n=5, obs_io=FAKE, age_io=FAKE, done_mask=FAKE, seed=1, ctr=2)
R_REFUSALS = CFG_REFUSALS + _sizes(('done_mask',), ('obs_io', 'age_io'), False)

S_OK = dict(n=5, obs=FAKE, act=FAKE, max_steps=1000, age_io=FAKE, obs_next=FAKE, rew=FAKE, done=FAKE)
S_REFUSALS = CFG_REFUSALS + _sizes((), ('obs', 'act', 'age_io', 'obs_next', 'rew', 'done'), False) + MAX_STEPS

RING_OK = dict(capacity=6000, next_idx=17, **{k: FAKE for k in RING})
T_OK = dict(n=5, obs_io=FAKE, act=FAKE, max_steps=1000, age_io=FAKE, seed=1, ctr=2, done_out=FAKE, **RING_OK)
T_REFUSALS = CFG_REFUSALS + _sizes(('done_out',), ('obs_io', 'act', 'age_io') + RING, True) + MAX_STEPS

W_OK = dict(policy=FAKE, n=5, iters=512, obs_io=FAKE, age_io=FAKE, max_steps=1000, sigma=0.1, noise_seed=1, noise_ctr=2, act_out=FAKE,
            env_seed=3, env_ctr=4, done_out=FAKE, **RING_OK)
W_REFUSALS = CFG_REFUSALS + _sizes(('done_out',), ('policy', 'obs_io', 'age_io', 'act_out') + RING, True) + MAX_STEPS + [
    (_dp, dict(iters=0), 'iters >= 1 (got 0)'),
    (_dp, dict(iters=-2), 'iters >= 1 (got -2)'),
    (_dp, dict(iters=1025, capacity=10000), 'iters <= 1024 (got 1025)'),
    (_dp, dict(iters=1024, capacity=5119), "iters * n = 5120 transitions do not fit the ring's capacity 5119"),
    (_dp, dict(iters=1201), "iters <= 1024 (got 1201)"),                 # (the iteration bound answers before the ring's size)
]


def _ring(a):
    return [I(a['capacity']), I(a['next_idx'])] + [a[k] for k in RING]


def _call_reset(lib, cfg_ref, a):
    return lib.mpg_model_env_reset(cfg_ref, I(a['n']), a['obs_io'], a['age_io'], a['done_mask'], U64(a['seed']), U64(a['ctr']), NULL)


def _call_step(lib, cfg_ref, a):
    return lib.mpg_model_env_step(cfg_ref, I(a['n']), a['obs'], a['act'], I(a['max_steps']), a['age_io'], a['obs_next'], a['rew'], a['done'],
                                  NULL)


def _call_ssr(lib, cfg_ref, a):
    return lib.mpg_model_env_step_store_reset(cfg_ref, I(a['n']), a['obs_io'], a['act'], I(a['max_steps']), a['age_io'], *_ring(a),
                                              U64(a['seed']), U64(a['ctr']), a['done_out'], NULL)


def _call_roll(lib, cfg_ref, a):
    return lib.mpg_worker_rollout_model(cfg_ref, a['policy'], I(a['n']), I(a['iters']), a['obs_io'], a['age_io'], I(a['max_steps']),
                                        F(a['sigma']), U64(a['noise_seed']), U64(a['noise_ctr']), a['act_out'], *_ring(a),
                                        U64(a['env_seed']), U64(a['env_ctr']), a['done_out'], NULL)


ENTRIES = [(RESET, _call_reset, R_OK, R_REFUSALS), (STEP, _call_step, S_OK, S_REFUSALS), (SSR, _call_ssr, T_OK, T_REFUSALS),
           (ROLL, _call_roll, W_OK, W_REFUSALS)]

test_reset_refusals = H.refusal_test(RESET, R_REFUSALS, R_OK, _call_reset)
test_step_refusals = H.refusal_test(STEP, S_REFUSALS, S_OK, _call_step)
test_step_store_reset_refusals = H.refusal_test(SSR, T_REFUSALS, T_OK, _call_ssr)
test_worker_rollout_refusals = H.refusal_test(ROLL, W_REFUSALS, W_OK, _call_roll)


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('name, call, ok', [e[:3] for e in ENTRIES], ids=[e[0] for e in ENTRIES])
def test_a_null_configuration_is_refused(engine, name, call, ok):
    H.null_configuration_refused(engine, name, call, ok)


@pytest.mark.parametrize('name, at_least', [(RESET, 11), (STEP, 11), (SSR, 11), (ROLL, 14)])
def test_every_refusal_has_a_text_of_its_own(name, at_least):
    H.refusal_texts_are_unique(name, 'model_rollout.hip', at_least)


def test_every_listed_condition_is_in_the_tables():
    """the conditions include/mpg_hip.h lists for the entry points are the ones the tables above provoke (null configuration: its own
    test)"""
    for name, _, _, table in ENTRIES:
        seen = set(t for _, _, t in table)
        for stem in ('has a real env', 'unknown env kind', 'obs_dim 11', 'act_dim 1', 'tanh policy with an action range', 'null pointer',
                     'no agents'):
            assert any(stem in t for t in seen), (name, stem)
        assert any('max_steps >= 0' in t for t in seen) == (name != RESET), name
        assert any("ring's capacity" in t for t in seen) == any('next_idx' in t for t in seen) == (name in (SSR, ROLL)), name
    seen = set(t for _, _, t in W_REFUSALS)
    assert any('iters >= 1' in t for t in seen) and any('iters <= 1024' in t for t in seen) and any('do not fit' in t for t in seen)


@pytest.mark.parametrize('engine', ENGINES)
def test_the_real_env_entry_points_keep_refusing_env_kind_2(engine):
    """kind 2 is served by the four entry points here alone: the first thing they refuse of the double pendulum's cfg is what is wrong
    behind the cfg, while mpg_env_*, the worker rollouts on the real envs and mpg_eval_rollout answer it as before"""
    with L.engine(engine):
        lib = L.lib()
        cfg = _dp()
        for name, call, ok, _ in ENTRIES:
            assert call(lib, ctypes.byref(cfg), dict(ok, age_io=NULL)) == MPG_EINVAL
            assert lib.mpg_last_error().decode() == name + ': null pointer'
        rc = lib.mpg_env_step(I(2), I(5), I(11), FAKE, FAKE, FAKE, FAKE, FAKE, NULL, NULL)
        assert rc == MPG_EINVAL and 'MuJoCo' in lib.mpg_last_error().decode()
        rc = lib.mpg_env_reset(I(2), I(5), I(11), FAKE, NULL, U64(0), U64(0), FAKE, NULL)
        assert rc == MPG_EINVAL and 'MuJoCo' in lib.mpg_last_error().decode()
        for entry in ('mpg_worker_rollout', 'mpg_worker_rollout_pendulum'):
            rc = getattr(lib, entry)(ctypes.byref(cfg), FAKE, I(5), I(4), FAKE, FAKE, F(0.), U64(0), U64(0), FAKE, I(100), I(0), FAKE, FAKE, FAKE,
                                     FAKE, FAKE, U64(0), U64(0), NULL, NULL)
            assert rc == MPG_EINVAL and 'MuJoCo' in lib.mpg_last_error().decode(), entry
        rc = lib.mpg_eval_rollout(ctypes.byref(cfg), FAKE, I(5), I(25), FAKE, FAKE, FAKE, FAKE, FAKE, NULL, NULL, NULL)
        assert rc == MPG_EINVAL and 'MuJoCo' in lib.mpg_last_error().decode()


def test_a_refusal_reaches_python_as_mpg_error():
    cfg = _dp()
    with pytest.raises(L.MpgError, match=ROLL + ': iters <= 1024'):
        L.call(ROLL, ctypes.byref(cfg), FAKE, I(1), I(1025), FAKE, FAKE, I(0), F(0.), U64(0), U64(0), FAKE, I(2000), I(0), FAKE, FAKE, FAKE, FAKE,
               FAKE, U64(0), U64(0), NULL, NULL)
    with pytest.raises(L.MpgError, match=STEP + ': no agents'):
        L.call(STEP, ctypes.byref(cfg), I(0), FAKE, FAKE, I(0), FAKE, FAKE, FAKE, FAKE, NULL)


# ---- the ops wrappers' own argument checks (before the library is called: host tensors never reach it) ----------------------------
def test_ops_wrappers_check_their_shapes():
    cfg = _dp()
    obs, act, age = torch.zeros(5, 11), torch.zeros(5, 1), torch.zeros(5, dtype=torch.int32)
    with pytest.raises(ValueError, match=r'model_env_step: obs \(5, 6\), age \(5,\) and act \(5, 1\) are not \[n, 11\], \[n\] and \[n, 1\]'):
        ops.model_env_step(cfg, torch.zeros(5, 6), act, age)
    with pytest.raises(ValueError, match='model_env_step: obs'):
        ops.model_env_step(cfg, obs, torch.zeros(5, 2), age)
    with pytest.raises(ValueError, match='model_env_step: obs'):
        ops.model_env_step(cfg, obs, act, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match=r'model_env_reset: obs \(5, 11\), age \(4,\) are not \[n, 11\], \[n\]'):
        ops.model_env_reset(cfg, obs, torch.zeros(4, dtype=torch.int32), 0, 0)
    ring = (torch.zeros(8, 11), torch.zeros(8, 1), torch.zeros(8), torch.zeros(8, 11), torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(ValueError, match='model_env_step_store_reset: obs'):
        ops.model_env_step_store_reset(cfg, obs, torch.zeros(4, 1), age, 0, ring, 8, 0, 0, 0)
