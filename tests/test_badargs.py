"""Error behaviour of the C ABI (include/mpg_hip.h: "0 on success, an MPG_ERR_* code otherwise, text behind mpg_last_error()").
Every entry point validates its arguments BEFORE it touches the device, so these refusals can be checked without a GPU: a bad
argument must come back as a non-zero code with a message that names the entry point - never as a crash, and never as a launch.
(The reference's counterparts fail with Python exceptions - an assert in segment_tree.py:40, numpy shape errors in buffer.py -
which is what mpg_amd._lib.call turns these codes into.)"""
import ctypes

import pytest

from mpg_amd import _lib as L

NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(0x1000)          # a non-null pointer that is never dereferenced: the call must be refused before any launch
I, U64, F, SZ = ctypes.c_int, ctypes.c_uint64, ctypes.c_float, ctypes.c_size_t

CASES = [
    # (entry point, arguments, what is wrong)
    ('mpg_env_step', (I(7), I(16), I(6), FAKE, FAKE, FAKE, FAKE, FAKE, NULL, NULL), 'unknown env kind'),
    ('mpg_env_step', (I(0), I(0), I(6), FAKE, FAKE, FAKE, FAKE, FAKE, NULL, NULL), 'no agents'),
    ('mpg_env_step', (I(0), I(16), I(5), FAKE, FAKE, FAKE, FAKE, FAKE, NULL, NULL), 'obs_dim below the six base entries'),
    ('mpg_env_step', (I(0), I(16), I(6 + 11), FAKE, FAKE, FAKE, FAKE, FAKE, NULL, NULL), 'more look-ahead entries than MPG_ENV_MAX_FUTURE'),
    ('mpg_env_step', (I(0), I(16), I(6), NULL, FAKE, FAKE, FAKE, FAKE, NULL, NULL), 'null state'),
    ('mpg_env_reset', (I(0), I(16), I(6), FAKE, NULL, U64(1), U64(0), NULL, NULL), 'null obs'),
    ('mpg_env_reset_from_obs', (I(0), I(16), I(6), FAKE, NULL, NULL), 'null init_obs'),
    ('mpg_env_step_store_reset', (I(0), I(64), I(6), FAKE, FAKE, I(32), I(0), FAKE, FAKE, FAKE, FAKE, FAKE, U64(1), U64(0), FAKE, NULL, NULL),
     'ring smaller than one batch of transitions'),
    ('mpg_env_step_store_reset', (I(0), I(16), I(6), FAKE, FAKE, I(64), I(64), FAKE, FAKE, FAKE, FAKE, FAKE, U64(1), U64(0), FAKE, NULL, NULL),
     'next_idx outside the ring'),
    ('mpg_sum_slots', (NULL, I(2), I(64), FAKE, NULL), 'null slots'),
    ('mpg_sum_slots', (FAKE, I(0), I(64), FAKE, NULL), 'no slots'),
    ('mpg_sum_slots_strided', (FAKE, I(2), SZ(32), I(64), FAKE, NULL), 'slice longer than the slot stride'),
    ('mpg_replay_add', (I(64), I(0), I(128), I(6), I(2), FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, NULL), 'more rows than the ring holds'),
    ('mpg_replay_add', (I(64), I(-1), I(16), I(6), I(2), FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, NULL), 'negative ring position'),
    ('mpg_replay_gather', (I(16), FAKE, I(17), I(2), FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, NULL, NULL), 'obs_dim beyond 16'),
    ('mpg_replay_gather', (I(16), NULL, I(6), I(2), FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, NULL, NULL), 'null index array'),
    ('mpg_uniform_indices', (I(0), I(16), U64(1), U64(1), FAKE, NULL), 'empty storage (the reference: randint(0, -1) raises)'),
    ('mpg_uniform_indices', (I(100), I(16), U64(1), U64(1), NULL, NULL), 'null output'),
    ('mpg_per_init', (FAKE, FAKE, FAKE, I(1000), NULL), 'capacity not a power of two (segment_tree.py:40 asserts the same)'),
    ('mpg_per_init', (NULL, FAKE, FAKE, I(1024), NULL), 'null tree'),
    ('mpg_normal_fill', (I(0), U64(1), U64(1), FAKE, NULL), 'nothing to fill'),
    ('mpg_mlp_forward', (NULL, I(6), I(4), I(2), I(0), I(16), FAKE, NULL, I(0), FAKE, NULL, NULL), 'null parameters'),
    ('mpg_mlp_forward', (FAKE, I(3), I(4), I(2), I(0), I(16), FAKE, NULL, I(0), FAKE, NULL, NULL), 'a network shape that is not built'),
    ('mpg_mlp_forward', (FAKE, I(6), I(4), I(2), I(0), I(0), FAKE, NULL, I(0), FAKE, NULL, NULL), 'no rows'),
    ('mpg_policy_action', (NULL, FAKE, I(16), FAKE, F(0.0), U64(0), U64(0), FAKE, NULL), 'null configuration'),
    ('mpg_clip_by_global_norm', (FAKE, FAKE, I(0), F(3.0), FAKE, NULL, NULL, NULL), 'no segments'),
    ('mpg_prof_read', (NULL, I(0), NULL, NULL), 'null profiler handle'),
]


SHARED = {'a network shape that is not built': 'unsupported network shape', 'null parameters': 'launch_forward', 'no rows': 'launch_forward'}


@pytest.mark.parametrize('name,args,why', CASES, ids=['%s-%s' % (c[0], c[2].split(' (')[0].replace(' ', '_')) for c in CASES])
def test_bad_argument_is_refused_with_a_code_and_a_message(name, args, why):
    lib = L.lib()
    rc = getattr(lib, name)(*args)
    assert rc != 0, '%s accepted: %s' % (name, why)
    msg = lib.mpg_last_error().decode()
    # the text names the entry point (or, for a refusal inside a shared launcher, what was refused)
    assert msg and (name.replace('mpg_', '') in msg.replace('mpg_', '') or SHARED.get(why, '\0') in msg), (name, msg)
    with pytest.raises(L.MpgError, match=name):          # ... and the binding raises (no silent fallback anywhere)
        L.call(name, *args)


def test_the_message_belongs_to_the_calling_thread():
    """mpg_last_error() is thread-local (the one piece of state the library keeps): a refusal in another thread
    does not replace this thread's text"""
    import threading
    lib = L.lib()
    assert lib.mpg_sum_slots(NULL, I(2), I(64), FAKE, NULL) != 0
    mine = lib.mpg_last_error().decode()
    seen = {}

    def other():
        assert lib.mpg_uniform_indices(I(0), I(16), U64(1), U64(1), FAKE, NULL) != 0
        seen['msg'] = lib.mpg_last_error().decode()
    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert 'uniform_indices' in seen['msg'] and 'sum_slots' in mine
    assert lib.mpg_last_error().decode() == mine


# ---- workspaces: every entry point that takes one refuses a buffer one byte short of its own query ----
MPG_EWORKSPACE = -1001
ROWS = 4096
SEL2, W2 = (I * 2)(0, 25), (F * 2)(0.3, 0.7)      # `select` / `w` are read on the host before the size check: real arrays


def _pt(obs_dim=6):
    from mpg_amd import ops
    return ops.make_cfg('PathTracking-v0', obs_dim=obs_dim)


def _rollout_pg(M, asp):
    return lambda ws, nb: (FAKE, FAKE, I(ROWS), I(M), I(25), SEL2, I(2), W2, FAKE, NULL, U64(1), U64(0), F(1.0 / ROWS), I(asp), FAKE,
                           FAKE, FAKE, ws, nb, NULL)


WS_CASES = [
    # (entry point, its query, cfg, the query's sizes after cfg, the entry point's arguments after cfg)
    ('mpg_q_targets', 'mpg_q_targets', 6, (ROWS,),
     lambda ws, nb: (FAKE, FAKE, FAKE, I(ROWS), FAKE, FAKE, NULL, F(0.2), F(0.5), FAKE, ws, nb, NULL)),
    ('mpg_td3_targets', 'mpg_q_targets', 6, (ROWS,),
     lambda ws, nb: (FAKE, FAKE, FAKE, I(ROWS), FAKE, FAKE, FAKE, F(0.2), F(0.5), FAKE, FAKE, ws, nb, NULL)),
    ('mpg_nstep_targets', 'mpg_q_targets', 6, (ROWS,),
     lambda ws, nb: (FAKE, FAKE, I(ROWS), I(5), FAKE, FAKE, FAKE, ws, nb, NULL)),
    ('mpg_q_loss_grad', 'mpg_q_loss_grad', 6, (ROWS,),
     lambda ws, nb: (FAKE, I(ROWS), FAKE, FAKE, FAKE, F(1.0 / ROWS), FAKE, FAKE, NULL, ws, nb, NULL)),
    ('mpg_td3_policy_grad', 'mpg_td3_policy_grad', 6, (ROWS,),
     lambda ws, nb: (FAKE, FAKE, FAKE, I(ROWS), FAKE, F(1.0 / ROWS), FAKE, FAKE, FAKE, ws, nb, NULL)),
    ('mpg_rollout_pg', 'mpg_rollout_pg', 6, (ROWS, 1, 25, 2, 0), _rollout_pg(1, 0)),
    ('mpg_rollout_pg', 'mpg_rollout_pg', 6, (ROWS, 1, 25, 2, 1), _rollout_pg(1, 1)),          # with the thin partials
    ('mpg_rollout_pg', 'mpg_rollout_pg', 9, (ROWS, 3, 25, 2, 0), _rollout_pg(3, 0)),          # with the wide inputs
    ('mpg_rollout_q_target', 'mpg_rollout_q_target', 6, (ROWS,),
     lambda ws, nb: (FAKE, FAKE, I(ROWS), I(25), FAKE, FAKE, NULL, U64(1), U64(0), FAKE, ws, nb, NULL)),
    ('mpg_rollout_q_estimation', 'mpg_rollout_q_estimation', 6, (ROWS, 1, 2),
     lambda ws, nb: (FAKE, FAKE, I(ROWS), I(1), SEL2, I(2), FAKE, FAKE, NULL, U64(1), U64(0), FAKE, ws, nb, NULL)),
    ('mpg_mpg_gradients', 'mpg_mpg_gradients', 6, (ROWS, 1, 25, 2, 2),
     lambda ws, nb: (I(2), FAKE, FAKE, I(ROWS), FAKE, FAKE, FAKE, FAKE, NULL, I(1), I(25), SEL2, I(2), W2, NULL, U64(1), U64(0),
                     F(1.0 / ROWS), FAKE, FAKE, FAKE, NULL, NULL, ws, nb, NULL)),
]


@pytest.mark.parametrize('name,query,obs_dim,sizes,args', WS_CASES,
                         ids=['%s-od%d-%s' % (c[0], c[2], 'x'.join(str(v) for v in c[3])) for c in WS_CASES])
def test_workspace_one_byte_short_is_refused_with_both_sizes(name, query, obs_dim, sizes, args):
    lib = L.lib()
    cfg = _pt(obs_dim)
    q = getattr(lib, query + '_workspace_bytes')
    need = q(ctypes.byref(cfg), *[I(v) for v in sizes])
    assert need > 0
    rc = getattr(lib, name)(ctypes.byref(cfg), *args(FAKE, SZ(need - 1)))
    msg = lib.mpg_last_error().decode()
    assert rc == MPG_EWORKSPACE, (name, rc, msg)
    assert msg.startswith(name + ':') and 'workspace too small' in msg and '%d < %d' % (need - 1, need) in msg, msg
    # the query itself answers 0 for what every entry point refuses: tanh output with an action range, no rows
    from mpg_amd import ops
    refused = ops.make_cfg('PathTracking-v0', obs_dim=obs_dim, policy_out_activation='tanh', action_range=1.0)
    assert q(ctypes.byref(refused), *[I(v) for v in sizes]) == 0
    assert q(ctypes.byref(cfg), I(0), *[I(v) for v in sizes[1:]]) == 0


def test_two_critics_with_four_slices_are_refused_before_any_launch():
    """mpg_mpg_gradients reduces n_q losses + 2 sums per slice in 8 jobs: two critics with MAXSEL = 4 slices do not fit.  The workspace
    query answers 0 and the entry point MPG_EINVAL with a message that says why - from the host-side checks (every pointer is FAKE:
    a launch would fault).  One critic with four slices (9 jobs) is refused alike; three slices are served with either count."""
    lib = L.lib()
    cfg = _pt()
    q = lib.mpg_mpg_gradients_workspace_bytes
    assert q(ctypes.byref(cfg), I(ROWS), I(1), I(25), I(4), I(2)) == 0
    assert q(ctypes.byref(cfg), I(ROWS), I(1), I(25), I(4), I(1)) == 0
    assert q(ctypes.byref(cfg), I(ROWS), I(1), I(25), I(3), I(1)) > 0 and q(ctypes.byref(cfg), I(ROWS), I(1), I(25), I(3), I(2)) > 0
    sel4, w4 = (I * 4)(0, 1, 24, 25), (F * 4)(0.2, 0.3, 0.4, 0.5)
    rc = lib.mpg_mpg_gradients(ctypes.byref(cfg), I(2), FAKE, FAKE, I(ROWS), FAKE, FAKE, FAKE, FAKE, NULL, I(1), I(25), sel4, I(4), w4, NULL,
                               U64(1), U64(0), F(1.0 / ROWS), FAKE, FAKE, FAKE, NULL, NULL, FAKE, SZ(1 << 40), NULL)
    msg = lib.mpg_last_error().decode()
    assert rc == -1000, (rc, msg)                # MPG_EINVAL
    assert msg.startswith('mpg_mpg_gradients:') and 'too many statistics' in msg, msg
