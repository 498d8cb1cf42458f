#!/usr/bin/env python3
"""Every refusal of the one-launch rollout entry points (and the two one-launch steps beside them) as text, per engine, without a GPU:
`entry, case, rc, mpg_last_error()` for every single fault and every pair of faults below.  The check that a clean-up of the host side
changed no refusal, nor which of two answers:   python3 tools/refusal_matrix.py > before.txt; ...edit...; ... | diff before.txt -
Every pointer is fake, so every case carries at least one fault (asserted): nothing is ever launched on purpose.  CPU only."""
import ctypes
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpg_amd import _lib as L   # noqa: E402
from mpg_amd import ops         # noqa: E402

NULL, FAKE = ctypes.c_void_p(0), ctypes.c_void_p(0x1000)
I, F, U = ctypes.c_int, ctypes.c_float, ctypes.c_uint64
RING = ('ring_obs', 'ring_act', 'ring_rew', 'ring_obs2', 'ring_done')


def ring(a):
    return (I(a['capacity']), I(a['next_idx'])) + tuple(a[k] for k in RING) + (U(2), U(0), a['done_out'])


def worker(a, noise):       # the four worker rollouts: noise = (explore_sigma, seed, ctr) or the draw's (seed, ctr)
    return (a['policy'], I(a['n']), I(a['iters']), a['state'], a['obs_io']) + noise + (a['act_out'],) + ring(a) + (NULL,)


def evalr(a, tail):
    return (a['policy'], I(a['n']), I(a['steps']), a['state'], a['obs_io'], a['obs_traj'], a['act_traj'], a['rew_traj'], a['done_out']) + tail


def envr(a):
    return (a['policy'], I(a['rows']), I(a['n']), a['obs0'], a['act0'], a['rewards'], a['last_obs'], NULL)


NOISE, DRAW = (F(0.1), U(1), U(0)), (U(1), U(0))
WORKER_PTRS, EVAL_PTRS, ENV_PTRS = ('policy', 'state', 'obs_io', 'act_out') + RING, ('policy', 'state', 'obs_io', 'obs_traj', 'act_traj', 'rew_traj'), \
    ('policy', 'obs0', 'act0', 'rewards', 'last_obs')
# entry: (env kind, the arguments behind cfg from a case's values, its required pointers, its integers, sampled)
ENTRIES = {
    'mpg_worker_step': (0, lambda a: (a['policy'], I(a['n']), a['state'], a['obs_io']) + NOISE + (a['act_out'],) + ring(a)
                        + (NULL, I(0), NULL, NULL, NULL, NULL, NULL), WORKER_PTRS, 'ring', False),
    'mpg_worker_sample_step': (0, lambda a: (a['policy'], I(a['n']), a['state'], a['obs_io']) + DRAW + (a['act_out'], FAKE) + ring(a) + (NULL,),
                               WORKER_PTRS, 'ring', True),
    'mpg_worker_rollout': (0, lambda a: worker(a, NOISE), WORKER_PTRS, 'ring iters', False),
    'mpg_worker_rollout_pendulum': (1, lambda a: worker(a, NOISE), WORKER_PTRS, 'ring iters', False),
    'mpg_worker_sample_rollout': (0, lambda a: worker(a, DRAW), WORKER_PTRS, 'ring iters', True),
    'mpg_worker_sample_rollout_pendulum': (1, lambda a: worker(a, DRAW), WORKER_PTRS, 'ring iters', True),
    'mpg_eval_rollout': (0, lambda a: evalr(a, (FAKE, NULL)), EVAL_PTRS, 'steps', False),
    'mpg_eval_rollout_pendulum': (1, lambda a: evalr(a, (NULL,)), EVAL_PTRS, 'steps', False),
    'mpg_env_rollout': (0, envr, ENV_PTRS, 'rows', False),
    'mpg_env_rollout_pendulum': (1, envr, ENV_PTRS, 'rows', False),
}
OK = dict(n=8, iters=64, steps=200, rows=40, capacity=512, next_idx=0, done_out=FAKE)
ENV = {0: ('PathTracking-v0', 5, 17, 1), 1: ('InvertedPendulumConti-v0', 3, 5, 2)}      # env id, obs width below / above range, wrong act width


def faults(kind, ptrs, ints, sampled):
    """[(label, {argument or 'cfg.field': value})]: each is refused on its own; 'cfg' None is the null configuration"""
    _, lo, hi, act = ENV[kind]
    out = [('cfg=NULL', {'cfg': None})] + [('kind=%d' % k, {'cfg.env_kind': k}) for k in (1 - kind, 2, 3)]
    out += [('obs_dim=%d' % lo, {'cfg.obs_dim': lo}), ('obs_dim=%d' % hi, {'cfg.obs_dim': hi}), ('act_dim=%d' % act, {'cfg.act_dim': act})]
    out += [('tanh+range', {'cfg.policy_out_act': 1, 'cfg.action_range': 1.5})]
    if sampled:
        out += [('range=inf', {'cfg.action_range': float('inf')})]
    out += [('%s=NULL' % p, {p: NULL}) for p in ptrs]
    if 'ring' in ints:
        out += [('n=0', {'n': 0}), ('n=-4', {'n': -4}), ('capacity=n-1', {'capacity': 7}), ('next_idx=-1', {'next_idx': -1}),
                ('next_idx=capacity', {'next_idx': 512})]
    if 'iters' in ints:
        out += [('iters=0', {'iters': 0}), ('iters=1025', {'iters': 1025}), ('iters*n=capacity+1', {'capacity': 511}),
                ('iters*n=2^32', {'n': 1 << 22, 'iters': 1024, 'capacity': (1 << 31) - 1})]
    if 'steps' in ints:
        out += [('n=0', {'n': 0}), ('n=-4', {'n': -4}), ('steps=0', {'steps': 0}), ('steps=1025', {'steps': 1025})]
    if 'rows' in ints:
        out += [('rows=0', {'rows': 0}), ('rows=-4', {'rows': -4}), ('n=0', {'n': 0}), ('n=1025', {'n': 1025})]
    return out


def run(lib, entry, case):
    kind, args, ptrs, _, _ = ENTRIES[entry]
    real = [f for f in case if f[0] != 'done_out=NULL']
    assert real, (entry, case)                  # a case without a fault would be a launch on fake pointers
    cfg, a = ops.make_cfg(ENV[kind][0]), dict(OK, **{p: FAKE for p in ptrs + ENV_PTRS + EVAL_PTRS})
    for _, diff in case:
        for k, v in diff.items():
            if k == 'cfg':
                cfg = None
            elif k.startswith('cfg.'):
                if cfg is not None:
                    setattr(cfg, k[4:], v)
            else:
                a[k] = v
    rc = getattr(lib, entry)(ctypes.byref(cfg) if cfg is not None else NULL, *args(a))
    print('%s | %s | %s | %d | %s' % (L.current_engine(), entry, ' + '.join(f[0] for f in case), rc, lib.mpg_last_error().decode()))


if __name__ == '__main__':
    from mpg_amd import build as B
    B.build(verbose=False)
    for engine in sorted(L.ENGINES):
        with L.engine(engine):
            lib = L.lib()
            for entry, (kind, _, ptrs, ints, sampled) in ENTRIES.items():
                fs = faults(kind, ptrs, ints, sampled)
                for f in fs:
                    run(lib, entry, [f])
                for f, g in itertools.combinations(fs + [('done_out=NULL', {'done_out': NULL})], 2):
                    if not set(f[1]) & set(g[1]):            # two faults in one argument are one fault
                        run(lib, entry, [f, g])
