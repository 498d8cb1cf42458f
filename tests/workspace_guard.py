"""The other side of the workspace contract (include/mpg_hip.h: "`*_workspace_bytes` bytes, caller-owned"): every learner entry point
run in EXACTLY the bytes its query reports, between two guard regions, over a workspace whose every byte was set beforehand - to 0xFF
(every float32 word a NaN) or to 0x00.  tests/test_badargs.py and the *_abi.py files check that one byte less is refused; this helper
is for showing that the reported size is enough, that nothing is written outside it, and that no result depends on what it held.

guarded() replaces mpg_amd.ops.workspace (ops._ws looks it up as a module global), check() looks at what the calls left, CASES is the
table of calls.  No test functions here: tests/test_workspace_guard.py (CPU) and tests/test_workspace_guard_gpu.py use it.

Integer arrays: read before the first GPU run - every Arena::take of the workspace descriptions in csrc/learner_api.hip (q_targets_ws,
q_loss_ws, policy_grad_ws, policy_sample_ws, sac_targets_ws) and csrc/rollout_kernels.hip (pg_ws, ampc_ws, rollout_q_ws, mg_ws) takes
floats, and mg_fallback_ws splits its bytes (Arena::bytes) between the workspaces of mpg_q_targets / mpg_q_loss_grad and of
mpg_rollout_pg, which are two of those.  So no workspace of these entry points holds an index that 0xFF would turn into -1, and every
case runs under both patterns.

Row counts (the weight gradient works on groups of 16 rows, in chunks of groups; wgrad_chunks() restates the chunking of
csrc/mlp_wgrad.h and tests/test_workspace_guard.py asserts what the table says under the constants in force):

    rows   what it reaches
    1      one group with 15 dead rows
    17     a full group and a group with one live row
    272    17 groups; the multi-job launch of mpg_mpg_gradients: 2 groups per chunk, 9 chunks, the last one holds one group
    1037   65 groups; the single-job launch: 2 per chunk, 33 chunks, the last one holds one ragged group
    2051   129 groups; k_wgrad_w2 of the split engine: 2 per chunk, 65 chunks, the last one holds one ragged group

2051 goes to the entry points whose weight-gradient launch passes no_thin at a width backward_takes_thin (csrc/mlp_kernels.hip) accepts:
mpg_q_loss_grad at K = 0 (critic input 8 wide, one output), mpg_td3_policy_grad and mpg_dpg_policy_grad at K = 0 (policy input 6 wide,
two used outputs), the squashed SAC policy gradient on the pendulum (4 wide, two used outputs).  The plain and PathTracking SAC forms use
four outputs and every K > 0 form a wide input: no thin form is built for them.  The all-steps sweeps (mpg_rollout_pg with
all_steps_param_grad, mpg_ampc_pg) take rows * M % 16 == 0 only and hand the weight gradient (n + 1) * rows * M rows; with the policy's
packed image bound at K = 0, M = 1 (the THIN reverse sweep) that launch is the k_wgrad_w2 form too.  Their row counts: 16 (one group per
step, one thin partial of 256), 1040 (260 groups: k_wgrad_w2 cuts 3 per chunk, 87 chunks, the last one holds 2) and 1056 (264 groups:
the single-job launch cuts 5 per chunk, 53 chunks, the last one holds 4).  The fused path of mpg_mpg_gradients takes rows % 16 == 0 as
well: 16, 272 and 1056 (66 groups: the multi-job launch cuts 5 per chunk, 14 chunks, the last one holds 1).  Horizon 3 everywhere but
one mpg_rollout_pg case (17 rows) and one mpg_ampc_pg case (32 rows: it refuses 17) at horizon 25."""
import collections
import contextlib
import functools
import os
import re

import numpy as np
import torch

from mpg_amd import ops
from tests import dp_oracle as DP
from tests.golden_inputs import mlp_weights_flat, reset_law_obs
from tests.model_edge_inputs import pendulum_wide_obs

GUARD = 1 << 20
NAN_FILL, ZERO_FILL = 0xFF, 0x00
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
PD = 'InvertedPendulumConti-v0'
DEV = 'cuda'

HandOut = collections.namedtuple('HandOut', 'buffer offset nb slot')


def all_ones_word_is_nan():
    """the float32 word 0xFFFFFFFF - what the 0xFF pattern leaves in every float of a workspace - is a NaN"""
    return bool(torch.tensor([0xFF] * 4, dtype=torch.uint8).view(torch.float32).isnan().all())


class Record(object):
    """what one guarded block handed out: (buffer, offset, nb, slot) per (device, slot, nb)"""

    def __init__(self, fill, misalign):
        self.fill, self.misalign = int(fill), int(misalign)
        self.handouts = []
        self._views = {}


@contextlib.contextmanager
def guarded(monkeypatch, fill, misalign=0, device=None):
    """For the duration, mpg_amd.ops.workspace(device, nb, slot) hands out the view [GUARD + misalign : GUARD + misalign + nb] of a uint8
    tensor of GUARD + nb + misalign + GUARD bytes, every byte of it `fill`: numel() is exactly nb, data_ptr() what the entry point gets.
    One buffer per (device, slot, nb): a second request with that key gets the same view, as the stock path's would.  device: where to
    allocate whatever the caller names (the CPU tests of this helper).  Yields the Record for check()."""
    assert all_ones_word_is_nan()
    rec = Record(fill, misalign)

    def workspace(dev, nbytes, slot=0):
        dev = device if device is not None else dev
        nb = int(nbytes)
        key = (str(dev), slot, nb)
        if key not in rec._views:
            buf = torch.full((GUARD + nb + rec.misalign + GUARD,), rec.fill, dtype=torch.uint8, device=dev)
            off = GUARD + rec.misalign
            view = buf[off:off + nb]
            assert view.is_contiguous() and view.numel() == nb and view.data_ptr() == buf.data_ptr() + off
            if buf.is_cuda:        # the allocator's blocks are 512-byte aligned: `misalign` is the view's offset from a 256-byte line
                assert view.data_ptr() % 256 == rec.misalign % 256, (view.data_ptr(), rec.misalign)
            rec._views[key] = view
            rec.handouts.append(HandOut(buf, off, nb, slot))
        return rec._views[key]

    with monkeypatch.context() as m:
        m.setattr(ops, 'workspace', workspace)
        yield rec


def check(record, what='', used=True):
    """Both guard regions of every hand-out still hold `fill` in every byte, its interior no longer does (the kernels used this buffer),
    and there was a hand-out at all.  Compared where the buffers live, with one synchronisation.  used=False: a call that takes a
    workspace and, by its code, leaves it alone - then the interior must still hold the fill."""
    assert record.handouts, (what, 'no workspace was asked for: the call did not go through ops.workspace')
    flags = []
    for h in record.handouts:
        lo, mid, hi = h.buffer[:h.offset], h.buffer[h.offset:h.offset + h.nb], h.buffer[h.offset + h.nb:]
        assert lo.numel() == GUARD + record.misalign and hi.numel() == GUARD and mid.numel() == h.nb
        flags.append(torch.stack([(lo == record.fill).all(), (hi == record.fill).all(), (mid == record.fill).all()]))
    flags = torch.stack(flags).cpu().numpy()
    for h, (lo_ok, hi_ok, untouched) in zip(record.handouts, flags):
        where = (what, 'slot %d, %d bytes, fill 0x%02X, misalign %d' % (h.slot, h.nb, record.fill, record.misalign))
        assert lo_ok, where + ('the guard in front of the workspace was written',)
        assert hi_ok, where + ('the guard behind the workspace was written: a kernel writes past the queried size',)
        if used:
            assert not untouched, where + ('the workspace still holds the fill in every byte: the call did not use it',)
        else:
            assert untouched, where + ('a call that is described as leaving its workspace alone wrote to it',)


def unwritten_words(record):
    """[(slot, float words of the workspace, words that still hold the 0xFF pattern)] after a call over a NAN_FILL workspace: how much of
    it the call never wrote.  A figure to report, not to assert (a kernel may write a NaN of that very pattern; none does here)."""
    assert record.fill == NAN_FILL
    out = []
    for h in record.handouts:
        words = h.buffer[h.offset:h.offset + h.nb // 4 * 4].view(torch.int32)
        out.append((h.slot, words.numel(), int((words == -1).sum().item())))
    return out


def backward_takes_thin(in_dim, ou):
    """csrc/mlp_kernels.hip backward_takes_thin, evaluated from its source text: the (input width, used outputs) at which the thin
    parameter gradients can ride in the backward launch and the weight-gradient launch is the dW2-only form"""
    src = open(os.path.join(ROOT, 'mpg_amd', 'csrc', 'mlp_kernels.hip')).read()
    m = re.search(r'bool backward_takes_thin\(int in_dim, int ou\) \{(?:\s*//[^\n]*\n)*\s*return ([^;]+);\s*\}', src)
    assert m, 'backward_takes_thin is no longer one return statement: restate how it is read here'
    expr = m.group(1)
    assert re.fullmatch(r'(?:in_dim|ou|\d+|<=|>=|==|!=|<|>|&&|\|\||!|\(|\)|\s)+', expr), expr
    expr = re.sub(r'!(?!=)', ' not ', expr.replace('&&', ' and ').replace('||', ' or '))
    return bool(eval(expr, {'__builtins__': {}}, {'in_dim': int(in_dim), 'ou': int(ou)}))


# ---- the chunking of a weight-gradient job (csrc/mlp_wgrad.h), restated --------------------------------------------------------
def wgrad_constants():
    """{name: value} of the MPG_WGRAD_* defaults of csrc/mlp_wgrad.h (the build sets none of them: mpg_amd/build.py)"""
    src = open(os.path.join(ROOT, 'mpg_amd', 'csrc', 'mlp_wgrad.h')).read()
    out = {k: int(v) for k, v in re.findall(r'^#define (MPG_WGRAD_[A-Z0-9_]+) (\d+)', src, flags=re.M)}
    assert {'MPG_WGRAD_MAX_CHUNKS', 'MPG_WGRAD_MAX_CHUNKS_SINGLE', 'MPG_WGRAD_MAX_CHUNKS_W2', 'MPG_WGRAD_W2_MIN_GROUPS'} <= set(out), out
    return out


def wgrad_chunks(rows, form, consts=None):
    """(groups per chunk, chunks, groups in the last chunk) of a weight-gradient job over `rows` rows.  form: 'multi' - the multi-job
    launch of mpg_mpg_gradients (wgrad_groups_per_chunk), 'single' - a launch that carries one network's job
    (wgrad_groups_per_chunk(., true)), 'w2' - the dW2-only launch of the split engine (wgrad_groups_per_chunk_w2)."""
    c = consts or wgrad_constants()
    ngroups = (rows + 15) // 16
    if form == 'w2':
        mc = c['MPG_WGRAD_MAX_CHUNKS_W2']
        gp = (ngroups + mc - 1) // mc
        if ngroups >= 4096 and gp < c['MPG_WGRAD_W2_MIN_GROUPS']:
            gp = c['MPG_WGRAD_W2_MIN_GROUPS']
    else:
        mc = c['MPG_WGRAD_MAX_CHUNKS_SINGLE' if form == 'single' else 'MPG_WGRAD_MAX_CHUNKS']
        gp = (ngroups + mc - 1) // mc
    gp = max(gp, 1)
    nch = (ngroups + gp - 1) // gp
    return gp, nch, ngroups - (nch - 1) * gp


# (rows handed to the weight gradient, form, (groups per chunk, chunks, groups in the last chunk)): what the module docstring's table says
RAGGED_CHUNKS = [(272, 'multi', (2, 9, 1)), (1037, 'single', (2, 33, 1)), (2051, 'w2', (2, 65, 1)),
                 (4 * 1040, 'w2', (3, 87, 2)), (4 * 1056, 'single', (5, 53, 4)), (1056, 'multi', (5, 14, 1))]


# ---- inputs: seeded draws, computed once per shape and never written to ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(env, K, rows, M=1, n=3):
    """numpy float32 arrays of one configuration: networks (policy, two critics), a replay batch (obs, act, rew, obs2), targets y,
    n-step rewards [n, rows], model noise eps [n, rows * M], two sets of head draws [rows, act_dim]"""
    rng = np.random.Generator(np.random.PCG64(100000 * ('pt', 'pd', 'dp').index(env) + 10000 * K + 7 * rows + 3 * M + n))
    f = lambda x: np.ascontiguousarray(x, np.float32)
    if env == 'pt':
        od, ad = 6 + K, 2
        wp, wq, wq2 = mlp_weights_flat(rng, od, 4), mlp_weights_flat(rng, od + 2, 1), mlp_weights_flat(rng, od + 2, 1)

        def draw_obs():
            o = reset_law_obs(rng, rows)
            return f(np.concatenate([o, o[:, 3:4] + 0.3 * rng.standard_normal((rows, K))], 1)) if K else o
        obs, obs2 = draw_obs(), draw_obs()
    elif env == 'pd':
        od, ad = 4, 1
        wp, wq, wq2 = mlp_weights_flat(rng, 4, 2), mlp_weights_flat(rng, 5, 1), mlp_weights_flat(rng, 5, 1)
        obs, obs2 = pendulum_wide_obs(rng, rows), pendulum_wide_obs(rng, rows)
    else:
        od, ad = 11, 1
        inp, _ = DP.load_case(GOLDEN, 256, 25)
        wp, wq, wq2 = f(inp['w_policy']), f(inp['w_Q1']), mlp_weights_flat(rng, 12, 1)
        obs, obs2 = DP.start_obs(rng, rows), DP.start_obs(rng, rows)
    d = dict(od=od, ad=ad, wp=wp, wq=wq, wq2=wq2, obs=obs, obs2=obs2, act=f(rng.uniform(-1, 1, (rows, ad))),
             rew=f(rng.uniform(-30, 0, rows)), y=f(0.3 * rng.standard_normal(rows) - 0.5), rewards=f(rng.uniform(-30, 0, (n, rows))),
             eps=f(rng.standard_normal((n, rows * M))), eps_a=f(rng.standard_normal((rows, ad))), eps_b=f(rng.standard_normal((rows, ad))))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def make_cfg(env, K=0, squash=False):
    if env == 'pt':
        return ops.make_cfg(obs_dim=6 + K, policy_out_activation='linear', action_range=1.5) if squash else ops.make_cfg(obs_dim=6 + K)
    return ops.make_cfg(PD) if env == 'pd' else ops.make_cfg(DP.ENV_ID)      # (the pendulum's default: linear output, range 3)


def dev(x):
    return torch.as_tensor(np.array(x, np.float32)).to(DEV)


def with_status(cfg):
    """a status word of the call's own (MPG_STATUS_* bits), compared like every other output"""
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    cfg.status = st.data_ptr()
    return st


def outputs(*tensors):
    return tuple(t.clone() for t in tensors)


# ---- the table --------------------------------------------------------------------------------------------------------------------
# name; fn(ops, engine) -> tuple of output tensors (clones); rows; the workspace query of the call with its configuration (cfg: a
# function, sizes: the query's arguments behind cfg for a row count); step: the distance to the next row count the entry point accepts;
# used: whether the call writes to its workspace at all.  ONE entry-point call per case: a second call in the same guarded block would get
# the first one's view back and run over its finite leftovers
Case = collections.namedtuple('Case', 'name fn rows query cfg sizes step used')
CASES = []


def _add(name, rows, fn, query, cfg, sizes, step=1, used=True):
    CASES.append(Case('%s-rows%d' % (name, rows), fn, rows, query, cfg, sizes, step, used))


def _tag(env, K):
    return env + ('-K%d' % K if env == 'pt' else '')


def _targets_cases():
    for env, K in (('pt', 0), ('pt', 3)):
        for rows in (1, 17, 1037):
            cfg_of, q, sz = functools.partial(make_cfg, env, K), 'mpg_q_targets_workspace_bytes', lambda r: (r,)

            def plain(ops, engine, env=env, K=K, rows=rows, critics=2, smooth=False):
                d, cfg = inputs(env, K, rows), make_cfg(env, K)
                st = with_status(cfg)
                return outputs(ops.q_targets(cfg, dev(d['wp']), dev(d['wq']), dev(d['wq2']) if critics == 2 else None, dev(d['rew']), dev(d['obs2']),
                                             smooth_eps=dev(d['eps_a']) if smooth else None), st)

            def td3(ops, engine, env=env, K=K, rows=rows, smooth=True):
                d, cfg = inputs(env, K, rows), make_cfg(env, K)
                st = with_status(cfg)
                return outputs(*ops.td3_targets(cfg, *[dev(d[k]) for k in ('wp', 'wq', 'wq2', 'rew', 'obs2')], dev(d['eps_a']) if smooth else None), st)

            def nstep(ops, engine, env=env, K=K, rows=rows, clip=None):
                d, cfg = inputs(env, K, rows), make_cfg(env, K)
                st = with_status(cfg)
                return outputs(ops.nstep_targets(cfg, dev(d['wp']), dev(d['wq']), dev(d['rewards']), dev(d['obs2']), clip=clip), st)
            _add('q_targets-' + _tag(env, K), rows, plain, q, cfg_of, sz)
            _add('q_targets_one_critic-' + _tag(env, K), rows, functools.partial(plain, critics=1), q, cfg_of, sz)
            _add('q_targets_smooth-' + _tag(env, K), rows, functools.partial(plain, smooth=True), q, cfg_of, sz)
            _add('td3_targets-' + _tag(env, K), rows, td3, q, cfg_of, sz)
            _add('td3_targets_no_smoothing-' + _tag(env, K), rows, functools.partial(td3, smooth=False), q, cfg_of, sz)
            _add('nstep_targets-' + _tag(env, K), rows, nstep, q, cfg_of, sz)
            _add('nstep_targets_clipped-' + _tag(env, K), rows, functools.partial(nstep, clip=ops.PENDULUM_NSTEP_Q_CLIP), q, cfg_of, sz)
    for env, K in (('pt', 0), ('pt', 3), ('pd', 0), ('dp', 0)):
        for rows in (1, 17, 1037):
            def q_target(ops, engine, env=env, K=K, rows=rows):
                d, cfg = inputs(env, K, rows), make_cfg(env, K)
                st = with_status(cfg)
                return outputs(ops.rollout_q_target(cfg, dev(d['wp']), dev(d['wq']), dev(d['obs']), dev(d['act']), dev(d['eps'])), st)
            _add('rollout_q_target-' + _tag(env, K), rows, q_target, 'mpg_rollout_q_target_workspace_bytes', functools.partial(make_cfg, env, K),
                 lambda r: (r,))
        for rows, M in ((1, 1), (17, 1), (1037, 1), (1, 2), (17, 2)):
            def q_est(ops, engine, env=env, K=K, rows=rows, M=M):
                d, cfg = inputs(env, K, rows, M), make_cfg(env, K)
                st = with_status(cfg)
                return outputs(ops.rollout_q_estimation(cfg, dev(d['wp']), dev(d['wq']), dev(d['obs']), dev(d['act']), dev(d['eps']), [0, 2, 3],
                                                        M=M), st)
            _add('rollout_q_estimation-%s-M%d' % (_tag(env, K), M), rows, q_est, 'mpg_rollout_q_estimation_workspace_bytes',
                 functools.partial(make_cfg, env, K), lambda r, M=M: (r, M, 3))


def _critic_cases():
    for K in (0, 3, 10):
        for rows in (1, 17, 1037) + ((2051,) if K == 0 else ()):
            def fn(ops, engine, K=K, rows=rows):
                d, cfg = inputs('pt', K, rows), make_cfg('pt', K)
                st = with_status(cfg)
                return outputs(*ops.q_loss_grad(cfg, dev(d['wq']), dev(d['obs']), dev(d['act']), dev(d['y']), want_td=True), st)
            _add('q_loss_grad-' + _tag('pt', K), rows, fn, 'mpg_q_loss_grad_workspace_bytes', functools.partial(make_cfg, 'pt', K), lambda r: (r,))


LOG_ALPHA, TARGET_ENTROPY = float(np.log(0.2)), -2.0


def _head_call(ops, kind, form, env, K, rows):
    """one call of a SAC entry point: kind 'grad' / 'targets' / 'sample' / 'sample_logits', form 'plain' / 'squashed' / 'auto' / 'squashed_auto'"""
    squash = form.startswith('squashed')
    d, cfg = inputs(env, K, rows), make_cfg(env, K, squash)
    st = with_status(cfg)
    suffix = '' if form == 'plain' else '_' + form
    pol, q1, q2 = dev(d['wp']), dev(d['wq']), dev(d['wq2'])
    if kind in ('sample', 'sample_logits'):
        return outputs(*getattr(ops, 'policy_sample' + suffix)(cfg, pol, dev(d['obs']), dev(d['eps_a']), want_logits=kind == 'sample_logits'), st)
    temp = torch.full((1,), LOG_ALPHA, dtype=torch.float32, device=DEV) if form.endswith('auto') else 0.2
    if kind == 'targets':
        return outputs(getattr(ops, 'sac_targets' + suffix)(cfg, pol, q1, q2, dev(d['rew']), dev(d['obs2']), dev(d['eps_a']), temp), st)
    if form.endswith('auto'):
        return outputs(*getattr(ops, 'sac_policy_grad' + suffix)(cfg, pol, q1, q2, dev(d['obs']), dev(d['eps_a']), temp, dev(d['eps_b']),
                                                                 TARGET_ENTROPY), st)
    return outputs(*getattr(ops, 'sac_policy_grad' + suffix)(cfg, pol, q1, q2, dev(d['obs']), dev(d['eps_a']), temp), st)


def _policy_grad_cases():
    for K in (0, 3):
        for rows in (1, 17, 1037) + ((2051,) if K == 0 else ()):
            def td3(ops, engine, K=K, rows=rows):
                d, cfg = inputs('pt', K, rows), make_cfg('pt', K)
                st = with_status(cfg)
                return outputs(*ops.td3_policy_grad(cfg, dev(d['wp']), dev(d['wq']), dev(d['wq2']), dev(d['obs'])), st)

            def dpg(ops, engine, K=K, rows=rows):
                d, cfg = inputs('pt', K, rows), make_cfg('pt', K)
                st = with_status(cfg)
                return outputs(*ops.dpg_policy_grad(cfg, dev(d['wp']), dev(d['wq']), dev(d['obs'])), st)
            cfg_of = functools.partial(make_cfg, 'pt', K)
            _add('td3_policy_grad-' + _tag('pt', K), rows, td3, 'mpg_td3_policy_grad_workspace_bytes', cfg_of, lambda r: (r,))
            _add('dpg_policy_grad-' + _tag('pt', K), rows, dpg, 'mpg_dpg_policy_grad_workspace_bytes', cfg_of, lambda r: (r,))
    queries = {'grad': 'mpg_sac_policy_grad%s_workspace_bytes', 'targets': 'mpg_sac_targets%s_workspace_bytes',
               'sample': 'mpg_policy_sample%s_workspace_bytes', 'sample_logits': 'mpg_policy_sample%s_workspace_bytes'}
    names = {'grad': 'sac_policy_grad', 'targets': 'sac_targets', 'sample': 'policy_sample', 'sample_logits': 'policy_sample_want_logits'}
    for kind in ('grad', 'targets', 'sample', 'sample_logits'):
        for form in ('plain', 'squashed', 'auto', 'squashed_auto')[:2 if kind.startswith('sample') else 4]:
            squash = form.startswith('squashed')
            for env, K in (('pt', 0), ('pt', 3)) + ((('pd', 0),) if squash else ()):
                thin = kind == 'grad' and env == 'pd'           # (policy input 4 wide, two used outputs: backward_takes_thin)
                for rows in (1, 17, 1037) + ((2051,) if thin else ()):
                    fn = functools.partial(lambda ops, engine, a: _head_call(ops, *a), a=(kind, form, env, K, rows))
                    # (with logits_out the logits go straight to the caller's array - csrc/learner_api.hip policy_sample - and the one
                    # array of this workspace is left alone: guards only)
                    _add('%s%s-%s' % (names[kind], '' if form == 'plain' else '_' + form, _tag(env, K)), rows, fn,
                         queries[kind] % ('_squashed' if squash else ''), functools.partial(make_cfg, env, K, squash), lambda r: (r,),
                         used=kind != 'sample_logits')


SELECT, W3 = (0, 2, 3), (0.2, 0.35, 0.5)


def _bind_cache(ops, cfg, d):
    """the networks as views of one flat [Q1 | policy] vector with its packed images registered in cfg (tests/test_slices_gpu.py
    packed_run): what sends an all-steps launch at K = 0, M = 1 to the THIN reverse sweep.  Returns (policy, Q1, the cache to keep)."""
    flat = dev(np.concatenate([d['wq'], d['wp']]))
    wc = ops.WeightCache(flat, [(d['od'] + d['ad'], 1), (d['od'], 2 * d['ad'])])
    cfg.wcache[0] = wc.pointer
    return flat[d['wq'].size:], flat[:d['wq'].size], wc


def _sweep_cases():
    def pg(ops, engine, env, K, rows, M, n, all_steps, cache):
        d, cfg = inputs(env, K, rows, M, n), make_cfg(env, K)
        st = with_status(cfg)
        pol, q1, wc = _bind_cache(ops, cfg, d) if cache else (dev(d['wp']), dev(d['wq']), None)
        sel, w = (SELECT, W3) if n == 3 else ((0, 5, 25), W3)
        out = outputs(*ops.rollout_pg(cfg, pol, q1, dev(d['obs']), dev(d['eps']), list(sel), w, M=M, all_steps_param_grad=all_steps), st)
        torch.cuda.synchronize()        # (the cache's images outlive the launches that read them)
        del wc
        return out

    def ampc(ops, engine, env, K, rows, M, n, cache):
        d, cfg = inputs(env, K, rows, M, n), make_cfg(env, K)
        st = with_status(cfg)
        pol, _, wc = _bind_cache(ops, cfg, d) if cache else (dev(d['wp']), None, None)
        out = outputs(*ops.ampc_pg(cfg, pol, dev(d['obs']), dev(d['eps']), M=M), st)
        torch.cuda.synchronize()
        del wc
        return out

    # step-0 mode: any row count
    for env, K in (('pt', 0), ('pt', 3), ('pd', 0), ('dp', 0)):
        for rows, M in ((1, 1), (17, 1), (1037, 1), (1, 2), (17, 2)):
            _add('rollout_pg-step0-%s-M%d' % (_tag(env, K), M), rows, functools.partial(pg, env=env, K=K, rows=rows, M=M, n=3, all_steps=False, cache=False),
                 'mpg_rollout_pg_workspace_bytes', functools.partial(make_cfg, env, K), lambda r, M=M: (r, M, 3, 3, 0))
    _add('rollout_pg-step0-pt-K0-M1-n25', 17, functools.partial(pg, env='pt', K=0, rows=17, M=1, n=25, all_steps=False, cache=False),
         'mpg_rollout_pg_workspace_bytes', functools.partial(make_cfg, 'pt', 0), lambda r: (r, 1, 25, 3, 0))
    # all-steps mode and mpg_ampc_pg: rows * M % 16 == 0
    forms = [('pt', 0, 1, True, (16, 1040, 1056)),           # THIN reverse sweep, k_wgrad_w2 on the split engine
             ('pt', 0, 1, False, (16, 1056)), ('pt', 3, 1, False, (16, 1056)),      # plain / WIDE sweeps, the single-job weight gradient
             ('pt', 0, 2, True, (8, 528)), ('pt', 3, 2, False, (8, 528)),           # M = 2 (a bound cache changes nothing but the images read)
             ('pd', 0, 1, False, (16, 1056)), ('dp', 0, 1, False, (16, 1056))]
    for env, K, M, cache, rows_list in forms:
        tag = '%s-M%d%s' % (_tag(env, K), M, '-cached' if cache else '')
        for rows in rows_list:
            _add('rollout_pg-all-' + tag, rows, functools.partial(pg, env=env, K=K, rows=rows, M=M, n=3, all_steps=True, cache=cache),
                 'mpg_rollout_pg_workspace_bytes', functools.partial(make_cfg, env, K), lambda r, M=M: (r, M, 3, 3, 1))
            _add('ampc_pg-' + tag, rows, functools.partial(ampc, env=env, K=K, rows=rows, M=M, n=3, cache=cache),
                 'mpg_ampc_pg_workspace_bytes', functools.partial(make_cfg, env, K), lambda r, M=M: (r, M, 3), step=16 // M)
    _add('ampc_pg-pt-K0-M1-cached-n25', 32, functools.partial(ampc, env='pt', K=0, rows=32, M=1, n=25, cache=True),
         'mpg_ampc_pg_workspace_bytes', functools.partial(make_cfg, 'pt', 0), lambda r: (r, 1, 25), step=16)


def _fused_cases():
    def mg(ops, engine, K, rows, M, n_q, select):
        d, cfg = inputs('pt', K, rows, M), make_cfg('pt', K)
        st = with_status(cfg)
        nets = [d['wq']] + ([d['wq2']] if n_q == 2 else []) + [d['wp']]
        params = dev(np.concatenate(nets))
        targets = dev(np.concatenate([(x * np.float32(0.97)).astype(np.float32) for x in nets]))
        grad, stats, y_out = (torch.zeros(k, dtype=torch.float32, device=DEV) for k in (params.numel(), 16, rows))
        ops.mpg_gradients(cfg, n_q, params, targets, dev(d['obs']), dev(d['act']), dev(d['rew']), dev(d['obs2']), None, list(select),
                          W3[:len(select)], grad, stats, y_out, M=M, eps=dev(d['eps']))
        return outputs(grad, stats, y_out, st)
    # fused path (rows % 16 == 0, M = 1, K = 0): two slices - the kernels built for [0, n] - and three; then the composed fallback with its
    # two sub-workspaces: rows = 17, M = 2, and a wide observation
    table = [(0, r, 1, (0, 3)) for r in (16, 272, 1056)] + [(0, 16, 1, SELECT), (0, 272, 1, SELECT)] + \
            [(0, 17, 1, (0, 3)), (0, 17, 1, SELECT), (0, 17, 2, (0, 3)), (0, 16, 2, SELECT), (3, 272, 1, (0, 3))]
    for K, rows, M, select in table:
        for n_q in (1, 2):
            path = 'fused' if (rows % 16 == 0 and M == 1 and K == 0) else 'fallback'
            _add('mpg_gradients-%s-%s-M%d-nq%d-sel%s' % (path, _tag('pt', K), M, n_q, '_'.join(str(k) for k in select)), rows,
                 functools.partial(mg, K=K, rows=rows, M=M, n_q=n_q, select=select), 'mpg_mpg_gradients_workspace_bytes',
                 functools.partial(make_cfg, 'pt', K), lambda r, M=M, ns=len(select), n_q=n_q: (r, M, 3, ns, n_q))


_targets_cases()
_critic_cases()
_policy_grad_cases()
_sweep_cases()
_fused_cases()
assert len({c.name for c in CASES}) == len(CASES)
