"""What the GPU tests of the one-launch worker samples share (tests/test_worker*_rollout*_gpu.py): the engine fixture, the policy
network with its cfg and status word, one side's sentinel-filled buffers, the whole-ring comparison of a launch with its chain, the
mask of written ring slots, the repeat loop, and the callers' pairs - OffPolicyWorker.sample with and without one_launch_sample, the
native step driver with the launch and kept on the chain (sample_iters < 0).  Floats are compared as their 32-bit patterns (a NaN row
has to match too).  A test file keeps its run_chain / run_launch with the ctypes calls written out, its policy tweaks, its start
states and every assertion particular to its entry point."""
import numpy as np
import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops

DEV = 'cuda'
RING = ('ring_obs', 'ring_act', 'ring_rew', 'ring_obs2', 'ring_done')
NAMES = ('state', 'obs_io', 'act_out', 'done_out') + RING + ('status',)


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


@pytest.fixture(params=['split', 'f32'])
def engine(request):
    """both builds of the library (mpg_amd/_lib.py ENGINES): the split-fp16 product and the exact-fp32 engine"""
    with L.engine(request.param):
        yield request.param


def ring_ptrs(t):
    return [L.ptr(t[k]) for k in RING]


def assert_same(a, b, what, names=NAMES):
    for k in names:
        assert torch.equal(bits(a[k]), bits(b[k])), (what, k)


class PolicyNet(object):
    """a policy network of mlp_weights_flat(PCG64(rng_seed), in_dim, n_out) - after tweak(flat), in place, if given - and the caller's
    cfg pointed at its status word, with or without the packed weight image"""

    def __init__(self, in_dim, n_out, cfg, packed, rng_seed, tweak=None):
        from tests.golden_inputs import mlp_weights_flat
        flat = mlp_weights_flat(np.random.Generator(np.random.PCG64(rng_seed)), in_dim, n_out)
        if tweak is not None:
            tweak(flat)
        self.od, self.cfg = in_dim, cfg
        self.pol = torch.as_tensor(flat).to(DEV)
        self.wc = None
        if packed:                                        # the packed-image instantiation: cfg.wcache[0] -> the policy's images
            self.wc = ops.WeightCache(self.pol, [(in_dim, n_out)])
            self.cfg.wcache[0] = self.wc.pointer
        self.status = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.cfg.status = self.status.data_ptr()


def start(env, od, ad, n, cap, init_obs=None, nan_row=None):
    """one side's buffers: the agents of `env` (n of them, just constructed) from its reset law or from init_obs, rings full of a
    sentinel"""
    obs = (env.reset() if init_obs is None else env.reset(init_obs=torch.as_tensor(init_obs).to(DEV))).clone()
    if nan_row is not None:                               # the agent and its observation: NaN from the start
        env._state[:, nan_row] = float('nan')
        obs[nan_row] = float('nan')
    f = dict(dtype=torch.float32, device=DEV)
    return dict(state=env._state, obs_io=obs, act_out=torch.full((n, ad), -7., **f), done_out=torch.full((n,), 0xAB, dtype=torch.uint8, device=DEV),
                ring_obs=torch.full((cap, od), -7., **f), ring_act=torch.full((cap, ad), -7., **f), ring_rew=torch.full((cap,), -7., **f),
                ring_obs2=torch.full((cap, od), -7., **f), ring_done=torch.full((cap,), 0xAB, dtype=torch.uint8, device=DEV))


def both(runs, make_start, n, iters, cap=None, nxt=5, ctr=7, ectr=3):
    """run(t, n, iters, cap, nxt, ctr, ectr) for every run of `runs`, each on a fresh t = make_start(n, cap); one synchronise; -> the
    dicts in the order of `runs`"""
    cap = iters * n + 13 if cap is None else cap
    out = [make_start(n, cap) for _ in runs]
    for run, t in zip(runs, out):
        run(t, n, iters, cap, nxt, ctr, ectr)
    torch.cuda.synchronize()
    return out


def touched(cap, nxt, count, device=DEV):
    """the ring slots that `count` transitions from slot nxt on are written to"""
    mask = torch.zeros(cap, dtype=torch.bool, device=device)
    mask[(nxt + torch.arange(count, device=device)) % cap] = True
    return mask


def assert_repeatable(make_start, run_launch, times):
    """`times` times run_launch(t) on a fresh t = make_start(): every result equals the first, all ten names"""
    first = None
    for _ in range(times):
        t = make_start()
        run_launch(t)
        if first is None:
            first = t
        else:
            assert_same(first, t, 'repeat')


# ---- OffPolicyWorker.sample ---------------------------------------------------------------------------------------------------
def worker_sample_pair(make_args, extra_counters=False):
    """OffPolicyWorker on make_args(**more) without and with one_launch_sample, two consecutive samples each (the second continues
    from what the first left): the counters, the five arrays of either batch, the worker's and the env's observations, the env state
    and the done flags are equal.  -> the two (worker, batches, counters); extra_counters: a stochastic policy's status check and
    its sample counter."""
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    out = []
    for one in (False, True):
        args = make_args(**(dict(one_launch_sample=True) if one else {}))
        w = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
        batches = [w.sample(), w.sample()]
        torch.cuda.synchronize()
        counters = (w._noise_ctr, w.env._ctr, w.num_sample, w.sample_times)
        if extra_counters:
            w.policy_with_value.check_status()
            counters += (w.policy_with_value._sample_ctr,)
        out.append((w, batches, counters))
    (wa, ba, ca), (wb, bb, cb) = out
    assert ca == cb, (ca, cb)
    for x, y in zip(ba, bb):
        assert len(x) == len(y) == 5
        for u, v in zip(x, y):
            assert u.shape == v.shape and u.dtype == v.dtype and torch.equal(bits(u), bits(v))
    assert torch.equal(bits(wa.obs), bits(wb.obs)) and torch.equal(bits(wa.env.obs), bits(wb.env.obs))
    assert torch.equal(bits(wa.env._state), bits(wb.env._state)) and torch.equal(wa.env.done, wb.env.done)
    return out


# ---- native step driver ---------------------------------------------------------------------------------------------------------
def _on_the_chain(opt, sample_iters, chain):
    assert opt._fused.c.sample_iters == sample_iters > 0
    if chain:
        opt._fused.c.sample_iters = -sample_iters         # include/mpg_hip.h: the same iterations on the entry points the launch replaces
    return opt


def per_trees(opt):
    """driver_state's extra of a prioritized replay"""
    rb = opt.replay_buffer
    return [rb._it_sum, rb._it_min, rb._stamp, rb._max_priority], ()


def driver_state(opt, extra=None):
    """-> (clones of the tensors a native driver's run leaves, its counters); extra(opt) -> (more tensors, more counters)"""
    pw, rb, c, f = opt.worker.policy_with_value, opt.replay_buffer, opt._fused.c, opt._fused
    tensors = [pw.params, pw.targets, pw.m, pw.v, rb.obs, rb.act, rb.rew, rb.obs2, rb.done, f.t['w_obs'], f.t['w_act'], f.t['w_done'],
               opt.worker.env._state, opt.learner.flat, pw.status]
    counters = (c.noise_ctr, c.env_ctr, c.ring_next, c.ring_size, c.replay_times, c.learner_counter, [c.opt_steps[i] for i in range(3)])
    if extra is not None:
        more = extra(opt)
        tensors, counters = tensors + list(more[0]), counters + tuple(more[1])
    return [x.clone() for x in tensors], counters


def driver_chain_pair(make_opt, sample_iters, steps=25, extra=None):
    """`steps` steps of make_opt()'s native driver with the launch, and of another kept on the chain: counters equal, every tensor
    equal bit for bit.  -> the two driver_state()s"""
    out = []
    for chain in (False, True):
        opt = _on_the_chain(make_opt(), sample_iters, chain)
        for _ in range(steps):
            opt.step()
        torch.cuda.synchronize()
        out.append(driver_state(opt, extra))
    (a, ca), (b, cb) = out
    assert ca == cb, (ca, cb)
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(bits(x), bits(y)), k
    return out


def worker_launch_counts(make_opt, sample_iters, max_samples):
    """-> [with the launch, on the chain]: what the driver's own timer counts in slot 2, the worker's launches, over the first step
    (iteration 0 samples)"""
    counts = []
    for chain in (False, True):
        opt = _on_the_chain(make_opt(), sample_iters, chain)
        prof = ops.Profiler(max_samples=max_samples)
        opt.set_profiler(prof)
        prof.start(1)
        opt.step()
        torch.cuda.synchronize()
        counts.append(prof.read(2)[1])
        opt.set_profiler(None)
        prof.close()
    return counts
