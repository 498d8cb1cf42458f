"""The native AMPC step (learner_version 8 of mpg_step_begin / mpg_step_end, taken with SingleProcessOffPolicyOptimizer(native_ampc=True))
on the GPU, both engines, against the method-by-method path bit for bit: parameters, Adam moments, the untouched target copy, the five
ring arrays, the worker's observations, the clip's norms, every counter and every statistic both paths report - over the sweeps' forms
(THIN, WIDE, ragged M, the horizon's ends), with exploration noise, on the pendulum's one-agent sample, with stock methods in between,
across a checkpoint, with the worker's chain instead of the one-launch sample, after a refused step, on a NaN batch and in mirrored
worlds of 2 and 4."""
import pytest
import torch

from mpg_amd import _lib as L

pytestmark = pytest.mark.gpu
PD = 'InvertedPendulumConti-v0'


def bits(t):
    t = t.contiguous()
    return t if t.dtype in (torch.uint8, torch.int32) else t.view(torch.int32)


@pytest.fixture(params=['split', 'f32'])
def engine(request):
    """both builds of the library (mpg_amd/_lib.py ENGINES): the split-fp16 product and the exact-fp32 engine"""
    with L.engine(request.param):
        yield request.param


def _stack(native, seed=0, interval=10, always_exchange=False, **kw):
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import AMPCLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    args = default_args('AMPC', seed=seed, nan_check_interval=10 ** 9, **kw)
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    learner = AMPCLearner(PolicyWithQs, args)
    more = dict(native_ampc=True) if native else {}           # the method path is built WITHOUT the keyword
    opt = SingleProcessOffPolicyOptimizer(worker, learner, ReplayBuffer(args, 0), None, args, sampling_interval=interval,
                                          always_exchange=always_exchange, **more)
    assert (opt._fused is not None) == native
    return opt


NAMES = ('params', 'adam m', 'adam v', 'targets', 'ring obs', 'ring act', 'ring rew', 'ring obs2', 'ring done', 'worker obs', 'norms')


def _state(opt):
    pw, rb, w, ln = opt.worker.policy_with_value, opt.replay_buffer, opt.worker, opt.learner
    torch.cuda.synchronize()
    tensors = [t.clone() for t in (pw.params, pw.m, pw.v, pw.targets, rb.obs, rb.act, rb.rew, rb.obs2, rb.done, w.obs, ln.norms)]
    counters = (dict(pw.opt_steps), rb._next_idx, len(rb), rb.replay_times, w._noise_ctr, w.env._ctr, ln.counter, opt.num_sampled_steps)
    return tensors, counters


def _equal_states(a, b):
    (ta, ca), (tb, cb) = a, b
    assert ca == cb, (ca, cb)
    for nm, x, y in zip(NAMES, ta, tb):
        assert x.shape == y.shape and torch.equal(bits(x), bits(y)), (nm, (bits(x) != bits(y)).sum().item())


def _equal_stats(sa, sb):
    both = sorted(set(sa) & set(sb))
    assert {'policy_loss', 'policy_gradient_norm'} <= set(both), (sorted(sa), sorted(sb))
    for k in both:
        assert sa[k] == sb[k], (k, sa[k], sb[k])


# ---- 1: 25 iterations from one seed ----------------------------------------------------------------------------------------------
DEFAULTS = dict(num_agent=8, batch_size=512, replay_batch_size=256, replay_starts=1024, max_buffer_size=4096)     # 64 worker steps per sample
CASES = {
    'thin-K0': dict(DEFAULTS),                                                                 # n = 25, M = 1: the THIN reverse sweep
    'wide-K3': dict(DEFAULTS, num_future_data=3),                                              # look-ahead entries: the WIDE sweeps
    'ragged-M2': dict(DEFAULTS, replay_batch_size=24, M=2, num_rollout_list_for_policy_update=[10]),      # 48 rollout rows
    'n31': dict(DEFAULTS, replay_batch_size=48, num_rollout_list_for_policy_update=[31]),      # the horizon's ends, three row groups
    'n1': dict(DEFAULTS, replay_batch_size=48, num_rollout_list_for_policy_update=[1]),
    'explore': dict(DEFAULTS, explore_sigma=0.1),
    'linear': dict(DEFAULTS, policy_out_activation='linear'),                                  # ('tanh' is the parser's default: thin-K0)
    'pendulum': dict(env_id=PD, replay_batch_size=256, replay_starts=512, max_buffer_size=4096),          # one agent, 512 iterations per sample
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_native_step_equals_method_by_method_path(engine, case):
    """learner_version 8 enqueues what the python classes enqueue"""
    kw = CASES[case]

    def run(native):
        opt = _stack(native, **kw)
        pw = opt.worker.policy_with_value
        if case == 'pendulum':
            assert (opt.worker.num_agent, opt.worker.batch_size) == (1, 512)
        elif case in ('thin-K0', 'explore'):
            assert pw.cfg.policy_out_act == 1                                                  # tanh
        targets0 = pw.targets.clone()
        for _ in range(25):
            opt.step()
        pw.check_status()
        assert torch.equal(bits(pw.targets), bits(targets0)), 'the step wrote the target copy'
        return _state(opt), opt.learner.get_stats()
    a, sa = run(True)
    b, sb = run(False)
    _equal_states(a, b)
    iters = 512 if case == 'pendulum' else 64
    warm = (512 if case == 'pendulum' else 1024) // (iters * (1 if case == 'pendulum' else 8))
    assert a[1][0] == {'policy': 25} and a[1][4] == (warm + 3) * iters                         # warm-up and three sampling calls
    assert torch.isfinite(a[0][0]).all() and a[0][10].item() > 0
    _equal_stats(sa, sb)


# ---- 2: stock methods between native steps -----------------------------------------------------------------------------------------
def test_stock_methods_interleaved_with_native_steps(engine):
    """worker.sample_with_count() + rb.add_batch() between native steps, on a 700-slot ring that wraps, end in the same state as the
    method path doing the same calls"""
    def run(native):
        opt = _stack(native, interval=2, num_agent=64, batch_size=64, replay_batch_size=96, replay_starts=256, max_buffer_size=700)
        for it in range(12):
            opt.step()
            if it % 3 == 1:
                batch, n = opt.worker.sample_with_count()
                opt.replay_buffer.add_batch(batch)
        assert len(opt.replay_buffer) == 700                  # (4 + 6 + 4 samples of 64: the ring wrapped)
        return _state(opt), opt.learner.get_stats()
    (a, sa), (b, sb) = run(True), run(False)
    _equal_states(a, b)
    _equal_stats(sa, sb)


# ---- 3: checkpoint -------------------------------------------------------------------------------------------------------------------
def test_checkpoint_resume_is_bit_identical(tmp_path, engine):
    """written by a native stack at iteration 8, loaded into a native stack built with another seed: after 12 more iterations the
    result is bit-identical to the uninterrupted run"""
    from mpg_amd.checkpoint import load_checkpoint, save_checkpoint

    def build(seed):
        return _stack(True, seed=seed, interval=3, num_agent=64, batch_size=64, replay_batch_size=64, replay_starts=256, max_buffer_size=1024,
                      num_rollout_list_for_policy_update=[10])
    a = build(5)
    for _ in range(8):
        a.step()
    path = save_checkpoint(str(tmp_path / 'ckpt.npz'), a)
    for _ in range(12):
        a.step()
    b = build(99)                        # different seed: every stream must come from the file
    meta = load_checkpoint(path, b)
    assert meta['optimizer']['iteration'] == 8 and b.iteration == 8 and meta['learner_cls'] == 'AMPCLearner'
    for _ in range(12):
        b.step()
    _equal_states(_state(a), _state(b))
    _equal_stats(a.learner.get_stats(), b.learner.get_stats())
    assert _state(a)[1][0] == {'policy': 20}


# ---- 4: the A/B switch -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('env', ['path-tracking-8x64', 'pendulum-1x64'])
def test_the_chain_of_worker_launches_equals_the_one_launch_sample(engine, env):
    """sample_iters < 0 (include/mpg_hip.h) keeps the chain of worker launches: the same stack, bit for bit"""
    kw = dict(num_agent=8, batch_size=512) if env.startswith('path') else dict(env_id=PD, num_agent=1, batch_size=64)

    def run(chain):
        opt = _stack(True, interval=3, replay_batch_size=64, replay_starts=128, max_buffer_size=2048, **kw)
        c = opt._fused.c
        assert c.sample_iters == 64 and c.num_agent * c.sample_iters <= c.ring_capacity
        if chain:
            c.sample_iters = -c.sample_iters
        for _ in range(7):                                   # samples at iterations 0, 3 and 6
            opt.step()
        opt.worker.policy_with_value.check_status()
        return _state(opt), opt.learner.get_stats()
    (a, sa), (b, sb) = run(False), run(True)
    _equal_states(a, b)
    _equal_stats(sa, sb)
    per = 64 * kw['num_agent']
    assert a[1][7] == (-(-128 // per) + 3) * per               # the warm-up's samples and three sampling calls


# ---- 5: a refused step ---------------------------------------------------------------------------------------------------------------
def test_a_refused_step_changes_nothing(engine):
    opt = _stack(True, interval=2, num_agent=64, batch_size=64, replay_batch_size=64, replay_starts=128, max_buffer_size=1024)
    opt.step()
    opt.step()
    before = _state(opt)
    assert opt.iteration == 2                                # an iteration that samples: the refusal comes before the sample
    opt._fused.c.n = 32
    with pytest.raises(L.MpgError, match='mpg_step_begin: .*0 < n < 32'):
        opt.step()
    assert opt.iteration == 2
    _equal_states(before, _state(opt))
    opt._fused.c.n = 25                                      # and the stack goes on as if nothing had been asked
    opt.step()
    ref = _stack(True, interval=2, num_agent=64, batch_size=64, replay_batch_size=64, replay_starts=128, max_buffer_size=1024)
    for _ in range(3):
        ref.step()
    _equal_states(_state(ref), _state(opt))


# ---- 6: NaN ----------------------------------------------------------------------------------------------------------------------------
def test_a_nan_batch_ends_alike_on_both_paths(engine):
    """every ring observation NaN before iteration 3 (which does not sample): the same status word, the same nonfinite flag, the same
    parameter bits, and check_status() raises alike"""
    def run(native):
        opt = _stack(native, num_agent=64, batch_size=64, replay_batch_size=64, replay_starts=128, max_buffer_size=1024)
        pw = opt.worker.policy_with_value
        for _ in range(3):
            opt.step()
        opt.replay_buffer.obs.fill_(float('nan'))
        opt.step()
        torch.cuda.synchronize()
        status, nonfinite, params = pw.status.clone(), pw.nonfinite.clone(), pw.params.clone()
        try:
            pw.check_status()
            raised = None
        except L.MpgError as e:
            raised = str(e)
        return status, nonfinite, params, raised, _state(opt)
    a, b = run(True), run(False)
    print('status %#x / %#x, nonfinite %s / %s, check_status: %r / %r' % (a[0].item(), b[0].item(), a[1].tolist(), b[1].tolist(), a[3], b[3]))
    assert a[0].item() == b[0].item(), (a[0].item(), b[0].item())
    assert torch.equal(a[1], b[1])
    assert torch.equal(bits(a[2]), bits(b[2]))
    assert a[3] == b[3], (a[3], b[3])
    _equal_states(a[4], b[4])
    # the step saw the NaN batch (or the test shows nothing): the clip's guard raised its flag and kept the gradient out of Adam
    assert a[1].item() != 0 and torch.isfinite(a[2]).all()


# ---- 7: mirrored worlds ----------------------------------------------------------------------------------------------------------------
def _world_stack(kind, fused, always_exchange):
    """tests/test_sharding_gpu.py::build_stack for the one kind it does not know; its sizes, sampling every third iteration"""
    assert kind == 'AMPC'
    return _stack(fused, interval=3, always_exchange=always_exchange, num_agent=64, batch_size=128, replay_batch_size=96, replay_starts=512,
                  max_buffer_size=1000)


def test_native_step_in_a_mirrored_world(monkeypatch, engine):
    """worlds of 2 and 4 whose ranks hold the same streams are bit-identical to one process with always_exchange, get_stats() included;
    one exchange per step (run_world asserts it); no nonzero pre-exchange entry of the one-process run is below TINY (asserted by
    check_mirrored_worlds, which is the condition of its exactness argument)"""
    from tests import test_sharding_gpu as SH
    monkeypatch.setattr(SH, 'build_stack', _world_stack)
    SH.check_mirrored_worlds(monkeypatch, 'AMPC', True)


# ---- 8: the default stays ---------------------------------------------------------------------------------------------------------------
def test_the_default_stays_the_method_path(engine):
    sizes = dict(num_agent=64, batch_size=64, replay_batch_size=64, replay_starts=64, max_buffer_size=256)
    opt = _stack(False, **sizes)
    assert opt._fused is None
    opt = _stack(True, **sizes)
    assert opt._fused is not None and opt._fused.c.learner_version == 8
    opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(opt.worker.policy_with_value.params).all()
