"""The native SAC step with the learned temperature (mpg_sac_auto_step_begin / mpg_sac_auto_step_end, taken with
SingleProcessOffPolicyOptimizer(native_sac=True) and a SACLearner built with alpha = 'auto') against the method-by-method path:
parameters, targets, Adam moments, the temperature's state block, ring, worker observations, counters and statistics bit for bit -
also with stock methods in between and across a checkpoint; a fixed-alpha stack still calls mpg_sac_step_begin; the default stays the
method path.  Both engines."""
import pytest
import torch

from mpg_amd import _lib as L
from tests.test_sac_native_gpu import bits

pytestmark = pytest.mark.gpu


@pytest.fixture(params=['split', 'f32'])
def engine(request):
    with L.engine(request.param):
        yield request.param


def _stack(native, seed=0, interval=10, alpha='auto', **kw):
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import SACLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    more = dict(alpha='auto', target_entropy=-2., delay_update=2) if alpha == 'auto' else dict(alpha=alpha)
    args = default_args('SAC', seed=seed, **more, **kw)
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    learner = SACLearner(PolicyWithQs, args)
    more = dict(native_sac=True) if native else {}           # the method path is built WITHOUT the keyword
    opt = SingleProcessOffPolicyOptimizer(worker, learner, ReplayBuffer(args, 0), None, args, sampling_interval=interval, **more)
    assert (opt._fused is not None) == native
    return opt


def _state(opt):
    pw, rb, w, ln = opt.worker.policy_with_value, opt.replay_buffer, opt.worker, opt.learner
    torch.cuda.synchronize()
    tensors = [t.clone() for t in (pw.params, pw.targets, pw.m, pw.v, pw.alpha_state, rb.obs, rb.act, rb.rew, rb.obs2, rb.done, w.obs)]
    counters = (dict(pw.opt_steps), pw.alpha_opt_steps, rb._next_idx, len(rb), rb.replay_times, w._noise_ctr, w.env._ctr, ln.counter,
                pw._sample_ctr, opt.num_sampled_steps)
    return tensors, counters


def _equal_states(a, b):
    (ta, ca), (tb, cb) = a, b
    assert ca == cb, (ca, cb)
    for i, (x, y) in enumerate(zip(ta, tb)):
        assert torch.equal(bits(x), bits(y)), i


@pytest.mark.parametrize('K', [0, 3])
@pytest.mark.parametrize('reuse', [1, 3])
def test_native_auto_step_equals_method_by_method_path(engine, reuse, K):
    """25 iterations from the same seeds at the reference's worker defaults (8 agents, batch_size 512), B = 256, delay_update 2: the
    policy's and the temperature's Adam step on the 13 even iterations"""
    def run(native):
        opt = _stack(native, num_agent=8, batch_size=512, replay_batch_size=256, replay_starts=1024, max_buffer_size=4096,
                     num_batch_reuse=reuse, num_future_data=K)
        for _ in range(25):
            opt.step()
        opt.worker.policy_with_value.check_status()
        return _state(opt), opt.learner.get_stats()
    a, sa = run(True)
    b, sb = run(False)
    _equal_states(a, b)
    assert a[1][0] == {'Q1': 25, 'Q2': 25, 'policy': 13} and a[1][1] == 13
    assert a[0][4][0].item() != 0.0 and torch.isfinite(a[0][4]).all()                 # log_alpha moved away from its start
    both = sorted(set(sa) & set(sb))
    assert {'alpha', 'alpha_loss', 'alpha_gradient_norm', 'alpha_time', 'q_loss1', 'q_loss2', 'policy_loss', 'policy_entropy', 'value_mean',
            'value_var', 'q_gradient_norm1', 'q_gradient_norm2', 'policy_gradient_norm'} <= set(both)
    for k in both:
        assert sa[k] == sb[k], (k, sa[k], sb[k])
    assert sa['alpha_gradient_norm'] > 0 and sa['alpha_time'] is None


def test_stock_methods_interleaved_with_native_steps(engine):
    """worker.sample() + rb.add_batch() between native steps, on a 700-slot ring that wraps, end in the same state as the method path
    doing the same calls"""
    def run(native):
        opt = _stack(native, interval=2, num_agent=64, batch_size=64, replay_batch_size=96, replay_starts=256, max_buffer_size=700,
                     num_batch_reuse=3)
        for it in range(12):
            opt.step()
            if it % 3 == 1:
                batch, n = opt.worker.sample_with_count()
                opt.replay_buffer.add_batch(batch)
        return _state(opt)
    _equal_states(run(True), run(False))


def test_checkpoint_resume_is_bit_identical(tmp_path, engine):
    from mpg_amd.checkpoint import load_checkpoint, save_checkpoint

    def build(seed):
        return _stack(True, seed=seed, interval=3, num_agent=64, batch_size=64, replay_batch_size=128, replay_starts=256,
                      max_buffer_size=1024, num_batch_reuse=2)
    a = build(5)
    for _ in range(8):
        a.step()
    path = save_checkpoint(str(tmp_path / 'ckpt.npz'), a)
    for _ in range(12):
        a.step()
    b = build(99)                        # different seed: every stream, and the temperature's block and counter, come from the file
    meta = load_checkpoint(path, b)
    assert meta['optimizer']['iteration'] == 8 and b.iteration == 8 and meta['policy']['alpha_opt_steps'] == 4
    for _ in range(12):
        b.step()
    _equal_states(_state(a), _state(b))
    assert _state(a)[1][1] == 10


def test_which_entry_points_a_stack_calls(engine, monkeypatch):
    """'auto' takes the _auto pair; a fixed-alpha stack still calls mpg_sac_step_begin and mpg_step_end; the default stays the method
    path"""
    small = dict(num_agent=64, batch_size=64, replay_batch_size=64, replay_starts=64, max_buffer_size=256)
    assert _stack(False, **small)._fused is None and _stack(False, alpha=0.03, **small)._fused is None
    for alpha, want in (('auto', ['mpg_sac_auto_step_begin', 'mpg_sac_auto_step_end']), (0.03, ['mpg_sac_step_begin', 'mpg_step_end'])):
        opt = _stack(True, alpha=alpha, **small)
        assert opt._fused.c.learner_version == 7
        called = []

        class Spy(object):
            def __init__(self, lib):
                self._lib = lib

            def __getattr__(self, name):
                fn = getattr(self._lib, name)
                if 'step_' in name:
                    called.append(name)
                return fn
        monkeypatch.setattr(opt._fused, '_lib', Spy(opt._fused._lib))
        opt.step()
        torch.cuda.synchronize()
        assert called == want, (alpha, called)
        assert torch.isfinite(opt.worker.policy_with_value.params).all()
