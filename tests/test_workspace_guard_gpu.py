"""Every learner entry point in exactly the bytes its `*_workspace_bytes` query reports, between two 1 MiB guard regions, over a workspace
that held NaN words (0xFF bytes) or zeros before the call, from a 256-byte aligned and from a 4-byte aligned pointer
(tests/workspace_guard.py: the helper, the table of cases and the row counts with the ragged form each reaches); the native step driver
with its two workspaces overwritten before every iteration; caller-owned output buffers of exactly the documented length between
sentinels.

This file tests INVARIANCE: every comparison is bit for bit against the stock call (ops.workspace untouched: a grown, reused buffer with
spare bytes behind it) and there is no tolerance anywhere.  Correctness against the oracle is the business of the other GPU tests."""
import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops
from tests import workspace_guard as G

pytestmark = pytest.mark.gpu
DEV = G.DEV


@pytest.fixture(params=['split', 'f32'])
def engine(request):
    """both builds of the library (mpg_amd/_lib.py ENGINES), as tests/test_slices_gpu.py's fixture"""
    with L.engine(request.param):
        yield request.param


def bits(t):
    t = t.contiguous()
    return t if t.dtype in (torch.uint8, torch.int32) else t.view(torch.int32)


def assert_same_bits(got, ref, where):
    """every tensor of `got` equals its partner in `ref` word for word (a NaN compares like any other word); the message names `where`,
    the output by position and the first differing index"""
    assert len(got) == len(ref), where + (len(got), len(ref))
    for pos, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape and a.dtype == b.dtype, where + ('output %d' % pos, a.shape, b.shape)
        x, y = bits(a).reshape(-1), bits(b).reshape(-1)
        if not torch.equal(x, y):
            bad = torch.nonzero(x != y).reshape(-1)
            i = int(bad[0].item())
            raise AssertionError(where + ('output %d' % pos, 'first differing index %d of %d (%d differ)' % (i, x.numel(), bad.numel()),
                                          'got %r, stock call %r' % (a.reshape(-1)[i].item(), b.reshape(-1)[i].item())))


RUNS = [('0xFF', G.NAN_FILL, 0), ('0x00', G.ZERO_FILL, 0), ('0xFF at a 4-byte aligned pointer', G.NAN_FILL, 4)]


@pytest.mark.parametrize('case', G.CASES, ids=[c.name for c in G.CASES])
def test_exact_workspace_any_contents(monkeypatch, engine, case):
    """the stock call, then the same call over a guarded workspace of exactly the queried size that held 0xFF, 0x00, and 0xFF again behind
    a pointer 4 bytes off a 256-byte line (the Arena aligns upwards and charges for it): guards intact, workspace used, every output
    the stock call's bits; the stock call's outputs hold no NaN"""
    ref = case.fn(ops, engine)
    torch.cuda.synchronize()
    for pos, t in enumerate(ref):
        assert not (t.is_floating_point() and bool(t.isnan().any())), (case.name, engine, 'stock call', 'output %d holds a NaN' % pos)
    for run, fill, misalign in RUNS:
        with G.guarded(monkeypatch, fill, misalign=misalign) as rec:
            got = case.fn(ops, engine)
        if misalign == 0 and fill == G.NAN_FILL:        # a figure, not a bar: how much of the workspace the call never wrote (pytest -s)
            for slot, words, left in G.unwritten_words(rec):
                print('   %s %s slot %d: %d of %d workspace words never written (%.1f %%)' % (engine, case.name, slot, left, words, 100.0 * left / words))
        G.check(rec, (case.name, engine, run), used=case.used)
        assert_same_bits(got, ref, (case.name, engine, run))


@pytest.mark.parametrize('entry', ['rollout_pg-all', 'ampc_pg'])
@pytest.mark.parametrize('rows', [16, 1056])
def test_the_cached_all_steps_cases_reach_the_thin_sweep(engine, entry, rows):
    """tests/test_slices_gpu.py assert_thin_ran on the table's own cases: the packed image alone changes no bit, while the THIN reverse
    sweep accumulates the first layer's gradient (dW1, db1) inside the sweep instead of in the weight-gradient launch - another
    summation order, other last bits.  Bit-equal first-layer arrays would mean that the '-cached' cases ran the plain sweep.  (With
    thin partials the weight-gradient launch of the split engine is k_wgrad_w2 by launch_wgrad's own condition; no result tells
    that form from k_wgrad, so it is not asserted.)"""
    by_name = {c.name: c for c in G.CASES}
    cached = by_name['%s-pt-K0-M1-cached-rows%d' % (entry, rows)].fn(ops, engine)
    plain = by_name['%s-pt-K0-M1-rows%d' % (entry, rows)].fn(ops, engine)
    first = 6 * 256 + 256
    assert cached[2].numel() == ops.policy_size(G.make_cfg('pt', 0)) and cached[2].shape == plain[2].shape
    assert not torch.equal(cached[2][:first], plain[2][:first]), (entry, engine, rows, 'the cached case did not reach the THIN reverse sweep')


# ---- the native step driver ---------------------------------------------------------------------------------------------------------
def _mpg_v2():
    from tests.test_lagged_sample_gpu import build           # (tests/test_reference_loop_gpu.py builds its stacks inline)
    return build('mpg-v2', None, True)


def _sac():
    from tests.test_sac_native_gpu import _stack
    return _stack(True, interval=2, num_agent=64, batch_size=64, replay_batch_size=96, replay_starts=256, max_buffer_size=700, num_batch_reuse=3)


@pytest.mark.parametrize('stack', [_mpg_v2, _sac], ids=['mpg-v2', 'sac'])
def test_step_driver_ignores_what_its_workspaces_held(engine, stack):
    """ws0 / ws1 of the step driver are handed straight to the entry points above (csrc/train_step.cpp) and no state lives in them
    between iterations: two stacks from the same seeds, one of them with both workspaces set to 0xFF before each of three iterations,
    end with the same bits in parameters, targets, Adam moments, the gradient and the status word"""
    def run(overwrite):
        opt = stack()
        step, pw = opt._fused, opt.worker.policy_with_value
        assert step is not None and step.ws1.numel() > 256
        for _ in range(3):
            if overwrite:
                step.ws0.fill_(0xFF)
                step.ws1.fill_(0xFF)
            opt.step()
        torch.cuda.synchronize()
        return [t.clone() for t in (pw.params, pw.targets, pw.m, pw.v, opt.learner.flat, pw.status, pw.nonfinite)], dict(pw.opt_steps)
    (a, ca), (b, cb) = run(True), run(False)
    assert ca == cb and all(v > 0 for v in ca.values()), (ca, cb)
    assert not a[0].isnan().any() and not torch.equal(a[2], torch.zeros_like(a[2]))          # three real steps
    assert_same_bits(a, b, (engine, 'workspaces overwritten before every iteration'))


# ---- caller-owned outputs of exactly the documented length ----------------------------------------------------------------------------
SENTINEL, PAD = -7.0, 1024          # 4 KiB of the sentinel on either side


class Between(object):
    """views of exactly the asked lengths, each between two 4 KiB regions of the sentinel in one larger tensor of its own"""

    def __init__(self):
        self.held = []

    def view(self, n):
        big = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.float32, device=DEV)
        self.held.append((big, n))
        return big[PAD:PAD + n]

    def check(self, where):
        flags = torch.stack([torch.stack([(big[:PAD] == SENTINEL).all(), (big[PAD + n:] == SENTINEL).all()]) for big, n in self.held]).cpu().numpy()
        for k, (front, behind) in enumerate(flags):
            assert front, where + ('buffer %d of length %d' % (k, self.held[k][1]), 'written in front of the view')
            assert behind, where + ('buffer %d of length %d' % (k, self.held[k][1]), 'written behind the view')


def _output_calls(rows):
    """(name, call(out) -> outputs): out is None (the wrapper allocates) or a Between that supplies every caller-owned buffer"""
    d, d3 = G.inputs('pt', 0, rows), G.inputs('pt', 3, rows)
    r16 = (rows + 15) // 16 * 16            # the next row count mpg_ampc_pg accepts
    da = G.inputs('pt', 0, r16)
    v = lambda out, n: out.view(n) if out is not None else None
    t = G.dev

    def q_loss(dd):
        cfg = G.make_cfg('pt', dd['od'] - 6)
        return lambda out: ops.q_loss_grad(cfg, t(dd['wq']), t(dd['obs']), t(dd['act']), t(dd['y']), grad_out=v(out, ops.q_size(cfg)),
                                           loss_out=v(out, 1), want_td=True)

    def rollout(dd):
        cfg = G.make_cfg('pt', dd['od'] - 6)
        return lambda out: ops.rollout_pg(cfg, t(dd['wp']), t(dd['wq']), t(dd['obs']), t(dd['eps']), list(G.SELECT), G.W3,
                                          grad_out=v(out, ops.policy_size(cfg)), stats_out=v(out, 2 * len(G.SELECT)))

    def ampc(out):
        cfg = G.make_cfg('pt', 0)
        return ops.ampc_pg(cfg, t(da['wp']), t(da['obs']), t(da['eps']), grad_out=v(out, ops.policy_size(cfg)), stats_out=v(out, 2))

    def pgrad(name, dd, squash=False):
        cfg = G.make_cfg('pt', dd['od'] - 6, squash)
        pol, q1, q2, obs, eps, eps2 = (dd[k] for k in ('wp', 'wq', 'wq2', 'obs', 'eps_a', 'eps_b'))
        size = ops.policy_size(cfg)
        if name == 'td3_policy_grad':
            return lambda out: ops.td3_policy_grad(cfg, t(pol), t(q1), t(q2), t(obs), grad_out=v(out, size), stats_out=v(out, 2))
        if name == 'dpg_policy_grad':
            return lambda out: ops.dpg_policy_grad(cfg, t(pol), t(q1), t(obs), grad_out=v(out, size), stats_out=v(out, 2))
        fn = getattr(ops, name)
        if name.endswith('auto'):
            la = torch.full((1,), G.LOG_ALPHA, dtype=torch.float32, device=DEV)
            return lambda out: fn(cfg, t(pol), t(q1), t(q2), t(obs), t(eps), la, t(eps2), G.TARGET_ENTROPY, grad_out=v(out, size),
                                  stats_out=v(out, 3), alpha_grad_out=v(out, 1))
        return lambda out: fn(cfg, t(pol), t(q1), t(q2), t(obs), t(eps), 0.2, grad_out=v(out, size), stats_out=v(out, 3))
    return [('q_loss_grad K0', q_loss(d)), ('q_loss_grad K3', q_loss(d3)), ('rollout_pg K0', rollout(d)), ('rollout_pg K3', rollout(d3)),
            ('ampc_pg K0 rows %d' % r16, ampc), ('td3_policy_grad K0', pgrad('td3_policy_grad', d)), ('td3_policy_grad K3', pgrad('td3_policy_grad', d3)),
            ('dpg_policy_grad K0', pgrad('dpg_policy_grad', d)), ('sac_policy_grad K0', pgrad('sac_policy_grad', d)),
            ('sac_policy_grad_squashed K3', pgrad('sac_policy_grad_squashed', d3, True)), ('sac_policy_grad_auto K0', pgrad('sac_policy_grad_auto', d)),
            ('sac_policy_grad_squashed_auto K0', pgrad('sac_policy_grad_squashed_auto', d, True))]


@pytest.mark.parametrize('rows', [17, 1037])
def test_caller_owned_outputs_of_exactly_the_documented_length(engine, rows):
    """grad_out, stats_out, loss_out (and alpha_grad_out) as views of exactly q_size / policy_size / the statistics' count floats between
    two 4 KiB regions of -7.0: both regions intact, and the values the stock call's bits.  The gradient lengths are odd (68 353 for the
    policy at six inputs) while the summation kernels work in blocks of 64: the tail is where a write would stray."""
    assert ops.policy_size(G.make_cfg('pt', 0)) % 64 and ops.q_size(G.make_cfg('pt', 0)) % 64
    for name, call in _output_calls(rows):
        ref = [x.clone() for x in call(None) if x is not None]
        out = Between()
        got = [x.clone() for x in call(out) if x is not None]
        where = (name, engine, 'rows %d' % rows)
        assert out.held, where
        out.check(where)
        assert_same_bits(got, ref, where)
        assert not any(bool(x.isnan().any()) for x in ref), where
        assert not any(bool((x == SENTINEL).all()) for x in got), where + ('an output buffer still holds the sentinel everywhere',)
