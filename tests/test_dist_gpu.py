"""Data-parallel form of the gradient step ON THE HIP KERNELS: two processes share the one GPU of the
test box and exchange through `gloo` (RCCL refuses two ranks on one device; the exchange step is the same single
all-reduce of the flat [gradients | statistics] buffer).  Parity statement: the N-rank gradient on a B-row minibatch
equals the reference learner's gradient on the same B rows."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import mpg_oracle as O

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _init(rank, world, port):
    """MPG_DIST_BACKEND (inherited from the test that spawned this process): 'gloo' or 'oneshot' (the IPC one-shot exchange)"""
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                      HSA_ENABLE_IPC_MODE_LEGACY='0')
    from mpg_amd import dist as D
    # MPG_TEST_RANK_PER_DEVICE=1 (tools/first_8gpu.sh, on a multi-GPU node): rank r on device r - the same tests with real peers
    # (IPC mappings and events across devices, copies over xGMI); default: every rank time-shares device 0 (the 1-GPU box)
    per_dev = os.environ.get('MPG_TEST_RANK_PER_DEVICE') == '1' and torch.cuda.device_count() > 1
    torch.cuda.set_device(rank % torch.cuda.device_count() if per_dev else 0)
    D.init_from_env(backend=os.environ.get('MPG_DIST_BACKEND', 'gloo'))
    return D


def _golden_worker(rank, world, port, q):
    D = _init(rank, world, port)
    from mpg_amd.config import default_args
    from mpg_amd.learners import MPGLearner
    from mpg_amd.policy import PolicyWithQs
    g = np.load(os.path.join(GOLDEN, 'mpg_v2_H256_B64.npz'))
    B = g['batch_obs'].shape[0]
    lo, hi = rank * B // world, (rank + 1) * B // world
    args = default_args('MPG-v2', replay_batch_size=hi - lo, num_batch_reuse=1)
    learner = MPGLearner(PolicyWithQs, args)
    pw = learner.policy_with_value
    flat = np.concatenate([g['w_' + n] for n in pw.names])
    pw.set_flat(flat, (flat * np.float32(g['target_scale'])).astype(np.float32))

    def dev(x):
        return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).cuda()
    batch = [dev(g[k][lo:hi]) for k in ('batch_obs', 'batch_actions', 'batch_rewards', 'batch_obs_tp1', 'batch_dones')]
    grads = learner.compute_gradient(batch, None, None, 100, eps=dev(g['eps'][:, lo:hi]))
    got = torch.cat([x.reshape(-1) for x in grads]).cpu().numpy()
    st = learner.get_stats()
    D.barrier()
    q.put((rank, got, {k: st[k] for k in ('value_mean', 'q_loss1', 'q_loss2', 'policy_gradient_norm', 'q_gradient_norm1')}))
    torch.distributed.destroy_process_group()


def _run(fn, world=2):
    port = _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=fn, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    return sorted(out, key=lambda t: t[0])


@pytest.fixture(params=['gloo', 'oneshot', 'oneshot-host'])
def exchange(request, monkeypatch):
    """the exchanges of the gradient buffer that a 1-GPU box can run with several ranks: gloo's all-reduce, and the one-shot
    all-reduce over IPC-mapped staging slots (mpg_amd/dist.py OneShotAllReduce) in its two synchronisation forms - interprocess
    events (default) and the round-3 host barrier - spawned workers inherit the variables"""
    monkeypatch.setenv('MPG_DIST_BACKEND', request.param.split('-')[0])
    monkeypatch.setenv('MPG_ONESHOT_SYNC', 'host' if request.param.endswith('-host') else 'event')
    return request.param


@pytest.mark.timeout(300)
def test_two_rank_gradient_equals_reference_gradient_on_the_full_batch(exchange):
    out = _run(_golden_worker)
    g = np.load(os.path.join(GOLDEN, 'mpg_v2_H256_B64.npz'))
    ref = g['it100_grads']
    assert np.array_equal(out[0][1], out[1][1])                    # every rank holds the same clipped gradient
    got, o = out[0][1], 0
    for din, dout in ((8, 1), (8, 1), (6, 4)):
        for shp in O.mlp_shapes(din, 256, dout):
            n = int(np.prod(shp))
            if np.linalg.norm(ref[o:o + n]) > 0:
                err = np.linalg.norm(got[o:o + n].astype(np.float64) - ref[o:o + n]) / np.linalg.norm(ref[o:o + n])
                assert err <= 1e-4, (din, shp, err)
            o += n
    for k, v in out[0][2].items():
        np.testing.assert_allclose(v, g['it100_' + k], rtol=1e-4, atol=1e-6, err_msg=k)


def _driver_worker(rank, world, port, q):
    D = _init(rank, world, port)
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import MPGLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    # MPG_TEST_REPLAY_ROWS (default 64): a batch that is not a multiple of 16 takes mpg_mpg_gradients' launch-per-stage path
    args = default_args('MPG-v2', num_agent=64, batch_size=64, replay_batch_size=int(os.environ.get('MPG_TEST_REPLAY_ROWS', '64')),
                        replay_starts=128, max_buffer_size=4096, seed=rank, init_seed=0)
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    worker.policy_with_value.sync_from_rank0()
    opt = SingleProcessOffPolicyOptimizer(worker, MPGLearner(PolicyWithQs, args), ReplayBuffer(args, 0), None, args,
                                          sampling_interval=1)
    assert opt._fused is not None and opt._fused.c.world_size == world
    for _ in range(int(os.environ.get('MPG_TEST_STEPS', '20'))):
        opt.step()
    pw = worker.policy_with_value
    torch.cuda.synchronize()
    D.barrier()
    q.put((rank, torch.cat([pw.params, pw.targets, pw.m, pw.v]).cpu().numpy(), worker.obs.cpu().numpy()))
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(300)
def test_native_step_driver_keeps_two_replicas_bit_identical(exchange):
    """Different env / replay / noise streams per rank, ONE all-reduce per step, replicated clip + Adam + Polyak:
    parameters, targets and Adam moments stay bit-identical across ranks without any weight broadcast."""
    out = _run(_driver_worker)
    assert np.array_equal(out[0][1], out[1][1]) and np.isfinite(out[0][1]).all()
    assert not np.array_equal(out[0][2], out[1][2])               # the ranks really saw different data


@pytest.mark.timeout(600)
def test_two_rank_training_loop_follows_the_data_parallel_oracle_loop(monkeypatch):
    """Config 5's semantics in closed loop, two ranks on the one GPU: each rank runs its own worker / replay / model-noise
    streams (seed = rank) through the native step driver, the flat gradient is exchanged (gloo) between mpg_step_begin and
    mpg_step_end, clip + Adam + Polyak run on every replica.  Against tests/c2_loop.data_parallel_step: the oracle's loop with two
    replicas' Philox inputs, the gradient of the CONCATENATED minibatch (every loss is a mean over the global batch), one shared set of
    parameters.  20 iterations from the same initial weights: parameter update within 1e-3 relative L2 (measured: printed)."""
    import torch as T
    from mpg_amd.policy import init_mlp_flat
    from tests.c2_loop import OracleConfig2Loop, data_parallel_step
    monkeypatch.setenv('MPG_DIST_BACKEND', 'gloo')
    out = _run(_driver_worker)                               # 20 native steps per rank, replicas bit-identical
    assert np.array_equal(out[0][1], out[1][1])
    gen = T.Generator().manual_seed(0)                       # PolicyWithQs' initialisation for init_seed = 0 (mpg_amd/policy.py)
    dims = {'Q1': (8, 1), 'Q2': (8, 1), 'policy': (6, 4)}
    w = {n: init_mlp_flat(gen, *dims[n]).numpy() for n in ('Q1', 'Q2', 'policy')}
    init = np.concatenate([w[n] for n in ('Q1', 'Q2', 'policy')])
    nthreads = T.get_num_threads()
    T.set_num_threads(8)
    loops = [OracleConfig2Loop(w, seed=r, num_agent=64, batch_size=64, replay_batch_size=64, replay_starts=128, capacity=4096) for r in range(2)]
    for _ in range(20):
        data_parallel_step(loops)
    T.set_num_threads(nthreads)
    ref, reft = loops[0].flat()
    n = ref.size
    got, gott = out[0][1][:n], out[0][1][n:2 * n]
    rel = lambda a, b: float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b.astype(np.float64)))
    e_u, e_p, e_t = rel(got - init, ref - init), rel(got, ref), rel(gott, reft)
    print('two-rank loop vs data-parallel oracle loop, 20 iterations: update %.1e, parameters %.1e, targets %.1e' % (e_u, e_p, e_t))
    assert e_u <= 1e-3 and e_p <= 1e-5 and e_t <= 1e-5, (e_u, e_p, e_t)


@pytest.mark.timeout(900)
def test_native_step_driver_keeps_four_replicas_bit_identical(monkeypatch):
    """The same with FOUR ranks time-sharing the one GPU (nothing had run with more than two ranks, so rank-count
    dependent state - slot indexing, the two staging parities, the per-peer events - was untested beyond 2).  Round 5: both IPC forms -
    one-shot and TWO-SHOT (reduce-scatter + all-gather) - and, because both take the rank-order sum, 10 native steps must leave the
    SAME bits in both.  (gloo with four ranks was dropped in round 5 to keep the suite's run time: nothing in that path depends on
    the rank count beyond what the two-rank test and the 8-rank bench dry run exercise.)"""
    monkeypatch.setenv('MPG_DIST_BACKEND', 'oneshot')
    monkeypatch.setenv('MPG_ONESHOT_SYNC', 'event')
    monkeypatch.setenv('MPG_TEST_STEPS', '10')          # (four processes time-slicing one GPU: ~3 s per step; both parities re-used 5 times)
    runs = []
    for mode in ('oneshot', 'twoshot'):
        monkeypatch.setenv('MPG_ONESHOT_MODE', mode)
        out = _run(_driver_worker, world=4)
        for r in range(1, 4):
            assert np.array_equal(out[0][1], out[r][1]), (mode, r)
            assert not np.array_equal(out[0][2], out[r][2])
        assert np.isfinite(out[0][1]).all()
        runs.append(out[0][1])
    assert np.array_equal(runs[0], runs[1])


@pytest.mark.timeout(900)
@pytest.mark.parametrize('backend', ['gloo', 'oneshot', 'gloo-rows60'])
def test_critics_exchange_under_the_reverse_sweep_leaves_the_same_bits(backend, monkeypatch):
    """SURVEY f4 "overlap with the Q-grad kernel" (off by default, MPG_OVERLAP_EXCHANGE=1): the library finishes the critics' gradient
    ahead of the reverse sweep and records the caller's event there (mpg_grad_opts_t.critics_ready_event); the driver exchanges
    the critics' slice on a second stream under the sweep and the policy's slice + statistics behind it.  Two exchanges instead of
    one, the same sums in the same order: 20 native steps on two ranks must leave the same bits as the single exchange.
    [gloo-rows60: a replay batch of 60 rows - not a multiple of 16 - takes the launch-per-stage path of mpg_mpg_gradients,
    which did not record critics_ready_event before round 6: the side stream then waited on a STALE record and exchanged the critics'
    slice while mpg_q_loss_grad was still writing it.]"""
    if backend.endswith('-rows60'):
        backend = backend.split('-')[0]
        monkeypatch.setenv('MPG_TEST_REPLAY_ROWS', '60')
    monkeypatch.setenv('MPG_DIST_BACKEND', backend)
    monkeypatch.setenv('MPG_ONESHOT_SYNC', 'event')
    runs = []
    for ov in ('0', '1'):
        monkeypatch.setenv('MPG_OVERLAP_EXCHANGE', ov)
        out = _run(_driver_worker)
        assert np.array_equal(out[0][1], out[1][1]) and np.isfinite(out[0][1]).all()
        runs.append(out[0][1])
    assert np.array_equal(runs[0], runs[1])


def _oneshot_sum_worker(rank, world, port, q):
    D = _init(rank, world, port)
    n = 205318 + 16                                      # the MPG-v2 gradient buffer
    g = torch.Generator(device='cpu').manual_seed(100 + rank)
    mine = (torch.randn(n, generator=g) * torch.logspace(-6, 2, n)).float()
    flat = mine.cuda()
    outs = []
    n_ex = int(os.environ.get('MPG_TEST_EXCHANGES', '6'))
    in_slot = os.environ.get('MPG_TEST_IN_SLOT') == '1'
    for k in range(n_ex):                                 # both staging parities, each re-used (6: twice; 90: across two event generations)
        buf = flat * float(k % 7 + 1)
        if in_slot:                                       # the contribution written straight into the staging slot; buf: only the destination
            D.grad_slot(n, flat.device).copy_(buf)
            buf.fill_(float('nan'))
            D.all_reduce_sum_(buf, in_slot=True)
        else:
            D.all_reduce_sum_(buf)
        if k < 6 or k >= n_ex - 2:
            outs.append((k, buf.cpu().numpy()))
    torch.cuda.synchronize()
    D.barrier()
    q.put((rank, mine.numpy(), outs))
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize('world,sync,mode,n_ex', [(2, 'event', 'oneshot', 6), (2, 'host', 'oneshot', 6), (8, 'event', 'oneshot', 6),
                                                  (2, 'event', 'twoshot', 90), (2, 'host', 'twoshot', 6), (8, 'event', 'twoshot', 6),
                                                  (3, 'event', 'twoshot', 6), (2, 'event-slot', 'oneshot', 6),
                                                  (3, 'event-slot', 'twoshot', 6), (2, 'event-S', 'oneshot', 6), (2, 'event-S', 'twoshot', 6)])
def test_oneshot_all_reduce_is_the_in_rank_order_sum_bit_for_bit(monkeypatch, world, sync, mode, n_ex):
    """OneShotAllReduce on its own: exchanges of a 205 334-float buffer with entries over eight orders of magnitude (both
    staging parities re-used: the slot-reuse waits of the event form are exercised; 90 exchanges cross two event generations).
    Every rank must hold exactly fl(..fl(x_0 + x_1) + .. + x_{world-1}) - the rank-order float32 sum - each time; 2 ranks in
    both synchronisation forms and 8 ranks (all time-sharing the one GPU of the test box) in the event form.
    Round 5: the same for the TWO-SHOT form (reduce-scatter + all-gather) with 2, 3 (slices of unequal length) and 8
    ranks (4 ranks: the native-driver test above) - its slice sums take the same rank order, so the result must be the same bits.
    `-slot`: every rank writes its buffer into D.grad_slot() and exchanges with in_slot=True (3 ranks, two-shot: unequal slices, the
    own slice not copied); `-S`: the separate "reads done" events (MPG_ONESHOT_S_EVENTS=1)."""
    sync, _, variant = sync.partition('-')
    monkeypatch.setenv('MPG_DIST_BACKEND', 'oneshot')
    monkeypatch.setenv('MPG_ONESHOT_SYNC', sync)
    monkeypatch.setenv('MPG_TEST_IN_SLOT', '1' if variant == 'slot' else '0')
    monkeypatch.setenv('MPG_ONESHOT_S_EVENTS', '1' if variant == 'S' else '0')
    monkeypatch.setenv('MPG_ONESHOT_MODE', mode)
    monkeypatch.setenv('MPG_TEST_EXCHANGES', str(n_ex))
    out = _run(_oneshot_sum_worker, world=world)
    xs = [out[r][1] for r in range(world)]
    assert len(out[0][2]) == min(n_ex, 8)
    for k, _ in out[0][2]:
        ref = xs[0] * np.float32(k % 7 + 1)
        for r in range(1, world):
            ref = ref + xs[r] * np.float32(k % 7 + 1)                       # float32 arithmetic, rank order
        for r in range(world):
            got = dict(out[r][2])[k]
            assert np.array_equal(got, ref), (k, r)


def _misuse_worker(rank, world, port, q):
    D = _init(rank, world, port)
    n = 4096 + 16
    dev = torch.device('cuda', torch.cuda.current_device())
    g = torch.Generator(device='cpu').manual_seed(7)
    x, y = torch.randn(n, generator=g).cuda(), torch.randn(n, generator=g).cuda()
    r = {}

    def refusal(fn):
        try:
            fn()
        except RuntimeError as e:
            return str(e)
        return None

    def plain(v):                                         # a correct plain exchange: with one rank the sum is v itself
        buf = v.clone()
        D.all_reduce_sum_(buf, force=True)
        return torch.equal(buf, v)
    out = torch.full((n,), float('nan'), device=dev)
    # 1. an in-slot exchange with no slot taken for it
    r['no_slot'] = refusal(lambda: D.all_reduce_sum_(out, force=True, in_slot=True))
    r['no_slot_then'] = plain(y)
    # 2. a plain exchange while a slot is outstanding (it would overwrite the slot)
    slot = D.grad_slot(n, dev, force=True)
    slot.copy_(x)
    r['same_slot'] = D.grad_slot(n, dev, force=True).data_ptr() == slot.data_ptr()
    buf = y.clone()
    r['outstanding'] = refusal(lambda: D.all_reduce_sum_(buf, force=True))
    D.all_reduce_sum_(out, force=True, in_slot=True)
    r['outstanding_then'] = torch.equal(out, x)
    # 3. an exchange from another stream than the exchanger's first
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        r['stream'] = refusal(lambda: D.all_reduce_sum_(buf, force=True))
    r['streams'] = ('%#x' % side.cuda_stream, '%#x' % torch.cuda.current_stream().cuda_stream)
    r['stream_then'] = plain(y)
    # a slot handed back: plain exchanges go on
    D.grad_slot(n, dev, force=True)
    D.release_slot(n)
    r['released_then'] = plain(x)
    torch.cuda.synchronize()
    q.put((rank, r))
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(300)
def test_oneshot_exchange_refuses_a_stale_slot_or_another_stream(monkeypatch):
    """The staging slot of grad_slot() belongs to the next exchange, and the reuse of the slots is ordered by ONE stream: an in-slot
    exchange without a slot, a plain exchange while a slot is outstanding (it would overwrite the slot) and an exchange from another
    stream are refused before anything is enqueued, and a correct exchange after each still returns the right sum (one rank)."""
    monkeypatch.setenv('MPG_DIST_BACKEND', 'oneshot')
    monkeypatch.setenv('MPG_ONESHOT_SYNC', 'event')
    r = _run(_misuse_worker, world=1)[0][1]
    assert r['no_slot'] is not None and r['no_slot_then']
    assert r['same_slot'] and r['outstanding'] is not None and r['outstanding_then']
    assert r['stream'] is not None and all(s in r['stream'] for s in r['streams']), (r['stream'], r['streams'])
    assert r['stream_then'] and r['released_then']


def _step_error_worker(rank, world, port, q):
    D = _init(rank, world, port)
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import MPGLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker
    args = default_args('MPG-v2', num_agent=64, batch_size=64, replay_batch_size=64, replay_starts=128, max_buffer_size=4096,
                        seed=0, init_seed=0)
    worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
    opt = SingleProcessOffPolicyOptimizer(worker, MPGLearner(PolicyWithQs, args), ReplayBuffer(args, 0), None, args,
                                          sampling_interval=1, always_exchange=True)
    learner, c = opt.learner, opt._fused.c
    for _ in range(3):
        opt.step()
    real = D.all_reduce_sum_

    def fail_once(*a, **k):
        D.all_reduce_sum_ = real
        raise RuntimeError('injected exchange failure')
    D.all_reduce_sum_ = fail_once
    try:
        opt.step()
        raised = False
    except RuntimeError:
        raised = True
    state = (raised, c.grad == learner.flat.data_ptr(), c.clip_partials_ready)
    D.all_reduce_sum_(learner.flat, force=True)           # refused if the failed step had left its slot outstanding
    opt.step()
    torch.cuda.synchronize()
    q.put((rank, state, bool(torch.isfinite(worker.policy_with_value.params).all().item())))
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(300)
def test_failed_exchange_leaves_the_step_context_on_the_flat_gradient(monkeypatch):
    """The native step with the one-shot slot exchange: if the exchange raises, the context points back at the flat gradient with no
    claim of ready clip partials, the slot is handed back (a plain exchange goes through), and the next step succeeds (one rank)."""
    monkeypatch.setenv('MPG_DIST_BACKEND', 'oneshot')
    monkeypatch.setenv('MPG_ONESHOT_SYNC', 'event')
    _, (raised, grad_is_flat, partials_ready), finite = _run(_step_error_worker, world=1)[0]
    assert raised and grad_is_flat and partials_ready == 0 and finite


def _rccl_worker(rank, world, port, q):
    """One rank, backend 'nccl' (= RCCL): the collective really runs between mpg_step_begin and mpg_step_end, on the
    stream the library launches on, and mpg_step_end takes the exchanged-gradient branch (mpg_sq_partials)."""
    os.environ.update(RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                      HSA_ENABLE_IPC_MODE_LEGACY='0')
    from mpg_amd import dist as D
    D.init_from_env(backend='nccl')
    assert torch.distributed.is_initialized() and torch.distributed.get_backend() == 'nccl'
    from mpg_amd.buffer import ReplayBuffer
    from mpg_amd.config import default_args
    from mpg_amd.learners import MPGLearner
    from mpg_amd.optimizer import SingleProcessOffPolicyOptimizer
    from mpg_amd.policy import PolicyWithQs
    from mpg_amd.worker import OffPolicyWorker

    def run(always_exchange):
        args = default_args('MPG-v2', num_agent=256, batch_size=256, replay_batch_size=256, replay_starts=512,
                            max_buffer_size=4096, seed=0, init_seed=0)
        worker = OffPolicyWorker(PolicyWithQs, args.env_id, args, 0)
        opt = SingleProcessOffPolicyOptimizer(worker, MPGLearner(PolicyWithQs, args), ReplayBuffer(args, 0), None, args,
                                              sampling_interval=1, always_exchange=always_exchange)
        assert opt._fused is not None and opt._fused.c.grads_exchanged == int(always_exchange)
        for _ in range(30):
            opt.step()
        torch.cuda.synchronize()
        pw = worker.policy_with_value
        return torch.cat([pw.params, pw.targets, pw.m, pw.v]).cpu().numpy(), opt.learner.norms.cpu().numpy()
    a, na = run(True)          # RCCL all-reduce (identity in a one-rank group) + clip partials from the reduced buffer
    b, nb = run(False)         # no collective, clip partials as a by-product of the gradient launch
    # a second stream user: the collective must also be ordered against the library when it is NOT torch's default stream
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c, nc = run(True)
    q.put((0, a, b, c, na, nb, nc))
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(600)
def test_rccl_all_reduce_between_step_begin_and_step_end():
    """backend='nccl' IS RCCL on ROCm.  A one-rank group on the one GPU of the test box: 30 native steps with the flat
    [gradients | statistics] buffer all-reduced by RCCL between mpg_step_begin and mpg_step_end end in bit-identical
    parameters / targets / Adam moments to 30 steps without the collective - i.e. RCCL loads, the collective is ordered
    correctly against the library's launches on the current stream (default and non-default), and the
    exchanged-gradient branch of the clip (mpg_sq_partials after the reduce) yields the same norms as the fused one."""
    port = _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_worker, args=(0, 1, port, q))
    p.start()
    _, a, b, c, na, nb, nc = q.get(timeout=500)
    p.join(60)
    assert p.exitcode == 0
    assert np.isfinite(a).all() and np.array_equal(a, b) and np.array_equal(a, c)
    assert np.array_equal(na, nb) and np.array_equal(na, nc)


@pytest.mark.timeout(900)
@pytest.mark.parametrize('backend,nproc', [('gloo', 2), ('oneshot', 2), ('gloo', 8), ('oneshot', 8)])
def test_bench_in_the_drivers_multi_rank_form(backend, nproc):
    """`bench.py` exactly as the driver launches it for N > 1 - `python -m torch.distributed.run --nnodes=1 --nproc-per-node 2
    --master-addr 127.0.0.1 --master-port P bench.py --gpus 2 --steps K --warmup W` - as a dry run on the one GPU of the test
    box (MPG_DIST_BACKEND=gloo / oneshot: both ranks on device 0; RCCL itself refuses two ranks on one device).  Checks the
    launch form, the rendezvous, the barrier-bracketed timed region, the max over ranks and the one JSON line of rank 0:
    n_gpus N, weak scaling, whole-job value = N x 4096 env-steps per step / time.  N = 8 (all eight ranks time-sharing the
    one GPU) is the driver's SCALE form: rank-count dependent state beyond 2 and the `exchange_ms` key."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # (a shorter burn-in than the bench's default 200 steps: N ranks time-share one GPU here, and this is a test of the launch form)
    env = dict(os.environ, MPG_DIST_BACKEND=backend, HSA_ENABLE_IPC_MODE_LEGACY='0', MPG_BENCH_BURN_IN='60')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(nproc), '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.join(root, 'bench.py'), '--gpus', str(nproc), '--steps', '10', '--warmup', '3',
           '--full', '--no-cpu-baseline']
    out = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=850)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]                 # rank 0 prints ONE line
    d = json.loads(lines[0])
    assert d['n_gpus'] == nproc and d['steps'] == 10 and d['warmup'] == 3 and d['scaling'] == 'weak' and d['higher_is_better'] is True
    assert d['config']['parallelism'] == 'dp%d' % nproc and d['config']['global_batch'] == nproc * 4096
    assert d['config']['dist_backend'].startswith(backend)
    np.testing.assert_allclose(d['value'], nproc * 4096 / (d['ms_per_step'] * 1e-3), rtol=1e-6)
    assert 'roofline' in d and d['vs_baseline'] is None
    assert d['exchange_ms'] is not None and d['exchange_ms'] > 0 and d['exchange_launches'] > 0
    # --full: five profiled regions of `steps` steps after the timed one, and the exchange alone in every form this group can run
    # (both IPC forms here)
    assert d['timed_regions'] == 5 and len(d['region_ms_per_step']) == 5 and all(r > 0 for r in d['region_ms_per_step'])
    forms = d['exchange_forms_ms']
    assert set(forms) >= {'oneshot', 'twoshot'} and all(isinstance(forms[k], float) and forms[k] > 0 for k in ('oneshot', 'twoshot')), forms


@pytest.mark.parametrize('n_slots', [1, 2, 8])
def test_sum_slots_sq_equals_sum_slots_then_sq_partials(n_slots):
    """mpg_sum_slots_sq (round 6: the exchange's rank-order sum with the clip's partial sums of squares of the RESULT as a by-product) ==
    mpg_sum_slots followed by mpg_sq_partials, bit for bit - sums, partials, and the statistics tail behind the networks - for the
    MPG-v2 layout (two critics + policy + 16 statistics), a strided slot array, and n_slots = 1 (the two-shot form's copy out of its
    gather array)."""
    import ctypes
    import mpg_amd._lib as L
    from mpg_amd import ops
    sizes = [ops.net_size(8, 1), ops.net_size(8, 1), ops.net_size(6, 4)]
    n = sum(sizes) + 16
    stride = n + 48
    g = torch.Generator().manual_seed(n_slots)
    slots = (torch.randn(n_slots, stride, generator=g) * 10.0 ** torch.randint(-4, 1, (n_slots, stride), generator=g).float()).cuda()
    csz = (ctypes.c_int * 3)(*sizes)
    out_a, out_b = torch.empty(n).cuda(), torch.full((n,), float('nan')).cuda()
    part_a, part_b = torch.zeros(3 * 272).cuda(), torch.full((3 * 272,), float('nan')).cuda()
    L.call('mpg_sum_slots_strided', L.ptr(slots), L.c_int(n_slots), L.c_size_t(stride), L.c_int(n), L.ptr(out_a), L.stream())
    L.call('mpg_sq_partials', L.ptr(out_a), csz, L.c_int(3), L.ptr(part_a), L.stream())
    L.call('mpg_sum_slots_sq', L.ptr(slots), L.c_int(n_slots), L.c_size_t(stride), L.c_int(n), L.ptr(out_b), csz, L.c_int(3), L.ptr(part_b),
           L.stream())
    torch.cuda.synchronize()
    assert torch.equal(out_a, out_b) and torch.equal(part_a, part_b)
    ref = slots[0, :n].clone()
    for r in range(1, n_slots):
        ref += slots[r, :n]
    assert torch.equal(out_b, ref)
