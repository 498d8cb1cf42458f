"""Data-parallel glue: one process per GPU, torch.distributed (backend 'nccl' = RCCL over xGMI on ROCm;
'gloo' in CPU tests).  The hot path has exactly ONE exchange step per gradient step: an all-reduce(sum) of the
flat [gradients | statistics] buffer; everything else shards with no communication."""
import os

import torch
import torch.distributed as dist


_oneshot = {}            # OneShotAllReduce objects of this process by (buffer length, tag) (MPG_DIST_BACKEND=oneshot), built at the first exchange
_exchange = 'collective'  # 'collective': dist.all_reduce of the process group's backend; 'oneshot': the IPC one-shot form below


def init_from_env(backend=None):
    """Reads RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* (torchrun).  Returns (rank, world, local_rank).
    MPG_DIST_BACKEND (or `backend`): 'nccl' (= RCCL, the default on GPUs), 'gloo' (dry runs of a multi-rank launch on a box
    with fewer GPUs than ranks: RCCL refuses two ranks on one device), or 'oneshot' - the gradient exchange runs as the
    one-shot all-reduce over IPC-mapped staging slots (OneShotAllReduce); the process group itself (rendezvous, handle
    exchange, host barrier, the bench's max-over-ranks) is then a gloo group."""
    global _exchange
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if (world > 1 or backend is not None) and not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29500')
        if backend is None:
            backend = os.environ.get('MPG_DIST_BACKEND') or ('nccl' if torch.cuda.is_available() else 'gloo')
        if backend == 'oneshot':
            _exchange, backend = 'oneshot', 'gloo'
        if backend == 'nccl':
            torch.cuda.set_device(local)
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, world, local


def twoshot_slices(n, world):
    """[(lo, hi)] per rank: slice r of a buffer of n floats in the two-shot form - contiguous, disjoint, covering [0, n); every slice but
    the last starts and ends on a multiple of 64 floats (256-byte aligned copies); trailing ranks may get empty slices"""
    chunk = (((n + world - 1) // world) + 63) // 64 * 64
    return [(min(n, r * chunk), min(n, (r + 1) * chunk)) for r in range(world)]


class _HostShm(object):
    """A POSIX shared-memory file the ranks of one node use for HOST-to-host hand-shakes of the one-shot exchange:
      * `calls[r][phase]` - int64 counters per rank (a cache line each; phase 0: the exchange's writes, phase 1: the two-shot
        form's all-gather): publish(phase, v) / wait(p, phase, v) order "peer issued its event record" before "I issue my wait"
        (a wait captures the event's latest record at the time of the call - a fact about the peers' host threads, not about the
        GPU, so it is settled host to host without draining any stream);
      * `gen[r]`     - the newest event GENERATION whose handles rank r has published;
      * `handles[g & 1][r]` - the interprocess-event handles (NEV x 64 bytes) of rank r's generation g."""
    HB = 64                                        # sizeof(hipIpcEventHandle_t)
    NEV = 6                                        # events per generation: W0 W1 S0 S1 (one-shot) + G0 G1 (two-shot)

    TIMEOUT_S = 120.0                              # wall-clock bound on any hand-shake wait (a dead peer is reported, not spun on)

    def __init__(self, world, rank, tag):
        import numpy as np
        import uuid
        self.world, self.rank = world, rank
        n_i64 = 16 * world
        nbytes = 8 * n_i64 + 2 * world * self.NEV * self.HB
        # a name nobody else can hold: rank 0 picks it (pid + uuid) and creates the file exclusively, the others learn it through
        # the process group (two jobs on one node, or a stale file of another user, can no longer collide - ADVICE r4)
        name = ['/dev/shm/mpg_oneshot_%d_%s_%s' % (os.getpid(), uuid.uuid4().hex, tag) if rank == 0 else None]
        if rank == 0:
            fd = os.open(name[0], os.O_CREAT | os.O_EXCL | os.O_RDWR, 0o600)
            with os.fdopen(fd, 'wb') as fh:
                fh.write(b'\0' * nbytes)
        dist.broadcast_object_list(name, src=0)
        path = name[0]
        self.raw = np.memmap(path, dtype=np.uint8, mode='r+', shape=(nbytes,))
        self.a = self.raw[:8 * n_i64].view(np.int64)
        self.h = self.raw[8 * n_i64:].reshape(2, world, self.NEV, self.HB)
        dist.barrier()
        if rank == 0:
            os.unlink(path)              # the mappings keep it alive; nothing is left behind if a rank dies

    def publish(self, phase, v):
        self.a[16 * self.rank + phase] = v

    def _spin(self, i, v, what):
        """waits until counter i reaches v: a short pure spin (the common case - the peers' hosts run ahead of their GPUs - is
        settled within it), then yielding the core between polls (ranks that time-share a few cores must not starve the peer they
        wait for), bounded by the wall clock"""
        import time
        a = self.a
        for _ in range(2000):
            if a[i] >= v:
                return
        deadline = time.monotonic() + self.TIMEOUT_S
        while a[i] < v:
            os.sched_yield()
            if time.monotonic() > deadline:
                raise RuntimeError('one-shot all-reduce: %s %d not reached within %.0f s (a peer died or stalled)' % (what, v, self.TIMEOUT_S))

    def wait(self, p, phase, v):
        self._spin(16 * p + phase, v, 'rank %d, %s' % (p, ('exchange', 'all-gather of exchange')[phase]))

    def publish_handles(self, g, handles):
        import numpy as np
        for k, hb in enumerate(handles):
            self.h[g & 1, self.rank, k, :] = np.frombuffer(bytes(hb), dtype=np.uint8)
        self.a[16 * self.rank + 8] = g + 1           # (x86: stores are not reordered with older stores)

    def peer_handles(self, p, g):
        self._spin(16 * p + 8, g + 1, 'rank %d, event generation' % p)
        return [bytes(self.h[g & 1, p, k, :]) for k in range(self.NEV)]


class OneShotAllReduce(object):
    """One-shot all-reduce of a flat float32 buffer for the ranks of ONE node (the reference's exchange is
    the learner -> optimizer gradient hand-over, optimizer.py:60-94, payload mpg_learner.py:448-455).

    Every rank owns a staging array [2 parities][world slots][n] in device memory and maps every peer's through HIP IPC
    (torch's CUDA-IPC reductions: hipIpcGetMemHandle / hipIpcOpenMemHandle; HSA_ENABLE_IPC_MODE_LEGACY=0 on this pool).  An
    exchange is
        1. rank r copies its buffer into slot r of EVERY rank's staging array (world device-to-device copies; between GPUs
           these are direct xGMI writes - one hop, all 7 links busy at once, no ring);
        2. a FENCE: everybody's writes must have landed before anybody sums;
        3. every rank sums the `world` slots of its own array in rank order 0, 1, 2, ... (mpg_sum_slots): every replica computes
           the SAME association of the same numbers, so the replicas stay bit-identical by construction.
    Two staging parities alternate by call.  TWO-SHOT form (`mode='twoshot'`, MPG_ONESHOT_MODE=twoshot; the reduce-scatter +
    all-gather of SURVEY f4): 1. rank r writes slice p of its buffer into slot r of rank p's array (1/world of the bytes per link);
    2. fence; rank r sums the `world` copies of ITS slice in rank order (the same association: bit-identical results) into every
    rank's gather array [2 parities][n]; fence; 3. the gather array is the result.

    The fence (_fence) is the one place where the synchronisation forms differ.  `sync='event'` (default): rank r records
    W_r[parity] (G_r[parity] after the all-gather) on its stream and makes its stream wait (hipStreamWaitEvent) for every peer's
    INTERPROCESS event.  The host never waits for the GPU: a per-rank counter in shared memory (_HostShm) orders "peer issued its
    record" before "I issue my wait".  One rank has no peer and fences nothing.  `sync='host'` (MPG_ONESHOT_SYNC=host):
    stream.synchronize() + dist.barrier() - the control the tests compare against.

    Slot reuse needs no event of its own: a peer's slots (and gather array) of this parity were last read by its exchange it - 2,
    and this rank waited for the peer's W of exchange it - 1, which sits BEHIND the whole of exchange it - 2 in the peer's stream.
    That holds only if all exchanges of one exchanger are enqueued on ONE stream: the first exchange binds it, others are refused.
    (MPG_ONESHOT_S_EVENTS=1 also records and waits for a "reads done" event S per exchange: the control for a first multi-GPU run.)

    A HIP interprocess event can be recorded 32 times in its life (the 33rd hipStreamWaitEvent on an opened handle returns
    hipErrorInvalidValue whatever the owner does in between - archive/proto/ipc_event/probe.py), so the events live in
    GENERATIONS of GEN_LEN exchanges: the next generation's events are created and their handles published through the
    shared-memory file while the current one is in use, and opened by the peers at the generation boundary.

    Validated for correctness only - up to 8 processes time-sharing one GPU; no multi-GPU number is claimed."""
    GEN_LEN = 40          # exchanges per event generation: 20 records per event (+ 1 at creation), under the limit of 32

    def __init__(self, n, device, sync=None, mode=None):
        from torch.multiprocessing.reductions import reduce_tensor
        from . import _lib as L
        self.L = L
        self.world, self.rank = dist.get_world_size(), dist.get_rank()
        self.n = int(n)
        self.sync = sync or os.environ.get('MPG_ONESHOT_SYNC', 'event')
        self.s_events = os.environ.get('MPG_ONESHOT_S_EVENTS') == '1'
        assert self.sync in ('event', 'host')
        self.mode = mode or os.environ.get('MPG_ONESHOT_MODE', 'oneshot')
        assert self.mode in ('oneshot', 'twoshot')
        self.slices = twoshot_slices(self.n, self.world)
        self.dev = torch.device(device) if not isinstance(device, torch.device) else device
        # ONE IPC-mapped allocation per rank: [2 parities][world slots + 1][n] - the staging slots and, behind them, the gather
        # array of the two-shot form
        self.block = torch.zeros(2, self.world + 1, self.n, dtype=torch.float32, device=device)
        self.stage = self.block[:, :self.world]
        self.gath = self.block[:, self.world]
        torch.cuda.synchronize()
        handles = [None] * self.world
        dist.all_gather_object(handles, reduce_tensor(self.block))
        self.peer_blocks, failure = [], None
        for r in range(self.world):
            if r == self.rank:
                self.peer_blocks.append(self.block)
                continue
            try:
                f, a = handles[r]
                self.peer_blocks.append(f(*a))           # rebuild_cuda_tensor: opens the peer's allocation
            except Exception as e:          # noqa: BLE001 - reported below, on EVERY rank (a one-sided raise would leave the others in a barrier)
                failure = 'rank %d cannot open the IPC handle of rank %d\'s staging array (%r)' % (self.rank, r, e)
                break
        failures = [None] * self.world
        dist.all_gather_object(failures, failure)
        if any(failures):
            raise RuntimeError('one-shot all-reduce: ' + '; '.join(f for f in failures if f) + '. HSA_ENABLE_IPC_MODE_LEGACY=0 must be set '
                               'in every rank\'s environment (dmabuf IPC), every rank must see the peer GPUs (HIP_VISIBLE_DEVICES / '
                               'ROCR_VISIBLE_DEVICES not hiding them) and the GPUs must be peer-accessible; MPG_DIST_BACKEND=nccl selects '
                               'the RCCL all-reduce instead.')
        self.peers = [b[:, :self.world] for b in self.peer_blocks]
        self.peer_gath = [b[:, self.world] for b in self.peer_blocks]
        self.calls = 0
        self.slot_call = None            # the exchange (its `calls` value) the slot handed out by grad_slot() belongs to
        self.stream = None               # the stream of the first exchange: every later one must be issued on it
        if self.sync == 'event':
            global _oneshot_tag
            _oneshot_tag += 1
            self.shm = _HostShm(self.world, self.rank, '%d_%d' % (self.n, _oneshot_tag))
            self.mine, self.theirs = {}, {}        # generation -> [W0, W1, S0, S1, G0, G1] / {peer: [...]}
            self._make_generation(0)
            self._make_generation(1)
            self._open_generation(0)
        dist.barrier()

    # ---- event generations ----
    def _make_generation(self, g):
        ev = [torch.cuda.Event(enable_timing=False, interprocess=True) for _ in range(_HostShm.NEV)]
        for e in ev:
            e.record()                   # an interprocess event gets its handle once it has been recorded
        self.mine[g] = ev
        self.shm.publish_handles(g, [e.ipc_handle() for e in ev])

    def _open_generation(self, g):
        self.theirs[g] = {p: [torch.cuda.Event.from_ipc_handle(self.dev, h) for h in self.shm.peer_handles(p, g)]
                          for p in range(self.world) if p != self.rank}

    def grad_slot(self):
        """This rank's slot of its OWN staging array for the NEXT exchange: a producer that writes its buffer straight into it and
        then calls all_reduce_sum_(out, in_slot=True) saves the copy into the slot.  Stream-ordered behind this rank's own earlier
        sums, which are the only readers of that slot.  Until that exchange (or release()) the slot is outstanding: a plain exchange
        would overwrite it and is refused."""
        self.slot_call = self.calls
        return self.stage[self.calls & 1, self.rank]

    def release(self):
        """hands back the slot of grad_slot() when its in-slot exchange will not be made"""
        self.slot_call = None

    def _check(self, st, in_slot):
        """refuses a call that would sum the wrong data - before anything is enqueued or `calls` moves"""
        if in_slot and self.slot_call != self.calls:
            raise RuntimeError('one-shot all-reduce: in_slot=True but no grad_slot() was taken for this exchange')
        if not in_slot and self.slot_call is not None:
            raise RuntimeError('one-shot all-reduce: a plain exchange would overwrite the outstanding slot of grad_slot() (release() it)')
        if self.stream is not None and st != self.stream:
            raise RuntimeError('one-shot all-reduce: issued on stream %#x, but this exchanger runs on stream %#x (another stream needs '
                               'another tag)' % (st.cuda_stream, self.stream.cuda_stream))

    def _fence(self, st, phase, g, par):
        """everybody's writes of this phase (0: into the staging slots, 1: into the gather arrays) have landed before what this
        rank enqueues next"""
        if self.sync == 'host':
            st.synchronize()                            # my writes have landed ...
            dist.barrier()                              # ... and so have everybody else's
        elif self.world > 1:
            k = 4 * phase + par                         # W[par] / G[par]
            self.mine[g][k].record(st)
            self.shm.publish(phase, self.calls)         # host: "my record of exchange `calls` has been issued"
            for p, ev in self.theirs[g].items():        # behind every peer's writes - a stream wait, not a host wait
                self.shm.wait(p, phase, self.calls)
                st.wait_event(ev[k])

    def _finish(self, src, n_slots, flat, seg_sizes, sq_part):
        """the final rank-order sum (or, n_slots = 1, the copy out of the gather array); with sq_part also the clip's partial sums of
        squares of the result (mpg_sum_slots_sq: the bits mpg_sq_partials would produce from `flat`)"""
        L = self.L
        if sq_part is not None:
            import ctypes
            sizes = (ctypes.c_int * len(seg_sizes))(*[int(x) for x in seg_sizes])
            L.call('mpg_sum_slots_sq', L.ptr(src), L.c_int(n_slots), L.c_size_t(self.n), L.c_int(self.n), L.ptr(flat), sizes,
                   L.c_int(len(seg_sizes)), L.ptr(sq_part), L.stream())
        elif n_slots == 1:
            flat.copy_(src.reshape(-1)[:self.n], non_blocking=True)
        else:
            L.call('mpg_sum_slots', L.ptr(src), L.c_int(n_slots), L.c_int(self.n), L.ptr(flat), L.stream())

    def all_reduce_sum_(self, flat, in_slot=False, seg_sizes=None, sq_part=None):
        """flat <- sum over ranks.  in_slot: this rank's contribution already sits in grad_slot() (taken BEFORE this call) and `flat` is
        only the destination; seg_sizes + sq_part: see _finish."""
        assert flat.numel() == self.n and flat.dtype == torch.float32 and flat.is_contiguous()
        st = torch.cuda.current_stream()
        self._check(st, in_slot)
        self.stream, self.slot_call = st, None
        par = self.calls & 1
        self.calls += 1
        L = self.L
        two = self.mode == 'twoshot'
        me = self.rank
        lo, hi = self.slices[me]
        src = self.stage[par, me] if in_slot else flat
        it = self.calls
        g = (it - 1) // self.GEN_LEN
        events = self.sync == 'event' and self.world > 1
        if events:
            if (it - 1) % self.GEN_LEN == 0 and g > 0:  # generation boundary: open the peers' events of g, prepare g + 1, drop g - 2
                self._open_generation(g)
                self._make_generation(g + 1)
                self.mine.pop(g - 2, None)
                self.theirs.pop(g - 2, None)
            if self.s_events and it > 2:                # 0. behind the peers' reads of this parity (exchange it - 2)
                g2 = (it - 3) // self.GEN_LEN
                for p, ev in self.theirs[g2].items():
                    st.wait_event(ev[2 + par])

        def scatter():                                  # two-shot (A): slice p of my buffer into slot `rank` of rank p's array
            for p in range(self.world):
                a, b = self.slices[p]
                if b > a and not (in_slot and p == me):  # (in_slot: my own slice is where it belongs already)
                    self.peers[p][par, me, a:b].copy_(src[a:b], non_blocking=True)

        def spread():                                   # one-shot 1.: my buffer into slot `rank` of every rank's array
            for r in range(self.world):
                if not (in_slot and r == me):
                    self.peers[r][par, me].copy_(src, non_blocking=True)

        def reduce_and_gather():                        # two-shot (B): the rank-order sum of MY slice, then into every rank's gather array
            if hi > lo:
                L.call('mpg_sum_slots_strided', L.ptr(self.stage[par, 0, lo:hi]), L.c_int(self.world), L.c_size_t(self.n), L.c_int(hi - lo),
                       L.ptr(self.gath[par, lo:hi]), L.stream())
                for p in range(self.world):
                    if p != me:
                        self.peer_gath[p][par, lo:hi].copy_(self.gath[par, lo:hi], non_blocking=True)
        if two:
            scatter()
        else:
            spread()                                    # 1.
        self._fence(st, 0, g, par)                      # 2.
        if two:
            reduce_and_gather()                         # my slice, reduced, into every rank's gather array
            self._fence(st, 1, g, par)                  # behind every peer's slice
            result, n_slots = self.gath[par], 1
        else:
            result, n_slots = self.stage[par], self.world
        self._finish(result, n_slots, flat, seg_sizes, sq_part)     # 3.
        if events and self.s_events:
            self.mine[g][2 + par].record(st)            # S[par]: my reads of this parity's slots (and gather array) are done
        return flat


_oneshot_tag = 0


def backend():
    if not dist.is_initialized():
        return None
    return 'oneshot (IPC staging slots; process group: %s)' % dist.get_backend() if _exchange == 'oneshot' else dist.get_backend()


def world_size():
    return dist.get_world_size() if dist.is_initialized() else 1


def _exchanger(n, device, tag):
    ex = _oneshot.get((n, tag))
    if ex is None:         # (a collective construction: every rank reaches it at the same exchange of the same length)
        ex = _oneshot[(n, tag)] = OneShotAllReduce(n, device)
    return ex


def grad_slot(n, device, force=False, tag=0):
    """With the one-shot backend: the staging slot the NEXT exchange of an n-float buffer takes this rank's contribution from
    (OneShotAllReduce.grad_slot) - write the buffer there and pass in_slot=True to all_reduce_sum_.  None with any other backend
    (or without an exchange): the caller keeps its own buffer."""
    if dist.is_initialized() and (dist.get_world_size() > 1 or force) and _exchange == 'oneshot':
        return _exchanger(n, device, tag).grad_slot()
    return None


def release_slot(n, tag=0):
    """Hands back the slot of grad_slot(n, ...) when its in-slot exchange will not be made (a no-op when none is outstanding)."""
    ex = _oneshot.get((n, tag))
    if ex is not None:
        ex.release()


def all_reduce_sum_(flat, force=False, tag=0, in_slot=False, seg_sizes=None, sq_part=None):
    """In-place sum over ranks of one flat float32 buffer (no-op on a single process unless `force`: a one-rank group
    still runs the collective - the way the RCCL path is exercised on a 1-GPU box).  `tag`: exchanges that may be in flight at the
    same time (on different streams) must not share a one-shot exchanger - staging parities, events and shared-memory counters are
    per object - so concurrent callers pass distinct tags (mpg_amd/fused.py: 1 = the critics' slice under the sweep)."""
    if dist.is_initialized() and (dist.get_world_size() > 1 or force):
        if _exchange == 'oneshot':
            _exchanger(flat.numel(), flat.device, tag).all_reduce_sum_(flat, in_slot=in_slot, seg_sizes=seg_sizes, sq_part=sq_part)
            return flat
        assert not in_slot, 'in_slot is the one-shot backend\'s (grad_slot returned None)'
        dist.all_reduce(flat, op=dist.ReduceOp.SUM)
    return flat


def barrier():
    if dist.is_initialized() and dist.get_world_size() > 1:
        dist.barrier()


def max_over_ranks(x):
    if dist.is_initialized() and dist.get_world_size() > 1:
        dev = 'cuda' if dist.get_backend() == 'nccl' else 'cpu'
        t = torch.tensor([float(x)], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())
    return float(x)
