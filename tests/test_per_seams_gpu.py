"""The prioritized replay's trees and the replay ring on the device (mpg_amd/csrc/per_kernels.hip, replay_kernels.hip) at the sizes
where the kernels change shape, against the float64 host model and the cases of tests/per_seam_inputs.py (tests/test_per_seams.py
pins the model to the reference's recorded results and shows that every case reaches its seam).  After EVERY update: touched leaves
against the model to 4e-16 (pow), untouched leaves unchanged bit for bit, every internal node of both trees bit-equal to
O.heap_tree of the device's own leaves, stamp == -1 everywhere, *max_priority exactly the model's."""
import numpy as np
import pytest
import torch

from oracle import mpg_oracle as O
from tests import per_seam_inputs as S

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def dev(x, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dt).to(DEV)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.int32, 8: np.int64, 1: np.uint8}[x.dtype.itemsize])


def assert_same_bits(a, b, msg=''):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (msg, a.dtype, b.dtype, a.shape, b.shape)
    np.testing.assert_array_equal(bits(a), bits(b), err_msg=msg)


class DevPER(object):
    """the device's trees behind mpg_per_init / _update / _add / _sample, through L.call"""

    def __init__(self, cap, alpha=S.ALPHA, eps=S.EPS):
        import mpg_amd._lib as L
        self.L, self.cap, self.alpha, self.eps = L, cap, alpha, eps
        self.s = torch.full((2 * cap,), float('nan'), dtype=torch.float64, device=DEV)      # (mpg_per_init writes every element)
        self.m = torch.full((2 * cap,), float('nan'), dtype=torch.float64, device=DEV)
        self.stamp = torch.full((cap,), 12345, dtype=torch.int32, device=DEV)
        self.maxp = torch.ones(1, dtype=torch.float64, device=DEV)
        L.call('mpg_per_init', L.ptr(self.s), L.ptr(self.m), L.ptr(self.stamp), L.c_int(cap), L.stream())

    def update(self, idx, td, with_max=True):
        L = self.L
        d_idx, d_td = dev(idx, torch.int32), dev(td)
        L.call('mpg_per_update', L.ptr(self.s), L.ptr(self.m), L.ptr(self.stamp), L.c_int(self.cap), L.c_int(len(idx)), L.ptr(d_idx),
               L.ptr(d_td), L.c_double(self.alpha), L.c_double(self.eps), L.ptr(self.maxp if with_max else None), L.stream())
        torch.cuda.synchronize()

    def add(self, ring, start, n, max_priority):
        L = self.L
        self.maxp.fill_(max_priority)
        scratch = torch.full((n,), -7, dtype=torch.int32, device=DEV)
        L.call('mpg_per_add', L.ptr(self.s), L.ptr(self.m), L.ptr(self.stamp), L.c_int(self.cap), L.c_int(ring), L.c_int(start), L.c_int(n),
               L.c_double(self.alpha), L.ptr(self.maxp), L.ptr(scratch), L.stream())
        torch.cuda.synchronize()
        np.testing.assert_array_equal(scratch.cpu().numpy(), (start + np.arange(n)) % ring)

    def sample(self, n_storage, n, u=None, seed=0, ctr=0, beta=0.4, weights=True):
        L = self.L
        idx = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        w = torch.full((n,), float('nan'), dtype=torch.float32, device=DEV) if weights else None
        d_u = None if u is None else dev(u, torch.float64)
        L.call('mpg_per_sample', L.ptr(self.s), L.ptr(self.m), L.c_int(self.cap), L.c_int(n_storage), L.c_int(n), L.ptr(d_u),
               L.c_u64(seed), L.c_u64(ctr), L.c_double(beta), L.ptr(idx), L.ptr(w), L.stream())
        torch.cuda.synchronize()
        return idx.cpu().numpy(), (w.cpu().numpy() if weights else None)

    def host(self):
        return self.s.cpu().numpy(), self.m.cpu().numpy(), self.stamp.cpu().numpy(), float(self.maxp.item())


def check_state(d, model, before, touched, what):
    """every property the issue asks for after a call; returns the device's (sum leaves, min leaves) for the next call's `before`"""
    cap = d.cap
    s, m, stamp, maxp = d.host()
    ls, lm = s[cap:].copy(), m[cap:].copy()
    mask = np.zeros(cap, bool)
    mask[touched] = True
    np.testing.assert_allclose(ls[mask], model.leaves[mask], rtol=4e-16, atol=0, err_msg=what + ': touched leaves')
    assert_same_bits(lm, np.where(model.written, ls, np.inf), what + ': min leaves')
    assert_same_bits(ls[~mask], before[0][~mask], what + ': untouched sum leaves')
    assert_same_bits(lm[~mask], before[1][~mask], what + ': untouched min leaves')
    assert_same_bits(s[1:cap], O.heap_tree(ls, np.add)[1:cap], what + ': sum tree nodes')
    assert_same_bits(m[1:cap], O.heap_tree(lm, np.minimum)[1:cap], what + ': min tree nodes')
    assert s[0] == 0.0 and m[0] == np.inf, what + ': node 0'
    leaked = np.flatnonzero(stamp != -1)
    assert leaked.size == 0, '%s: %d stamps left, first at leaf %d = %d' % (what, leaked.size, leaked[0], stamp[leaked[0]])
    assert maxp == model.max_priority, '%s: max priority %r, model %r' % (what, maxp, model.max_priority)
    return ls, lm


def fresh(cap, **kw):
    d, model = DevPER(cap, **kw), S.HostPER(cap, **kw)
    s, m, stamp, _ = d.host()
    assert np.all(s == 0.0) and np.all(m == np.inf) and np.all(stamp == -1)
    return d, model, (s[cap:].copy(), m[cap:].copy())


# ---- a. updates ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_max', [True, False], ids=['max_priority', 'max_priority_null'])
@pytest.mark.parametrize('cap', S.UPDATE_CAPS)
def test_update_sequences_against_the_host_model(cap, with_max):
    """mpg_per_update: the fill (a full rebuild), then batches of 1, capacity / 64 and capacity / 64 + 1 entries (touched paths up to
    equality, a rebuild past it; at 2^17 also 1025 and 2048 entries on the paths and 2049 rebuilt; at 2^21 one rebuilt batch).  Every
    batch with room holds an entry with the largest |td| so far that a later duplicate overrides: it counts towards *max_priority
    (buffer.py:182-189) and leaves no trace in the leaves."""
    case = S.update_case(cap)
    d, model, before = fresh(cap)
    for k, (idx, td) in enumerate([case['fill']] + [(i, t) for i, t, _ in case['batches']]):
        d.update(idx, td, with_max)
        touched = model.update(idx, td, track_max=with_max)
        what = 'capacity %d, call %d (n = %d, %s)' % (cap, k, len(idx), 'paths' if S.takes_paths(len(idx), cap) else 'rebuild')
        before = check_state(d, model, before, touched, what)
    assert with_max or model.max_priority == 1.0


@pytest.mark.parametrize('cap', S.UPDATE_CAPS)
def test_add_sequences_against_the_host_model(cap):
    """mpg_per_add: the same sizes as slots of a ring that is no power of two, wrapping past its end, each call at a max priority of
    its own (leaf = max_priority ** alpha in float64; the value itself stays as it is)."""
    case = S.add_case(cap)
    d, model, before = fresh(cap)
    for k, (start, n, mp) in enumerate(case['calls']):
        model.max_priority = mp
        d.add(case['ring'], start, n, mp)
        touched = model.add(case['ring'], start, n)
        before = check_state(d, model, before, touched, 'capacity %d, add %d (start %d, n = %d)' % (cap, k, start, n))


# ---- b. sampling ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cap', S.SAMPLE_CAPS)
def test_tie_family_goes_right_on_equality(cap):
    """All leaves 1.0, u_j = j / capacity: the mass equals the prefix sum of the first j leaves exactly, where the reference's
    `left > prefix` goes right (segment_tree.py:133-140) - index j, in the staged descent and in the one that reads memory."""
    d, model, before = fresh(cap, eps=0.0)
    d.update(np.arange(cap), np.ones(cap, np.float32))
    check_state(d, model, before, model.update(np.arange(cap), np.ones(cap, np.float32)), 'ones')
    s = d.host()[0]
    assert np.all(s[cap:] == 1.0) and s[1] == float(cap)
    js = S.tie_js(cap)
    u = js / float(cap)
    idx, w = d.sample(cap, js.size, u=u)
    np.testing.assert_array_equal(idx, O.find_prefixsum_idx_batch(s, u * s[1]))
    np.testing.assert_array_equal(idx, js)
    assert np.all(w == np.float32(1.0))                                   # equal leaves: every weight is pow(1, -beta) / pow(1, -beta)
    np.testing.assert_array_equal(d.sample(cap, 1, u=[0.0])[0], [0])
    np.testing.assert_array_equal(d.sample(cap, 1, u=[1.0], weights=False)[0], [cap - 1])
    np.testing.assert_array_equal(d.sample(cap, 3, u=[1.0, 0.0, 1.0], weights=False)[0], [cap - 1, 0, cap - 1])


@pytest.mark.parametrize('cap', S.SAMPLE_CAPS)
def test_library_draws_against_the_oracle_descent(cap):
    """u = NULL: the kernel's own Philox uniforms (O.per_uniform_philox) on random priorities, n_storage 1, capacity / 2 + 1 and
    capacity.  Indices exact against the reference's descent on the device's tree; IS weights to 2e-6 (float32), exactly 1 at beta 0."""
    for ns in S.sample_storages(cap):
        d, model, before = fresh(cap)
        td = S.sample_priorities(cap, ns)
        d.update(np.arange(ns), td)
        check_state(d, model, before, model.update(np.arange(ns), td), 'capacity %d, %d filled' % (cap, ns))
        st, mt = d.host()[:2]
        seen = []
        for n, seed, ctr in S.library_draws():
            expect = O.find_prefixsum_idx_batch(st, O.per_uniform_philox(n, seed, ctr) * st[1])
            for beta in S.SAMPLE_BETAS:
                what = 'capacity %d, %d filled, n = %d, seed %#x, ctr %#x, beta %g' % (cap, ns, n, seed, ctr, beta)
                idx, w = d.sample(ns, n, seed=seed, ctr=ctr, beta=beta)
                np.testing.assert_array_equal(idx, expect, err_msg=what)
                np.testing.assert_allclose(w, S.is_weights(st, mt, idx, ns, beta), rtol=2e-6, atol=0, err_msg=what)
                if beta == 0.0:
                    assert np.all(w == np.float32(1.0)), what
            idx_only, _ = d.sample(ns, n, seed=seed, ctr=ctr, weights=False)
            np.testing.assert_array_equal(idx_only, expect)
            seen.append(expect)
        seen = np.concatenate(seen)
        assert ns == 1 or (0 in seen and ns - 1 in seen)


# ---- c. draw + gather in one launch --------------------------------------------------------------------------------------------
def device_ring(arrays):
    return [dev(a, torch.uint8 if a.dtype == np.uint8 else torch.float32) for a in arrays]


def nan_outputs(n, od, ad):
    return [torch.full(shape, float('nan'), dtype=torch.float32, device=DEV) for shape in ((n, od), (n, ad), (n,), (n, od), (n,))]


def replay_gather(idx, od, ad, ring, with_done=True):
    import mpg_amd._lib as L
    out = nan_outputs(len(idx), od, ad)
    d_idx = dev(idx, torch.int32)
    L.call('mpg_replay_gather', L.c_int(len(idx)), L.ptr(d_idx), L.c_int(od), L.c_int(ad), *[L.ptr(r) for r in ring],
           *[L.ptr(o) for o in out[:4]], L.ptr(out[4] if with_done else None), L.stream())
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def sample_gather(d, ns, n, od, ad, ring, u=None, seed=0, ctr=0, beta=0.4, with_done=True):
    import mpg_amd._lib as L
    out = nan_outputs(n, od, ad)
    idx = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    w = torch.full((n,), float('nan'), dtype=torch.float32, device=DEV)
    d_u = None if u is None else dev(u, torch.float64)
    L.call('mpg_per_sample_gather', L.ptr(d.s), L.ptr(d.m), L.c_int(d.cap), L.c_int(ns), L.c_int(n), L.ptr(d_u), L.c_u64(seed), L.c_u64(ctr),
           L.c_double(beta), L.ptr(idx), L.ptr(w), L.c_int(od), L.c_int(ad), *[L.ptr(r) for r in ring], *[L.ptr(o) for o in out[:4]],
           L.ptr(out[4] if with_done else None), L.stream())
    torch.cuda.synchronize()
    return idx.cpu().numpy(), w.cpu().numpy(), [o.cpu().numpy() for o in out]


@pytest.mark.parametrize('od,ad', S.WIDTHS)
def test_sample_gather_equals_sample_then_gather(od, ad):
    """mpg_per_sample_gather == mpg_per_sample + mpg_replay_gather on all seven outputs, at both register widths of gather_row, with
    n_storage < capacity; a caller's u = 1 ends in the last FILLED slot (mpg_per_sample keeps find_prefixsum_idx's rightmost leaf)."""
    cap, ns, n = 2048, 1500, 257
    seed, ctr = S.SAMPLE_KEYS[0]
    d, model, before = fresh(cap)
    td = S.sample_priorities(cap, ns)
    d.update(np.arange(ns), td)
    check_state(d, model, before, model.update(np.arange(ns), td), 'fill')
    host = S.HostRing(cap, od, ad)
    host.add(0, *S.ring_rows(np.random.Generator(np.random.PCG64(300 + od)), ns, od, ad))
    ring = device_ring(host.arrays())
    idx, w = d.sample(ns, n, seed=seed, ctr=ctr)
    rows = replay_gather(idx, od, ad, ring)
    g_idx, g_w, g_rows = sample_gather(d, ns, n, od, ad, ring, seed=seed, ctr=ctr)
    np.testing.assert_array_equal(g_idx, idx)
    assert_same_bits(g_w, w, 'IS weights')
    for name, a, b, ref in zip(('obs', 'act', 'rew', 'obs2', 'done'), g_rows, rows, host.gather(idx)):
        assert_same_bits(a, b, name + ': one launch against two')
        assert_same_bits(a, ref, name + ': against the ring')
    assert 0 in idx and ns - 1 in idx
    _, _, no_done = sample_gather(d, ns, n, od, ad, ring, seed=seed, ctr=ctr, with_done=False)
    for a, b in zip(no_done[:4], g_rows[:4]):
        assert_same_bits(a, b, 'o_done = NULL')
    assert np.all(np.isnan(no_done[4]))
    u = np.array([1.0, 0.0, 1.0])
    np.testing.assert_array_equal(d.sample(ns, 3, u=u)[0], [cap - 1, 0, cap - 1])
    e_idx, e_w, e_rows = sample_gather(d, ns, 3, od, ad, ring, u=u)
    np.testing.assert_array_equal(e_idx, [ns - 1, 0, ns - 1])
    st, mt = d.host()[:2]
    np.testing.assert_allclose(e_w, S.is_weights(st, mt, e_idx, ns, 0.4), rtol=2e-6, atol=0)
    for name, a, ref in zip(('obs', 'act', 'rew', 'obs2', 'done'), e_rows, host.gather(e_idx)):
        assert_same_bits(a, ref, name + ': u = 1')


# ---- d. the ring ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('od,ad', S.WIDTHS)
def test_ring_add_and_gather_against_a_numpy_mirror(od, ad):
    """mpg_replay_add / mpg_replay_gather, bit for bit: a wrapping add, n == capacity from the last slot, an add without dones (they
    become 1), a gather of more than one block with both ends of the ring, and one without the done output."""
    import mpg_amd._lib as L
    cap = 300
    rng = np.random.Generator(np.random.PCG64(400 + od))
    host = S.HostRing(cap, od, ad)
    ring = device_ring(host.arrays())
    for k, (next_idx, n, with_done) in enumerate(((0, 100, True), (100, 250, True), (cap - 1, cap, True), (290, 37, False))):
        rows = S.ring_rows(rng, n, od, ad)
        staged = device_ring(rows)
        L.call('mpg_replay_add', L.c_int(cap), L.c_int(next_idx), L.c_int(n), L.c_int(od), L.c_int(ad), *[L.ptr(x) for x in staged[:4]],
               L.ptr(staged[4] if with_done else None), *[L.ptr(r) for r in ring], L.stream())
        torch.cuda.synchronize()
        host.add(next_idx, *rows[:4], rows[4] if with_done else None)
        for name, a, ref in zip(('obs', 'act', 'rew', 'obs2', 'done'), ring, host.arrays()):
            assert_same_bits(a.cpu().numpy(), ref, 'add %d: %s' % (k, name))
    assert np.all(host.done[np.arange(290, 327) % cap] == 1) and 0 in host.done
    idx = rng.integers(0, cap, 257)
    idx[:2] = (0, cap - 1)
    got, ref = replay_gather(idx, od, ad, ring), host.gather(idx)
    for name, a, b in zip(('obs', 'act', 'rew', 'obs2', 'done'), got, ref):
        assert_same_bits(a, b, 'gather: ' + name)
    got = replay_gather(idx, od, ad, ring, with_done=False)
    for name, a, b in zip(('obs', 'act', 'rew', 'obs2'), got, ref):
        assert_same_bits(a, b, 'gather without dones: ' + name)
    assert np.all(np.isnan(got[4]))


def uniform_indices(ns, n, seed, ctr):
    import mpg_amd._lib as L
    idx = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    L.call('mpg_uniform_indices', L.c_int(ns), L.c_int(n), L.c_u64(seed), L.c_u64(ctr), L.ptr(idx), L.stream())
    torch.cuda.synchronize()
    return idx.cpu().numpy()


def sample_uniform(ns, n, seed, ctr, od, ad, ring):
    import mpg_amd._lib as L
    out = nan_outputs(n, od, ad)
    idx = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    L.call('mpg_replay_sample_uniform', L.c_int(ns), L.c_int(n), L.c_u64(seed), L.c_u64(ctr), L.c_int(od), L.c_int(ad),
           *[L.ptr(r) for r in ring], L.ptr(idx), *[L.ptr(o) for o in out], L.stream())
    torch.cuda.synchronize()
    return idx.cpu().numpy(), [o.cpu().numpy() for o in out]


@pytest.mark.parametrize('ns', S.UNIFORM_STORAGES)
def test_uniform_draws_against_the_oracle(ns):
    """mpg_uniform_indices and mpg_replay_sample_uniform against O.uniform_indices_philox (word i & 3 of block i >> 2, multiply-shift
    into [0, n_storage)), up to n_storage = 2^31 - 1.  The largest storage is ONE int32 array that holds its own row numbers, passed as
    every array of a ring of width 1 (the kernels only read the ring): row s then holds s in every float array, bit for bit, and
    byte s of the array as its done flag."""
    if ns <= 1000:
        od, ad = 9, 2
        host = S.HostRing(ns, od, ad)
        host.add(0, *S.ring_rows(np.random.Generator(np.random.PCG64(500 + ns)), ns, od, ad))
        ring = device_ring(host.arrays())
    else:
        od, ad = 1, 1
        rows = torch.arange(0, ns, dtype=torch.int32, device=DEV)
        assert rows.numel() == ns and int(rows[-1].item()) == ns - 1
        as_float, as_bytes = rows.view(torch.float32), rows.view(torch.uint8)
        ring = [as_float, as_float, as_float, as_float, as_bytes]
    for seed, ctr in S.UNIFORM_KEYS:
        for n in S.UNIFORM_NS:
            expect = O.uniform_indices_philox(ns, n, seed, ctr)
            assert expect.min() >= 0 and expect.max() < ns               # (checked before the gathering launch reads those rows)
            np.testing.assert_array_equal(uniform_indices(ns, n, seed, ctr), expect)
            idx, got = sample_uniform(ns, n, seed, ctr, od, ad, ring)
            np.testing.assert_array_equal(idx, expect)
            if ns <= 1000:
                ref = host.gather(expect)
            else:
                where = torch.as_tensor(expect, device=DEV)
                r = rows[where].cpu().numpy()
                np.testing.assert_array_equal(r, expect)
                r = r.view(np.float32)
                ref = (r[:, None], r[:, None], r, r[:, None], as_bytes[where].cpu().numpy().astype(np.float32))
            for name, a, b in zip(('obs', 'act', 'rew', 'obs2', 'done'), got, ref):
                assert_same_bits(a, b, 'n_storage %d, n = %d: %s' % (ns, n, name))
    if ns > 1000:
        del ring, as_float, as_bytes, rows
        torch.cuda.empty_cache()
