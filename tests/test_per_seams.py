"""CPU half of the prioritized-replay seam tests (tests/per_seam_inputs.py): the float64 host model against the results that the
reference's own SegmentTree / PrioritizedReplayBuffer recorded, and the conditions under which the cases reach the seams they are
named after.  The conditions are requirements on the inputs, not measurements: if a seed misses one, the seed changes."""
import numpy as np
import pytest

from oracle import mpg_oracle as O
from tests import per_seam_inputs as S


# ---- the host model against the reference's recorded results -------------------------------------------------------------------
def test_host_model_vs_reference_segment_tree(golden):
    """segment_tree_ref.npz: 700 float64 priorities ** 0.6 set one by one, find_prefixsum_idx of 512 masses, 100 more sets with
    duplicate indices, the descent again, and the two ends of the mass range.  Totals, minima and every index exact."""
    g = golden('segment_tree_ref.npz')
    cap, n = int(g['capacity']), int(g['n'])
    m = S.HostPER(cap, alpha=float(g['alpha']), eps=0.0)
    m.update(np.arange(n), g['prios'], dtype=np.float64)                # (the fixture's priorities are float64 and hold their eps)
    np.testing.assert_allclose(m.leaves[:n], [float(p) ** float(g['alpha']) for p in g['prios']], rtol=4e-16)
    st, mt = m.trees()
    assert st[1] == float(g['total']) and mt[1] == float(g['min_all'])
    np.testing.assert_array_equal(m.draw(g['u']), g['idx'])
    m.update(g['upd_idx'], g['upd_p'], dtype=np.float64)
    st, mt = m.trees()
    assert st[1] == float(g['total2']) and mt[1] == float(g['min_all2'])
    np.testing.assert_array_equal(m.draw(g['u']), g['idx2'])
    np.testing.assert_array_equal(m.draw([0.0, 1.0]), g['edge_idx'])
    assert m.max_priority == max(1.0, float(np.max(np.concatenate([g['prios'], g['upd_p']]))))


def test_host_model_vs_reference_prioritized_buffer(golden):
    """per_buffer_ref.npz: the reference's PrioritizedReplayBuffer methods, unmodified - 500 adds at max priority, a draw, float32 TD
    errors as priorities, 300 adds through the wrapping 700-slot ring, a draw, priorities with duplicate indices, a draw.  Leaves to
    4e-16, drawn indices, totals, minima and both max priorities exact, IS weights to 1e-15."""
    g = golden('per_buffer_ref.npz')
    cap, tcap, B, beta = int(g['capacity']), int(g['tree_capacity']), int(g['B']), float(g['beta'])
    m = S.HostPER(tcap, alpha=float(g['alpha']), eps=float(g['eps']))

    def draw(k, n_storage):
        st, mt = m.trees()
        assert st[1] == float(g['draw%d_total' % k]) and mt[1] == float(g['draw%d_min' % k])
        idx = m.draw(g['u'][k])
        np.testing.assert_array_equal(idx, g['draw%d_idx' % k])
        np.testing.assert_allclose(m.weights(idx, n_storage, beta), g['draw%d_weights' % k], rtol=1e-15)
        return idx
    m.add(cap, 0, 500)
    np.testing.assert_allclose(m.leaves, g['leaves_a'], rtol=4e-16)
    idx = draw(0, 500)
    assert idx.size == B
    m.update(idx, g['td'][0])
    np.testing.assert_allclose(m.leaves, g['leaves_b'], rtol=4e-16)
    assert m.max_priority == float(g['max_priority_b'])
    m.add(cap, 500, 300)
    assert (500 + 300) % cap == int(g['next_idx_c'])
    np.testing.assert_allclose(m.leaves, g['leaves_c'], rtol=4e-16)
    draw(1, cap)
    m.update(g['update2_idx'], g['td'][1])
    np.testing.assert_allclose(m.leaves, g['leaves_d'], rtol=4e-16)
    assert m.max_priority == float(g['max_priority_d'])
    draw(2, cap)


def test_host_model_takes_the_last_duplicate_and_counts_every_entry():
    m = S.HostPER(8, alpha=0.5, eps=0.25)
    touched = m.update([3, 5, 3, 3], np.array([9.0, -2.0, 100.0, 0.75], np.float32))
    np.testing.assert_array_equal(touched, [3, 5])
    assert m.leaves[3] == 1.0 and m.leaves[5] == 1.5 and m.max_priority == 100.25
    np.testing.assert_array_equal(m.min_leaves()[[0, 3, 5]], [np.inf, 1.0, 1.5])
    m.update([0], np.array([500.0], np.float32), track_max=False)
    assert m.max_priority == 100.25
    np.testing.assert_array_equal(m.add(6, 4, 4), [0, 1, 4, 5])
    assert m.leaves[1] == 100.25 ** 0.5 and m.leaves[0] == m.leaves[5] == m.leaves[1] and m.leaves[3] == 1.0


# ---- the update cases reach their seams ----------------------------------------------------------------------------------------
def test_update_case_table_reaches_every_kernel_shape():
    assert S.UPDATE_CAPS == (1, 2, 64, 512, 1024, 2048, 4096, 1 << 17, 1 << 21)
    for cap in S.UPDATE_CAPS:
        ns, sizes = S.n_storage_of(cap), S.batch_sizes(cap)
        assert 1 <= ns <= cap and (cap <= 2 or ns & (ns - 1) != 0), (cap, ns)
        if cap == S.BIG_CAP:
            continue
        assert 1 in sizes
        if cap >= S.PATHS_RATIO:                               # both sides of `n * 64 <= capacity`
            at, past = cap // S.PATHS_RATIO, cap // S.PATHS_RATIO + 1
            assert at in sizes and past in sizes
            assert at * S.PATHS_RATIO == cap and past * S.PATHS_RATIO == cap + S.PATHS_RATIO
            assert S.takes_paths(at, cap) and not S.takes_paths(past, cap)
    # one workgroup with nsub_leaves = capacity; the smallest top rebuilds; the top's stride loop (its block is 512 threads)
    assert [c for c in S.UPDATE_CAPS if c < S.SUB] == [1, 2, 64, 512]
    assert [c // S.SUB for c in (2048, 4096)] == [2, 4]
    assert S.BIG_CAP // S.SUB // 2 > 512
    assert S.batch_sizes(S.BIG_CAP) == (S.BIG_CAP // 64 + 1,) and not S.takes_paths(S.batch_sizes(S.BIG_CAP)[0], S.BIG_CAP)
    # one thread of k_update_paths serves several entries of a level
    strided = [n for n in S.batch_sizes(1 << 17) if n > S.PATHS_BLOCK and S.takes_paths(n, 1 << 17)]
    assert strided == [1025, 2048]
    assert 2049 in S.batch_sizes(1 << 17) and not S.takes_paths(2049, 1 << 17)


@pytest.mark.parametrize('cap', S.UPDATE_CAPS)
def test_update_batches_hold_what_they_are_named_after(cap):
    case = S.update_case(cap)
    ns = case['n_storage']
    m = S.HostPER(cap)
    idx, td = case['fill']
    np.testing.assert_array_equal(idx, np.arange(ns))
    m.update(idx, td)
    seen_lo, seen_hi = np.abs(td).min(), np.abs(td).max()
    for b, (idx, td, hidden) in enumerate(case['batches']):
        n = idx.size
        assert td.dtype == np.float32 and np.all(np.isfinite(td)) and idx.min() >= 0 and idx.max() < ns
        assert np.abs(td).min() >= np.float32(1e-6) and np.abs(td).max() <= np.float32(1e3)
        seen_lo, seen_hi = min(seen_lo, np.abs(td).min()), max(seen_hi, np.abs(td).max())
        p = np.array(m.priorities(td))
        if n == 1:
            assert hidden is None and idx[0] in (0, ns - 1)
        else:
            # the overridden maximum: above every other entry of the batch and above the running maximum; its survivor is smaller
            assert hidden == 0 and idx[0] == idx[n - 1]
            assert p[0] > p[1:].max() and p[0] > m.max_priority and p[n - 1] < p[0]
            owners = S.HostPER.last_occurrence(idx)
            assert 0 not in owners and max(m.max_priority, p[owners].max()) < p[0]       # what a maximum over owners alone gives
        if n >= 5 and ns >= 3:
            assert idx[2] == idx[1] + 1 and idx[3] == idx[1] + 2
        if n >= 7:
            assert 0 in idx and ns - 1 in idx
        if n >= 12:
            assert np.unique(idx).size <= n - (n - 6) // 4 and np.any(td[6:6 + (n - 6) // 4] != td[6 + 2 * ((n - 6) // 4):6 + 3 * ((n - 6) // 4)])
        before = m.max_priority
        m.update(idx, td)
        assert m.max_priority == max(before, p.max()) and (n == 1 or m.max_priority == p[0])
    if len(case['batches']) == 4:
        assert seen_hi == np.float32(1e3)
    assert seen_lo <= np.float32(1.1e-6) or ns < 64
    # leaf 0 and leaf n_storage - 1 are written by some batch at every capacity
    every = np.concatenate([x[0] for x in case['batches']])
    assert 0 in every and (ns - 1 in every or len(case['batches']) == 1)


@pytest.mark.parametrize('cap', S.UPDATE_CAPS)
def test_add_cases_wrap_a_ring_that_is_no_power_of_two(cap):
    case = S.add_case(cap)
    ring = case['ring']
    assert ring <= cap and (cap <= 2 or ring & (ring - 1) != 0)
    assert case['calls'][0] == (0, ring, 1.0) and [n for _, n, _ in case['calls'][1:]] == list(S.batch_sizes(cap))
    for start, n, mp in case['calls'][1:]:
        assert 0 <= start < ring and mp > 0
        if n >= 2 and ring >= 2:
            assert start + n > ring, 'the slots do not wrap'
    assert len(set(mp for _, _, mp in case['calls'])) == len(case['calls'])


# ---- the sampling cases reach their seams --------------------------------------------------------------------------------------
def _descent_ge(tree, mass):
    """the descent with `left >= prefix`: what the tie family must tell from the reference's `>`"""
    cap = tree.size // 2
    node, prefix = np.ones(mass.size, np.int64), np.array(mass, np.float64)
    while node[0] < cap:
        left = tree[2 * node]
        go_left = left >= prefix
        prefix = np.where(go_left, prefix, prefix - left)
        node = np.where(go_left, 2 * node, 2 * node + 1)
    return node - cap


@pytest.mark.parametrize('cap', S.SAMPLE_CAPS)
def test_tie_family_lands_on_prefix_sums(cap):
    m = S.HostPER(cap, eps=0.0)
    m.update(np.arange(cap), np.ones(cap, np.float32))
    assert np.all(m.leaves == 1.0)
    st, _ = m.trees()
    js = S.tie_js(cap)
    u = js / float(cap)
    assert st[1] == float(cap) and np.all(u * st[1] == js)                # exact: every mass equals a prefix sum of the leaves
    np.testing.assert_array_equal(O.find_prefixsum_idx_batch(st, u * st[1]), js)        # the reference goes RIGHT on equality
    np.testing.assert_array_equal(m.draw([0.0, 1.0]), [0, cap - 1])
    if cap > 1:
        assert np.all(_descent_ge(st, u * st[1])[js > 0] != js[js > 0])  # `>=` lands elsewhere for every j > 0
    if cap <= S.TOPN:
        np.testing.assert_array_equal(js, np.arange(cap))
    else:
        assert set((1023, 1024, 1025, cap - 1025, cap - 1024, cap - 1023, cap - 1)) <= set(js.tolist()) and js.size < 1024


@pytest.mark.parametrize('cap', S.SAMPLE_CAPS)
def test_library_draws_reach_both_ends_and_the_unstaged_levels(cap):
    assert S.SAMPLE_NS == (1, 255, 257, 1000) and S.SAMPLE_BETAS == (0.0, 0.4, 1.0) and len(S.SAMPLE_KEYS) == 2
    assert all(seed >> 32 and ctr >> 32 for seed, ctr in S.SAMPLE_KEYS)
    assert set(S.sample_storages(cap)) == set(x for x in (1, cap // 2 + 1, cap) if x <= cap)
    for ns in S.sample_storages(cap):
        td = S.sample_priorities(cap, ns)
        assert td.size == ns and np.all(np.isfinite(td)) and np.all(td != 0)
        m = S.HostPER(cap)
        m.update(np.arange(ns), td)
        st, mt = m.trees()
        drawn, n_left, n_right = [], 0, 0
        for n, seed, ctr in S.library_draws():
            u = O.per_uniform_philox(n, seed, ctr)
            assert u.size == n and 0.0 < u.min() and u.max() < 1.0
            idx, nl, nr = S.descent_turns(st, u * st[1], S.TOPN // 2)
            np.testing.assert_array_equal(idx, O.find_prefixsum_idx_batch(st, u * st[1]))
            assert idx.max() < ns                                         # (no draw leans on the device's clamp to the filled slots)
            w = S.is_weights(st, mt, idx, ns, 0.4)
            assert np.all(np.isfinite(w)) and w.max() <= 1.0 + 1e-12 and w.min() > 1e-30
            drawn.append(idx)
            n_left, n_right = n_left + nl, n_right + nr
        drawn = np.concatenate(drawn)
        if ns > 1:
            assert 0 in drawn and ns - 1 in drawn, (cap, ns)
        if cap >= S.TOPN:                                                 # a left and a right turn at the first level read from memory
            assert n_left > 0 and (n_right > 0 or ns == 1), (cap, ns, n_left, n_right)      # (one filled leaf: leaf 0, all turns left)
        else:
            assert n_left == n_right == 0


def test_ring_and_uniform_case_tables():
    assert S.WIDTHS == ((4, 1), (8, 2), (9, 2), (11, 1), (16, 2))
    assert S.UNIFORM_STORAGES == (1, 2, 3, 1000, 2 ** 31 - 1) and S.UNIFORM_NS == (1, 3, 4, 5, 257)
    assert all(seed >> 32 and ctr >> 32 for seed, ctr in S.UNIFORM_KEYS)
    for ns in S.UNIFORM_STORAGES:
        for seed, ctr in S.UNIFORM_KEYS:
            idx = O.uniform_indices_philox(ns, 257, seed, ctr)
            assert idx.min() >= 0 and idx.max() < ns
            for n in S.UNIFORM_NS:                                        # row i's draw does not depend on the batch size
                np.testing.assert_array_equal(O.uniform_indices_philox(ns, n, seed, ctr), idx[:n])
    assert O.uniform_indices_philox(2 ** 31 - 1, 257, *S.UNIFORM_KEYS[0]).max() > 2 ** 30      # (the large storage is really used)
    r = S.HostRing(5, 3, 1)
    rows = S.ring_rows(np.random.Generator(np.random.PCG64(1)), 4, 3, 1)
    r.add(3, *rows[:4], None)
    np.testing.assert_array_equal(r.done, [1, 1, 0, 1, 1])
    np.testing.assert_array_equal(r.obs[[3, 4, 0, 1]], rows[0])
    r.add(4, *rows)
    np.testing.assert_array_equal(r.done[[4, 0, 1, 2]], rows[4])
    np.testing.assert_array_equal(r.gather(np.array([4, 2]))[4], rows[4][[0, 3]].astype(np.float32))
