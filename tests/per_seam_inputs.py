"""A float64 host model of the prioritized replay's tree state, and the cases that drive the kernels of mpg_amd/csrc/per_kernels.hip
and replay_kernels.hip through the sizes at which they change shape.  Shared by tests/test_per_seams.py (CPU: the model against the
reference's recorded results, and the conditions that make the device test worth running) and tests/test_per_seams_gpu.py (the
kernels against the model on these cases).  A plain helper module.

The seams (per_kernels.hip):
  k_rebuild_bottom / k_rebuild_top (SUB = 1024)   capacity < 1024: one workgroup with nsub_leaves = capacity; 2048 / 4096: the smallest
                                                  top rebuilds (ntop 2 and 4); >= 2^21: ntop / 2 > blockDim, the stride loop of the top;
  mpg_per_update, `n * 64 <= capacity`            touched paths on one side of equality, full rebuild on the other; n > 1024: one thread
                                                  of k_update_paths serves several entries per level;
  k_sample (TOPN = 2048)                          capacity <= 1024: the whole tree is staged in LDS; 2048: the first unstaged level;
                                                  1: no descent at all; `left > prefix`: the reference goes RIGHT on equality;
  stamp[]                                         -1 everywhere after every update (k_unstamp / k_rebuild_bottom);
  *max_priority                                   max(previous, |td| + eps over EVERY entry), overridden duplicates included
                                                  (buffer.py:182-189 runs max() once per entry).
The model is made of oracle/mpg_oracle.py's pieces only (heap_tree, find_prefixsum_idx_batch, per_uniform_philox, the IS-weight formula
of per_is_weights, uniform_indices_philox)."""
import functools

import numpy as np

from oracle import mpg_oracle as O

ALPHA, EPS = 0.6, 1e-6
SUB, TOPN, PATHS_RATIO, PATHS_BLOCK = 1024, 2048, 64, 1024      # per_kernels.hip: SUB, TOPN, `n * 64 <= capacity`, k_update_paths' block


# ---- the host model ----------------------------------------------------------------------------------------------------------
class HostPER(object):
    """PrioritizedReplayBuffer's tree state (buffer.py:94-189) in float64: the leaves, which of them were ever written (the others are
    the neutral elements: 0 in the sum tree, +inf in the min tree) and the running max priority.
      update(idx, td)          leaf[idx[i]] = (|float32(td[i])| + eps) ** alpha in python floats, the last duplicate wins;
                               max_priority = max(previous, max over ALL entries of |td| + eps)      (buffer.py:166-189)
      add(ring, start, n)      slots (start + i) % ring enter at max_priority ** alpha                   (buffer.py:127-136)
      trees()                  O.heap_tree of the leaves: (sum heap, min heap)
      draw(u, n_storage)       O.find_prefixsum_idx_batch(u * total)                                     (buffer.py:138-144)
      weights(idx, n, beta)    per_is_weights' formula                                                    (buffer.py:146-160)"""

    def __init__(self, capacity, alpha=ALPHA, eps=EPS, max_priority=1.0):
        assert capacity > 0 and capacity & (capacity - 1) == 0
        self.cap, self.alpha, self.eps = capacity, float(alpha), float(eps)
        self.leaves = np.zeros(capacity, np.float64)
        self.written = np.zeros(capacity, bool)
        self.max_priority = float(max_priority)

    @staticmethod
    def last_occurrence(idx):
        """positions of the entries that survive a sequential loop over idx: the last one of every index"""
        idx = np.asarray(idx, np.int64)
        _, first_rev = np.unique(idx[::-1], return_index=True)
        return np.sort(idx.size - 1 - first_rev)

    def priorities(self, td, dtype=np.float32):
        """|td| + eps per entry as python floats; td is read as `dtype` first (the device reads float32)"""
        return [abs(float(x)) + self.eps for x in np.asarray(td, dtype)]

    def update(self, idx, td, track_max=True, dtype=np.float32):
        idx = np.asarray(idx, np.int64)
        p = self.priorities(td, dtype)
        assert idx.size == len(p) and idx.min() >= 0 and idx.max() < self.cap and min(p) > 0      # buffer.py:183-184
        for k in self.last_occurrence(idx):
            self.leaves[idx[k]] = p[k] ** self.alpha
        self.written[idx] = True
        if track_max:
            self.max_priority = max(self.max_priority, max(p))
        return np.unique(idx)

    def add(self, ring_capacity, start, n):
        slots = (start + np.arange(n, dtype=np.int64)) % ring_capacity
        self.leaves[slots] = self.max_priority ** self.alpha
        self.written[slots] = True
        return np.unique(slots)

    def min_leaves(self):
        return np.where(self.written, self.leaves, np.inf)

    def trees(self):
        return O.heap_tree(self.leaves, np.add), O.heap_tree(self.min_leaves(), np.minimum)

    def draw(self, u):
        st = O.heap_tree(self.leaves, np.add)
        return O.find_prefixsum_idx_batch(st, np.asarray(u, np.float64) * st[1])

    def weights(self, idx, n_storage, beta):
        return is_weights(*self.trees(), idx, n_storage, beta)


def is_weights(st, mt, idx, n_storage, beta):
    """O.per_is_weights' formula (buffer.py:146-160) on heap arrays"""
    cap = st.size // 2
    total = st[1]
    max_w = (mt[1] / total * n_storage) ** (-beta)
    return (st[cap + np.asarray(idx, np.int64)] / total * n_storage) ** (-beta) / max_w


def descent_turns(tree, mass, first_node):
    """find_prefixsum_idx restated with a log: (indices, number of left turns, number of right turns taken at nodes >= first_node).
    The indices must equal O.find_prefixsum_idx_batch's (tests/test_per_seams.py checks that)."""
    cap = tree.size // 2
    node = np.ones(mass.size, np.int64)
    prefix = np.array(mass, np.float64)
    n_left = n_right = 0
    while node[0] < cap:
        left = tree[2 * node]
        go_left = left > prefix
        n_left += int(np.count_nonzero(go_left & (node >= first_node)))
        n_right += int(np.count_nonzero(~go_left & (node >= first_node)))
        prefix = np.where(go_left, prefix, prefix - left)
        node = np.where(go_left, 2 * node, 2 * node + 1)
    return node - cap, n_left, n_right


# ---- 3a: update sequences ------------------------------------------------------------------------------------------------------
UPDATE_CAPS = (1, 2, 64, 512, 1024, 2048, 4096, 1 << 17, 1 << 21)
BIG_CAP = 1 << 21                   # the fill and ONE rebuild batch only: the one way into k_rebuild_top's stride loop
EXTRA_BATCHES = {2: (2,), 1 << 17: (1025, 2048, 2049)}


def n_storage_of(cap):
    """filled leaves: not a power of two where capacity > 2"""
    return cap if cap <= 2 else cap - cap // 8 - 1


def batch_sizes(cap):
    if cap == BIG_CAP:
        return (cap // PATHS_RATIO + 1,)
    sizes = set((1, cap // PATHS_RATIO, cap // PATHS_RATIO + 1) + EXTRA_BATCHES.get(cap, ()))
    return tuple(sorted(n for n in sizes if n >= 1))


def takes_paths(n, cap):
    return n * PATHS_RATIO <= cap


def signed_log_uniform(rng, n, lo, hi):
    mag = 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), n)
    return (mag * rng.choice([-1.0, 1.0], n)).astype(np.float32)


HIDDEN_FIRST, HIDDEN_STEP, BODY_HI = 250.0, 250.0, 100.0        # (a sequence has at most four batches: the fourth reaches 1e3)


def hidden_max(b):
    """|td| of batch b's overridden entry: above every other entry (<= BODY_HI) and above every earlier batch's"""
    return HIDDEN_FIRST + HIDDEN_STEP * b


def make_batch(rng, b, n, n_storage):
    """Batch number b of a sequence: n signed float32 priorities between 1e-6 and 1e3 at indices below n_storage, with, as far as n
    has room for them,
      n == 1   the single entry alternates between leaf n_storage - 1 and leaf 0;
      n >= 2   entry 0 and entry n - 1 share a leaf: entry 0 holds the batch's largest |td| (hidden_max(b), above the running maximum),
               entry n - 1, which overrides it, a small one;
      n >= 5   entries 1..3 are three neighbouring leaves;
      n >= 7   entry 4 is leaf 0, entry 5 leaf n_storage - 1;
      n >= 12  a quarter of the rest repeats indices of another quarter with priorities of its own.
    Returns (idx int64 [n], td float32 [n], the position of the overridden maximum or None)."""
    idx = rng.integers(0, n_storage, n)
    td = signed_log_uniform(rng, n, 1e-6, BODY_HI)
    if n == 1:
        idx[0] = (n_storage - 1, 0)[b % 2]
        return idx, td, None
    if n >= 12:
        q = (n - 6) // 4
        idx[6:6 + q] = idx[6 + 2 * q:6 + 3 * q]
    shared = int(rng.integers(0, n_storage)) if n >= 7 else 0
    idx[0] = idx[n - 1] = shared
    td[0] = np.float32(hidden_max(b) * (-1.0 if b % 2 else 1.0))
    td[n - 1] = np.float32(3e-3)
    if n >= 5 and n_storage >= 3:
        m = int(rng.integers(0, n_storage - 2))
        idx[1:4] = (m, m + 1, m + 2)
        td[1], td[2] = np.float32(1e-6), np.float32(-BODY_HI)    # (the lower end of the span, and the body's upper end)
    if n >= 7:
        idx[4], idx[5] = 0, n_storage - 1
    return idx, td, 0


@functools.lru_cache(maxsize=None)
def update_case(cap):
    """The sequence of one capacity: dict(cap, n_storage, fill=(idx, td), batches=[(idx, td, hidden position)]).  PCG64 seed per
    capacity; the fill is arange(n_storage) with priorities of its own (<= BODY_HI).  Computed once and shared: leave it unchanged."""
    rng = np.random.Generator(np.random.PCG64(1000 + int(np.log2(cap))))
    ns = n_storage_of(cap)
    fill = (np.arange(ns, dtype=np.int64), signed_log_uniform(rng, ns, 1e-6, BODY_HI))
    return dict(cap=cap, n_storage=ns, fill=fill, batches=[make_batch(rng, b, n, ns) for b, n in enumerate(batch_sizes(cap))])


def add_case(cap):
    """The same sequence of sizes through mpg_per_add: ring_capacity = n_storage (not a power of two where capacity > 2), every batch
    starting n // 2 slots before the ring's end so that its slots wrap (n >= 2), each at a max priority of its own.
    Returns dict(cap, ring, calls=[(start, n, max priority)]); the first call is the fill from slot 0."""
    ring = n_storage_of(cap)
    calls = [(0, ring, 1.0)]
    for b, n in enumerate(batch_sizes(cap)):
        calls.append(((ring - max(n // 2, 1)) % ring, n, 1.0 + 0.37 * (b + 1)))
    return dict(cap=cap, ring=ring, calls=calls)


# ---- 3b: sampling --------------------------------------------------------------------------------------------------------------
SAMPLE_CAPS = (1, 2, 512, 1024, 2048, 1 << 17)
SAMPLE_NS = (1, 255, 257, 1000)
SAMPLE_KEYS = ((0x1234567800000011, 0x0000000300000007), (0xfeedbeef00c0ffee, 0x8000000100000000))      # (seed, ctr): high words set
SAMPLE_BETAS = (0.0, 0.4, 1.0)


def tie_js(cap):
    """the j of the tie family (u_j = j / capacity on all-ones leaves: mass == j exactly, a prefix sum of the tree)"""
    if cap <= TOPN:
        return np.arange(cap, dtype=np.int64)
    edges = np.arange(0, cap + 1, 1024, dtype=np.int64)
    js = np.concatenate([edges - 1, edges, edges + 1, np.arange(0, cap, 997, dtype=np.int64)])
    return np.unique(js[(js >= 0) & (js < cap)])


def sample_storages(cap):
    return tuple(sorted(set((1, cap // 2 + 1, cap)) & set(range(1, cap + 1))))


def sample_priorities(cap, n_storage):
    """float32 priorities of the first n_storage leaves: three decades at random, then leaf 0 and leaf n_storage - 1 raised to about
    2 % of the total mass each, so that the library's own few thousand draws reach both ends of the storage"""
    rng = np.random.Generator(np.random.PCG64(2000 + 64 * int(np.log2(cap)) + int(np.log2(n_storage))))
    td = signed_log_uniform(rng, n_storage, 1e-3, 10.0)
    if n_storage > 2:
        body = float(np.sum((np.abs(td.astype(np.float64)) + EPS) ** ALPHA))
        td[0] = np.float32((0.02 * body) ** (1.0 / ALPHA))
        td[-1] = np.float32(-(0.02 * body) ** (1.0 / ALPHA))
    return td


def library_draws():
    """every (n, seed, ctr) the device test draws with the library's own uniforms"""
    return [(n, seed, ctr) for n in SAMPLE_NS for seed, ctr in SAMPLE_KEYS]


# ---- 3c / 3d: ring -------------------------------------------------------------------------------------------------------------
WIDTHS = ((4, 1), (8, 2), (9, 2), (11, 1), (16, 2))             # gather_row switches its register width at obs_dim 8 -> 9
UNIFORM_STORAGES = (1, 2, 3, 1000, 2 ** 31 - 1)
UNIFORM_NS = (1, 3, 4, 5, 257)                                   # one Philox block serves four rows
UNIFORM_KEYS = ((0x0badcafe00000005, 0x0000000200000009), (0x7fffffff12345678, 0xffffffff00000001))


def ring_rows(rng, n, od, ad):
    """n transitions: (obs, act, rew, obs2 float32, done uint8 with both values)"""
    return (rng.standard_normal((n, od)).astype(np.float32), rng.uniform(-1, 1, (n, ad)).astype(np.float32),
            rng.standard_normal(n).astype(np.float32), rng.standard_normal((n, od)).astype(np.float32),
            rng.integers(0, 2, n).astype(np.uint8))


class HostRing(object):
    """ReplayBuffer's ring (buffer.py:21-68) as numpy arrays: add at (next_idx + i) % capacity, gather by row"""

    def __init__(self, capacity, od, ad):
        self.cap = capacity
        self.obs, self.act = np.zeros((capacity, od), np.float32), np.zeros((capacity, ad), np.float32)
        self.rew, self.obs2, self.done = np.zeros(capacity, np.float32), np.zeros((capacity, od), np.float32), np.zeros(capacity, np.uint8)

    def add(self, next_idx, obs, act, rew, obs2, done):
        d = (next_idx + np.arange(len(rew))) % self.cap
        self.obs[d], self.act[d], self.rew[d], self.obs2[d] = obs, act, rew, obs2
        self.done[d] = 1 if done is None else done             # (mpg_replay_add without dones: every transition ends its episode)

    def arrays(self):
        return self.obs, self.act, self.rew, self.obs2, self.done

    def gather(self, idx):
        return self.obs[idx], self.act[idx], self.rew[idx], self.obs2[idx], self.done[idx].astype(np.float32)
