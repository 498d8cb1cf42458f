"""The cache policy of every G16 stash access, read from the ISA of the translation units as the shipped flags compile them
(no GPU needed; same mechanism as the ISA checks of tests/test_abi.py).  A stash access is 16 bytes per lane, two per call on
ONE address pair 1024 bytes apart (mlp_core.h: stash_store / stash_load); the policy a call site chose is a word on the
instruction: `sc1` on a write-through store, `nt` on a non-temporal load.  POLICY below is the shipped choice per kernel
(EXPERIMENTS.md, "Cache policy of the stashes"): a later edit of stash_store / stash_load or of a call site cannot drop or
spread a policy without this file changing too."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# translation units that hold stash accesses
UNITS = ['rollout_fwd.hip', 'rollout_fwd_pendulum.hip', 'rollout_fwd_double_pendulum.hip', 'rollout_bwd.hip',
         'rollout_bwd_pendulum.hip', 'rollout_bwd_double_pendulum.hip', 'fused_kernels.hip', 'mlp_kernels.hip']
# kernel (demangled, as tools/stash_policy_census.py prints it) -> the accesses with a cache-policy word it must hold, as
# {(kind, width, words): count}.  Every kernel that is not listed holds no access with a cache-policy word at all.
FWD = 'rollout::k_rollout_fwd<rollout::PathTracking, true, false>'
BWD = 'rollout::k_rollout_bwd<rollout::PathTracking, true, false, false>'
POLICY = {
    FWD: {('store', 'dwordx4', ('sc1',)): 8},      # H1 and H2 of a step, two 16-byte stores each, in the two copies of the step loop
    BWD: {('load', 'dwordx4', ('nt',)): 6},        # three stash_load call sites (H2 of step n, H1 and H2 in the loop), two loads each
}
STORE_X4 = re.compile(r'^\s*global_store_dwordx4\s+(v\[\d+:\d+\]),\s*v\[\d+:\d+\],\s*off(.*)$')


@pytest.fixture(scope='module')
def census_mod():
    spec = importlib.util.spec_from_file_location('stash_policy_census', os.path.join(ROOT, 'tools', 'stash_policy_census.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def kernels(census_mod):
    """{demangled kernel: (census row, [16-byte global stores as (address registers, offset, policy words)])}"""
    out = {}
    for f in UNITS:
        asm = census_mod.asm_of(f)
        rows = census_mod.census_of(asm)
        cur = None
        for line in asm.splitlines():
            m = re.match(r'^(_Z\w+):', line)
            if m:
                cur = census_mod.demangle(m.group(1))
                out[cur] = (rows[m.group(1)], [])
                continue
            s = STORE_X4.match(line.split(';')[0])
            if s and cur:
                words = s.group(2).split()
                off = [int(w.split(':')[1]) for w in words if w.startswith('offset:')]
                out[cur][1].append((s.group(1), off[0] if off else 0, tuple(w for w in words if not w.startswith('offset:'))))
    return out


def test_policy_table_names_existing_kernels(kernels):
    assert len(kernels) > 20
    for k in POLICY:
        assert k in kernels, k


def test_write_through_stashes_are_complete(kernels):
    """In the kernel whose stash stores are write-through, both 16-byte stores of every stash pair carry sc1 and no plain pair is left"""
    stores = kernels[FWD][1]
    wt = [s for s in stores if s[2] == ('sc1',)]
    assert len(wt) == POLICY[FWD][('store', 'dwordx4', ('sc1',))]
    # the write-through form is a pair on one address: offset 0, then offset 1024
    for a, b in zip(wt[0::2], wt[1::2]):
        assert a[0] == b[0] and (a[1], b[1]) == (0, 1024), (a, b)
    # a plain stash pair would show as two neighbouring 16-byte stores through the SAME address registers, 1024 bytes apart
    for a, b in zip(stores, stores[1:]):
        if a[0] == b[0] and abs(a[1] - b[1]) == 1024:
            assert a[2] == b[2] == ('sc1',), (a, b)


def test_nontemporal_stash_loads_are_complete():
    """Every stash read of the reverse sweep goes through the kernel's policy tag (two 16-byte loads per call site: the count that
    test_no_other_kernel_carries_a_cache_policy pins), and its stash stores keep the default form"""
    src = open(os.path.join(ROOT, 'mpg_amd', 'csrc', 'rollout_bwd.hip')).read()
    assert len(re.findall(r'\bstash_load<LD>\(', src)) * 2 == POLICY[BWD][('load', 'dwordx4', ('nt',))]
    assert not re.search(r'\bstash_load\(', src)
    assert not re.search(r'\bstash_store<', src)


def test_no_other_kernel_carries_a_cache_policy(kernels):
    for k, (row, stores) in kernels.items():
        marked = {key: n for key, n in row.items() if key[2]}
        assert marked == POLICY.get(k, {}), (k, marked)


def test_plain_stash_pairs_are_recognised(kernels):
    """The pair rule above is not vacuous: the kernels that keep the plain form show such pairs"""
    plain_pairs = 0
    for k, (row, stores) in kernels.items():
        if k not in POLICY:
            plain_pairs += sum(1 for a, b in zip(stores, stores[1:]) if a[0] == b[0] and abs(a[1] - b[1]) == 1024 and not a[2] and not b[2])
    assert plain_pairs >= 8, plain_pairs
