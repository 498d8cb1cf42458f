"""tests/rollout_harness.py itself, on CPU tensors: the shared comparison of the one-launch worker samples' GPU tests cannot silently
compare less than the copies it replaced did - every one of the ten names, floats as bit patterns - and the mask of written ring
slots marks exactly the slots a launch writes."""
import pytest
import torch

from tests.rollout_harness import NAMES, assert_same, bits, touched

FLOATS = ('state', 'obs_io', 'act_out', 'ring_obs', 'ring_act', 'ring_rew', 'ring_obs2')
BYTES = ('done_out', 'ring_done')


def side():
    """one side's dict in the shapes and dtypes of the GPU tests' (6 agents, a ring of 11), a NaN among the floats"""
    g = torch.Generator().manual_seed(3)
    shapes = dict(state=(6, 6), obs_io=(6, 9), act_out=(6, 2), ring_obs=(11, 9), ring_act=(11, 2), ring_rew=(11,), ring_obs2=(11, 9))
    t = {k: torch.randn(*s, generator=g) for k, s in shapes.items()}
    t['ring_rew'][4] = float('nan')
    t['done_out'] = torch.full((6,), 0xAB, dtype=torch.uint8)
    t['ring_done'] = torch.randint(0, 2, (11,), generator=g).to(torch.uint8)
    t['status'] = torch.zeros(1, dtype=torch.int32)
    return t


def copy(t):
    return {k: v.clone() for k, v in t.items()}


def test_the_names_are_the_ten_buffers_of_a_side():
    assert len(NAMES) == len(set(NAMES)) == 10 and set(NAMES) == set(FLOATS) | set(BYTES) | {'status'}
    assert set(side()) == set(NAMES)


def test_equal_sides_pass_a_nan_of_one_bit_pattern_included():
    a = side()
    b = copy(a)
    assert torch.isnan(a['ring_rew'][4]) and not torch.equal(a['ring_rew'], b['ring_rew'])     # == would not do
    assert_same(a, b, 'equal')


def test_zero_against_minus_zero_fails():
    a = side()
    a['ring_act'][3, 1] = 0.
    b = copy(a)
    b['ring_act'][3, 1] = -0.
    assert torch.equal(a['ring_act'], b['ring_act'])                                            # == would pass
    with pytest.raises(AssertionError, match='ring_act'):
        assert_same(a, b, 'signed zero')


@pytest.mark.parametrize('key', NAMES)
def test_one_flipped_low_bit_in_any_single_name_fails_under_that_name(key):
    a = side()
    b = copy(a)
    flat = bits(b[key]).view(-1)                       # shares b[key]'s storage: the clones are contiguous
    flat[-1] ^= 1                                      # float32: the lowest mantissa bit
    with pytest.raises(AssertionError) as e:
        assert_same(a, b, 'one bit')
    assert "'one bit', '%s'" % key in str(e.value)
    others = tuple(k for k in NAMES if k != key)
    assert_same(a, b, 'the rest', names=others)


@pytest.mark.parametrize('key', BYTES)
def test_differing_uint8_arrays_fail(key):
    a = side()
    b = copy(a)
    b[key][2] = 0xAB if int(a[key][2]) != 0xAB else 1
    with pytest.raises(AssertionError, match=key):
        assert_same(a, b, 'bytes')


@pytest.mark.parametrize('key', NAMES)
def test_a_missing_name_raises(key):
    a = side()
    b = copy(a)
    del b[key]
    with pytest.raises(KeyError, match=key):
        assert_same(a, b, 'missing')
    with pytest.raises(KeyError, match=key):
        assert_same(b, a, 'missing')


# every iters * n of the four files' whole-ring cases, and of their wrapped ones
@pytest.mark.parametrize('count', sorted({n * iters for n in (1, 8, 16, 40) for iters in (1, 2, 5, 64)} | {1 * 512}))
def test_touched_marks_the_slots_behind_five_in_a_ring_of_thirteen_more(count):
    cap = count + 13
    m = touched(cap, 5, count, device='cpu')
    assert m.dtype == torch.bool and m.shape == (cap,) and int(m.sum()) == count
    assert m[5:5 + count].all() and not m[:5].any() and not m[5 + count:].any()


@pytest.mark.parametrize('count', [8 * 5, 40 * 5, 16 * 64, 1 * 64])
def test_touched_wraps_modulo_the_capacity(count):
    m = touched(count, count - 3, count, device='cpu')
    assert m.shape == (count,) and m.all()                                # cap == count from cap - 3: every slot once
    cap = count + 13
    m = touched(cap, cap - 3, count, device='cpu')                        # and with room to spare: three at the end, the rest in front
    assert int(m.sum()) == count and m[cap - 3:].all() and m[:count - 3].all() and not m[count - 3:cap - 3].any()
