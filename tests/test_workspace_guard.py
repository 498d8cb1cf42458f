"""tests/workspace_guard.py without a GPU: the guard helper on CPU tensors, the table of cases against the workspace queries (host code,
as in tests/test_badargs.py) on both engines, and the chunk arithmetic the table's row counts rest on."""
import ctypes

import pytest
import torch

from mpg_amd import _lib as L
from mpg_amd import ops
from tests import workspace_guard as G


@pytest.fixture(params=['split', 'f32'])
def engine(request):
    with L.engine(request.param):
        yield request.param


# ---- the helper ---------------------------------------------------------------------------------------------------------------------
def test_all_ones_word_is_nan():
    assert G.all_ones_word_is_nan()
    assert torch.tensor([-1], dtype=torch.int32).view(torch.float32).isnan().item()      # 0xFFFFFFFF


@pytest.mark.parametrize('fill', [G.NAN_FILL, G.ZERO_FILL])
def test_the_view_is_exactly_the_request_between_two_guards(monkeypatch, fill):
    stock = ops.workspace
    with G.guarded(monkeypatch, fill, device='cpu') as rec:
        assert ops.workspace is not stock
        v = ops.workspace('cuda', 1000, 1)              # (device: the helper's own, whatever the caller names)
        assert v.dtype == torch.uint8 and v.is_contiguous() and v.numel() == 1000 and not v.is_cuda
        (h,) = rec.handouts
        assert (h.offset, h.nb, h.slot) == (G.GUARD, 1000, 1) and h.buffer.numel() == 2 * G.GUARD + 1000
        assert v.data_ptr() == h.buffer.data_ptr() + G.GUARD
        assert bool((h.buffer == fill).all())
        assert ops.workspace('cuda', 1000, 1) is v and len(rec.handouts) == 1          # the same key: the same view
        assert ops.workspace('cuda', 1000, 0) is not v and ops.workspace('cuda', 1001, 1) is not v and len(rec.handouts) == 3
    assert ops.workspace is stock


def test_misalign_moves_the_pointer_by_that_many_bytes(monkeypatch):
    with G.guarded(monkeypatch, G.NAN_FILL, misalign=4, device='cpu') as rec:
        v = ops.workspace('cpu', 512)
        (h,) = rec.handouts
        assert v.numel() == 512 and h.offset == G.GUARD + 4 and v.data_ptr() == h.buffer.data_ptr() + G.GUARD + 4
        assert h.buffer.numel() == 2 * G.GUARD + 4 + 512


def _touched(monkeypatch, fill, misalign=0):
    """a record whose one workspace was written from its first byte to its last, as a call would leave it"""
    cm = G.guarded(monkeypatch, fill, misalign=misalign, device='cpu')
    rec = cm.__enter__()
    v = ops.workspace('cpu', 768)
    v[0], v[-1] = 7, 9
    cm.__exit__(None, None, None)
    return rec


@pytest.mark.parametrize('fill', [G.NAN_FILL, G.ZERO_FILL])
@pytest.mark.parametrize('misalign', [0, 4])
def test_check_passes_on_untouched_guards_and_a_touched_interior(monkeypatch, fill, misalign):
    G.check(_touched(monkeypatch, fill, misalign))


@pytest.mark.parametrize('fill', [G.NAN_FILL, G.ZERO_FILL])
@pytest.mark.parametrize('where', ['first byte', 'byte in front of the view', 'byte behind the view', 'last byte'])
def test_check_fails_on_one_changed_guard_byte(monkeypatch, fill, where):
    rec = _touched(monkeypatch, fill, misalign=4)
    (h,) = rec.handouts
    i = {'first byte': 0, 'byte in front of the view': h.offset - 1, 'byte behind the view': h.offset + h.nb, 'last byte': h.buffer.numel() - 1}[where]
    h.buffer[i] = 0x5A
    with pytest.raises(AssertionError, match='in front of' if i < h.offset else 'behind'):
        G.check(rec)


def test_check_fails_on_an_untouched_interior_and_without_a_hand_out(monkeypatch):
    with G.guarded(monkeypatch, G.NAN_FILL, device='cpu') as rec:
        with pytest.raises(AssertionError, match='no workspace was asked for'):
            G.check(rec)
        ops.workspace('cpu', 768)
    with pytest.raises(AssertionError, match='did not use it'):
        G.check(rec)


def test_check_of_a_call_that_leaves_its_workspace_alone_and_the_count_of_unwritten_words(monkeypatch):
    with G.guarded(monkeypatch, G.NAN_FILL, misalign=4, device='cpu') as rec:
        v = ops.workspace('cpu', 768, 1)
    G.check(rec, used=False)
    assert G.unwritten_words(rec) == [(1, 192, 192)]
    v[8:16] = 0
    assert G.unwritten_words(rec) == [(1, 192, 190)]
    with pytest.raises(AssertionError, match='wrote to it'):
        G.check(rec, used=False)


def test_backward_takes_thin_is_read_from_the_source():
    got = {(i, o): G.backward_takes_thin(i, o) for i in (4, 6, 7, 8, 9) for o in (1, 2, 4)}
    assert got[(4, 2)] and got[(6, 2)] and got[(8, 1)] and not got[(9, 1)] and not got[(6, 4)], got


# ---- the table against the queries ---------------------------------------------------------------------------------------------------
def _need(case, rows):
    cfg = case.cfg()
    return getattr(L.lib(), case.query)(ctypes.byref(cfg), *[ctypes.c_int(int(v)) for v in case.sizes(rows)])


@pytest.mark.parametrize('case', G.CASES, ids=[c.name for c in G.CASES])
def test_every_case_names_a_query_that_serves_it(engine, case):
    """more than 0 bytes for the case's configuration and row count, not fewer at the next row count the entry point accepts; and the
    Arena's promise for an unaligned buffer from the query alone: every array is charged its bytes rounded up to 256 plus 256, so an
    answer is a multiple of 256 and at least 512 (the second of the two forms: the arrays are not counted from here)"""
    need, more = _need(case, case.rows), _need(case, case.rows + case.step)
    assert need > 0, (case.name, case.query)
    assert more >= need, (case.name, need, more)
    assert need % 256 == 0 and need >= 512, (case.name, need)


def test_the_table_holds_every_group_of_entry_points():
    names = ' '.join(c.name for c in G.CASES)
    for piece in ('q_targets-', 'td3_targets-', 'nstep_targets-', 'nstep_targets_clipped-', 'rollout_q_target-', 'rollout_q_estimation-', 'q_loss_grad-pt-K10',
                  'td3_policy_grad-', 'dpg_policy_grad-', 'sac_policy_grad-', 'sac_policy_grad_squashed-pd', 'sac_policy_grad_auto-',
                  'sac_policy_grad_squashed_auto-', 'sac_targets-', 'sac_targets_squashed-', 'sac_targets_auto-', 'sac_targets_squashed_auto-',
                  'policy_sample-', 'policy_sample_squashed-pd', 'rollout_pg-step0-', 'rollout_pg-all-pt-K0-M1-cached', 'rollout_pg-all-pt-K3',
                  'rollout_pg-all-dp', 'ampc_pg-pt-K0-M1-cached', 'ampc_pg-pd', 'n25', 'mpg_gradients-fused-pt-K0-M1-nq1', 'mpg_gradients-fused-pt-K0-M1-nq2',
                  'mpg_gradients-fallback-pt-K0-M2', 'mpg_gradients-fallback-pt-K3'):
        assert piece in names, piece
    rows = {c.rows for c in G.CASES}
    assert {1, 17, 272, 1037, 2051} <= rows, rows
    assert {'policy_sample-pt-K0-rows1', 'policy_sample_want_logits-pt-K0-rows1', 'td3_targets-pt-K0-rows1', 'q_targets_one_critic-pt-K0-rows1'} <= \
        {c.name for c in G.CASES}
    assert [c.name.split('-')[0] for c in G.CASES if not c.used] and {c.name.split('-')[0].replace('_squashed', '') for c in G.CASES if not c.used} == \
        {'policy_sample_want_logits'}


def test_2051_rows_go_exactly_where_the_weight_gradient_can_be_the_dw2_only_form():
    """the (input width, used outputs) of every case's weight-gradient launch against backward_takes_thin as csrc/mlp_kernels.hip states
    it (read from the source): the cases with 2051 rows are those it accepts, no more and no fewer"""
    widths = {'q_loss_grad-pt-K0': (8, 1), 'q_loss_grad-pt-K3': (11, 1), 'q_loss_grad-pt-K10': (18, 1)}
    for K in (0, 3):
        for name, ou in (('td3_policy_grad', 2), ('dpg_policy_grad', 2), ('sac_policy_grad', 4), ('sac_policy_grad_squashed', 4),
                         ('sac_policy_grad_auto', 4), ('sac_policy_grad_squashed_auto', 4)):
            widths['%s-pt-K%d' % (name, K)] = (6 + K, ou)
    widths.update({'sac_policy_grad_squashed-pd': (4, 2), 'sac_policy_grad_squashed_auto-pd': (4, 2)})
    stems = {c.name.rsplit('-rows', 1)[0] for c in G.CASES}
    assert set(widths) <= stems, set(widths) - stems
    assert {s for s in stems if s.split('-')[0].endswith(('_policy_grad', 'q_loss_grad')) or 'sac_policy_grad' in s} == set(widths)
    with_2051 = {c.name.rsplit('-rows', 1)[0] for c in G.CASES if c.rows == 2051}
    assert with_2051 == {s for s, (ind, ou) in widths.items() if G.backward_takes_thin(ind, ou)}, with_2051
    assert with_2051 and with_2051 != set(widths)


# ---- the chunk arithmetic --------------------------------------------------------------------------------------------------------------
def test_the_larger_row_counts_leave_a_short_last_chunk():
    """csrc/mlp_wgrad.h wgrad_groups_per_chunk / wgrad_groups_per_chunk_w2 under the MPG_WGRAD_* constants in force: every row count the
    table gives for a ragged last chunk has one - more than one chunk, the last one shorter than the others - and exactly the one the
    table states.  A change of those constants fails here instead of leaving the row counts stale."""
    consts = G.wgrad_constants()
    assert (G.wgrad_chunks(1, 'single', consts), G.wgrad_chunks(17, 'single', consts)) == ((1, 1, 1), (1, 2, 1))
    for rows, form, want in G.RAGGED_CHUNKS:
        gp, nch, last = got = G.wgrad_chunks(rows, form, consts)
        assert nch > 1 and 0 < last < gp, (rows, form, got)
        assert got == want, (rows, form, got, want)
    assert G.wgrad_chunks(16 * 4096, 'w2', consts)[0] == consts['MPG_WGRAD_W2_MIN_GROUPS']      # (the large-job floor of the w2 form)
