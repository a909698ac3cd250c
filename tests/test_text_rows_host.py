"""CPU checks of the row plan of the text encoder's real-token route (gloria/models/text_rows.py: plan_rows): contents of
row_start / row_ids on ragged prefixes, and "not eligible" (None) for every mask the packed kernels must not see."""

import numpy as np

from gloria.models.text_rows import plan_rows


def _mask(lengths, L):
    return (np.arange(L)[None, :] < np.asarray(lengths)[:, None]).astype(np.int64)


def _dst(lengths, L):
    """every live token its own word slot, nothing behind the prefix"""
    t = np.arange(L)[None, :]
    return np.where(t < np.asarray(lengths)[:, None], t, -1)


def test_ragged_prefixes_give_prefix_sums_and_original_rows():
    lengths, L = [3, 7, 1, 40, 16], 40
    plan = plan_rows(_mask(lengths, L), _dst(lengths, L), 128)
    assert plan is not None
    row_start, row_ids = plan
    assert row_start.dtype == np.int32 and row_ids.dtype == np.int32
    assert row_start.tolist() == [0, 3, 10, 11, 51, 67]
    want = [b * L + t for b, n in enumerate(lengths) for t in range(n)]
    assert row_ids.tolist() == want and len(want) == sum(lengths)        # T exact: no rounding up, no dead tail rows
    # a mask of other nonzero values and a bool mask are the same plan
    for m in (_mask(lengths, L) * 7, _mask(lengths, L).astype(bool)):
        p2 = plan_rows(m, _dst(lengths, L), 128)
        assert p2[0].tolist() == row_start.tolist() and p2[1].tolist() == want


def test_dropped_tokens_inside_the_prefix_stay_live_rows():
    lengths, L = [5, 9], 12
    dst = _dst(lengths, L)
    dst[0, 3:5] = -1                       # tokens behind [SEP] / an unflushed last word: still keys of their sentence
    plan = plan_rows(_mask(lengths, L), dst, 128)
    assert plan is not None and plan[0].tolist() == [0, 5, 14]


def test_hole_in_a_mask_is_not_eligible():
    lengths, L = [6, 9, 4], 12
    m = _mask(lengths, L)
    m[1, 2] = 0
    assert plan_rows(m, _dst(lengths, L), 128) is None
    m = _mask(lengths, L)
    m[2, 8] = 1                            # a live token behind a gap
    assert plan_rows(m, _dst(lengths, L), 128) is None


def test_empty_mask_row_is_not_eligible():
    lengths, L = [6, 0, 4], 12
    assert plan_rows(_mask(lengths, L), _dst(lengths, L), 128) is None


def test_live_word_piece_behind_the_prefix_is_not_eligible():
    lengths, L = [6, 9, 4], 12
    dst = _dst(lengths, L)
    dst[2, 4] = 4                          # aggregation would read a row the packed tensor does not hold
    assert plan_rows(_mask(lengths, L), dst, 128) is None


def test_more_tokens_than_the_short_kernels_take_is_not_eligible():
    L = 129
    for lengths in ([129, 5, 17], [128, 5, 17], [12, 5, 17]):
        assert plan_rows(_mask(lengths, L), _dst(lengths, L), 128) is None
    assert plan_rows(_mask([128, 5, 17], 128), _dst([128, 5, 17], 128), 128) is not None
    assert plan_rows(_mask([97, 5, 17], 128), _dst([97, 5, 17], 128), 96) is None      # the limit is the caller's


def test_all_full_batch_is_not_packed():
    lengths, L = [12, 12, 12], 12
    assert plan_rows(_mask(lengths, L), _dst(lengths, L), 128) is None


def test_shape_mismatch_is_not_eligible():
    assert plan_rows(_mask([3, 4], 8), _dst([3, 4], 9), 128) is None
    assert plan_rows(np.ones(8), np.zeros(8), 128) is None


def test_benchmark_batch_counts():
    """the flagship batch: 256 captions padded to 97 tokens hold 7 488 real token rows"""
    from gloria.datasets.synthetic import make_batch
    from gloria.models.text_model import Vocab, wordpiece_slots
    batch = make_batch(256, seed=1234, lengths="words")
    ids, mask = batch["caption_ids"].numpy(), batch["attention_mask"].numpy()
    dst = wordpiece_slots(ids, Vocab.synthetic())[0]
    plan = plan_rows(mask, dst, 128)
    assert plan is not None
    row_start, row_ids = plan
    n = np.diff(row_start)
    assert row_start[-1] == row_ids.shape[0] == 7488 and n.max() == 54 and n.min() == 6
    assert (mask.reshape(-1)[row_ids] != 0).all() and (np.diff(row_ids) > 0).all()
