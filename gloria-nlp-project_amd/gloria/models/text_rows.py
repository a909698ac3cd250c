"""Row plan of the text encoder's real-token route: the BERT layers run on the T live token rows of a batch instead of
its B * L padded ones (include/glr.h: glr_attn_rows_fwd / _bwd, glr_drop_add_ln_rows_fwd, glr_wordpiece_segsum_rows_fwd /
_bwd; DESIGN.md "Text encoder on real token rows").

A pad row is never a live key, word-piece aggregation never reads it (dst = -1) and its gradient is exactly zero in every
layer, so nothing the step returns depends on it.  The plan is two small int32 arrays built on the host from the host
copies of the mask and the word-slot table (no device sync), uploaded once per step:

  row_start [B + 1]   prefix sum of the live token counts n_b      row_ids [T]   original row b * L + t of packed row r

`plan_rows` is pure numpy: it returns None whenever a precondition fails and the caller then runs the padded path.
`GLR_TEXT_PACKED=0` switches the route off."""

import os

import numpy as np
import torch

from .. import _native as N


def _switch():
    return os.environ.get("GLR_TEXT_PACKED", "1") != "0"


ENABLED = _switch()


def plan_rows(mask, dst, max_tokens):
    """mask [B, L] (nonzero = live token), dst [B, L] (word slot of a token, -1 = dropped), max_tokens = longest sentence
    the row kernels take -> (row_start int32 [B + 1], row_ids int32 [T]) or None (not eligible).

    Eligible: L <= max_tokens, every mask row is a non-empty prefix of ones, the prefix covers every token with
    dst >= 0, and packing removes at least one row (T < B * L)."""
    mask = np.asarray(mask)
    dst = np.asarray(dst)
    if mask.ndim != 2 or mask.shape != dst.shape or mask.size == 0:
        return None
    B, L = mask.shape
    if L > max_tokens:
        return None
    live = mask != 0
    n = live.sum(1)
    t = np.arange(L)[None, :]
    prefix = t < n[:, None]
    if (n < 1).any() or not np.array_equal(live, prefix):
        return None
    if ((dst >= 0) & ~prefix).any():
        return None
    T = int(n.sum())
    if T >= B * L:
        return None
    row_start = np.zeros(B + 1, dtype=np.int32)
    np.cumsum(n, out=row_start[1:])
    row_ids = np.nonzero(prefix.reshape(-1))[0].astype(np.int32)
    return row_start, row_ids


class PackedRows:
    """the plan on the device; handed to the BERT layers in place of the key mask"""

    def __init__(self, row_start, row_ids, B, L, device):
        self.B, self.L, self.T = int(B), int(L), int(row_ids.shape[0])
        self.row_start_host = np.ascontiguousarray(row_start, dtype=np.int32)     # read by the attention entry points
        self.longest = int(np.diff(self.row_start_host).max())
        both = N.upload(np.concatenate([self.row_start_host, np.ascontiguousarray(row_ids, dtype=np.int32)]), device)
        self.row_start = both[:B + 1]
        self.row_ids = both[B + 1:]
        self.row_ids64 = self.row_ids.to(torch.int64)                           # index_select wants int64
