"""BertSelfAttention's softmax(Q K^T / sqrt(d) + mask) -> dropout -> . V for short captions as ONE HIP kernel per direction
(include/glr.h: glr_attn_fwd / glr_attn_bwd; reference: transformers' BertSelfAttention inside the BertModel of
/root/reference/gloria/models/text_model.py:18-20).

`self_attention(q, k, v, key_mask, n_heads, p, training)` takes the [B, L, H] outputs of the query / key / value Linears
as they are and returns the context in the same layout.  The kernels cover what the training step runs: GPU, bf16
(autocast), head size 64, L <= 128 tokens; every other case is torch's scaled_dot_product_attention on the same
tensors.  Dropout bits: a counter-based hash of the score's position (two rounds of a 32-bit multiply-xorshift mixer,
16 bits per score: csrc/glr_attn.hip) KEYED by the CUDA generator's (seed, offset) drawn the same way the sub-layer
epilogues draw their Philox keys (fused_ln._philox_args) - reproducible under torch.manual_seed, not the same stream as
torch's own dropout.  The epilogues use Philox4x32-10 itself; here it cost 40 quarter-rate integer multiplies per 8
scores in a kernel that is VALU-bound, so the per-score draw is the cheaper mixer and only the KEY comes from Philox's
counter.  `GLR_FUSED_ATTN=0` switches the kernels off.

Captions of 129 to 512 tokens run the block-streaming kernels of csrc/glr_attn_long.hip (glr_attn_long_fwd / _bwd) through
the same autograd function (`_SelfAttn`, whatever the layout: `_layout` gives the pointers, `_route` the kernel pair): lse
and the keep bits are sized by Lp = L rounded up to 128 ([B * nh, Lp] and [B * nh, Lp, Lp / 32]: 32 KB of keep bits per
sentence x head at 512 tokens, held until the backward), and the dropout counter is the one documented in include/glr.h.  `GLR_FUSED_ATTN_LONG` (0 / 1, default 1: DESIGN.md has the measurement
behind it - faster than torch on ragged batches, slower when every key of the padded length is live) switches only that
range; with it off those lengths run torch's scaled_dot_product_attention as every other unsupported case does."""

import math
import os

import torch
import torch.nn.functional as F

from .. import _native as N
from .rng import philox_args
from .text_rows import PackedRows

ENABLED = os.environ.get("GLR_FUSED_ATTN", "1") != "0"
LONG_ENABLED = os.environ.get("GLR_FUSED_ATTN_LONG", "1") != "0"
_MAX_L = None
_MAX_L_LONG = None


def _max_tokens():
    global _MAX_L
    if _MAX_L is None:
        _MAX_L = int(N.lib().glr_attn_max_tokens(1))
    return _MAX_L


def _long_max_tokens():
    global _MAX_L_LONG
    if _MAX_L_LONG is None:
        _MAX_L_LONG = int(N.lib().glr_attn_long_max_tokens())
    return _MAX_L_LONG


def _length_ok(L):
    """the short kernels up to 128 tokens, the block-streaming ones behind their own switch up to 512"""
    return L <= _max_tokens() or (LONG_ENABLED and L <= _long_max_tokens())


def _entry(L):
    """(forward, backward, name, rows of lse / keep) of the kernel pair that runs L tokens"""
    L_ = N.lib()
    if L <= _max_tokens():
        return L_.glr_attn_fwd, L_.glr_attn_bwd, "glr_attn", 128
    return L_.glr_attn_long_fwd, L_.glr_attn_long_bwd, "glr_attn_long", (L + 127) // 128 * 128


def heads_ok(hidden, nh):
    """the head geometry the kernels take: heads of 64 features"""
    return hidden == nh * 64


def _layout(tensors):
    """(query, key, value base addresses, their row stride, H, shape of o) of split q, k, v [.., H] or of ONE packed
    [.., 3H] tensor (query | key | value columns, bf16: the blocks start 2H and 4H bytes in)"""
    if len(tensors) == 3:
        q, k, v = tensors
        return q.data_ptr(), k.data_ptr(), v.data_ptr(), q.shape[-1], q.shape[-1], q.shape
    (qkv,) = tensors
    base, H = qkv.data_ptr(), qkv.shape[-1] // 3
    return base, base + 2 * H, base + 4 * H, 3 * H, H, qkv.shape[:-1] + (H,)


def _route(keys, nh, o_shape):
    """(forward, backward, name, rows of lse / keep, arguments that locate the sentences, dimension arguments) of the
    kernel pair for a key mask (bool [B, L] or None) over o_shape = [B, L, H], or for a PackedRows over [T, H]: the short
    kernels with every key live, lse / keep in the shapes the padded call of the same sentences has"""
    if isinstance(keys, PackedRows):
        L_ = N.lib()
        return (L_.glr_attn_rows_fwd, L_.glr_attn_rows_bwd, "glr_attn_rows", _entry(keys.longest)[3],
                (N.ptr(keys.row_start), keys.row_start_host.ctypes.data), (keys.B, nh))
    return _entry(o_shape[1]) + ((N.ptr(keys),), (o_shape[0], nh, o_shape[1]))


class _SelfAttn(torch.autograd.Function):
    """tensors: q, k, v [B, L, H], or ONE [B, L, 3H] tensor (the output of a single fused Linear; the backward writes
    dq | dk | dv straight into its gradient, row stride 3H on both sides), or with keys a PackedRows ONE [T, 3H] tensor of
    real token rows only (models/text_rows.py): sentence b owns rows row_start[b] .. row_start[b + 1].  The dropout counter
    keeps its padded form there, so a sentence draws the bits the padded kernel draws for it."""

    @staticmethod
    def forward(ctx, keys, nh, p, scale, *tensors):
        qp, kp, vp, ld, H, o_shape = _layout(tensors)
        fwd, _, name, Lp, where, dims = _route(keys, nh, o_shape)
        dev = tensors[0].device
        o = torch.empty(o_shape, dtype=tensors[0].dtype, device=dev)
        lse = torch.empty(dims[0] * nh, Lp, dtype=torch.float32, device=dev)
        keep = torch.empty(dims[0] * nh, Lp, Lp // 32, dtype=torch.int32, device=dev) if p > 0 else None
        seed, off, cell = philox_args(dev) if p > 0 else (0, 0, None)
        N.check(fwd(qp, kp, vp, *where, *dims, ld, H, float(scale), float(p), seed, off, cell, N.ptr(o), N.ptr(lse),
                    N.ptr(keep), N.stream()), name + "_fwd")
        rows = keys if isinstance(keys, PackedRows) else None
        ctx.save_for_backward(*tensors, o, lse, keep, None if rows is not None else keys)
        ctx.meta = (rows, nh, float(p), float(scale))
        return o

    @staticmethod
    def backward(ctx, d_o):
        *tensors, o, lse, keep, key_mask = ctx.saved_tensors
        rows, nh, p, scale = ctx.meta
        qp, kp, vp, ld, H, o_shape = _layout(tensors)
        _, bwd, name, _, where, dims = _route(key_mask if rows is None else rows, nh, o_shape)
        d_o = d_o.to(torch.bfloat16).contiguous()
        grads = tuple(torch.empty_like(t) for t in tensors)
        N.check(bwd(qp, kp, vp, N.ptr(o), N.ptr(d_o), *where, N.ptr(lse), N.ptr(keep), *dims, ld, H, scale, p,
                    *_layout(grads)[:3], N.stream()), name + "_bwd")
        return (None, None, None, None) + grads


def self_attention_rows(qkv, rows, nh, p, training):
    """qkv: bf16 [T, 3H] (query | key | value columns) of the packed rows of `rows` -> context [T, H]"""
    if qkv.dtype != torch.bfloat16 or qkv.shape[0] != rows.T or qkv.shape[1] % 3 or not heads_ok(qkv.shape[1] // 3, nh):
        raise RuntimeError("self_attention_rows: a bf16 [T, 3 * n_heads * 64] tensor of the plan's rows is required")
    return _SelfAttn.apply(rows, nh, p if training else 0.0, 1.0 / 8.0, qkv.contiguous())


def _mask_ok(key_mask):
    return key_mask is None or (key_mask.dtype == torch.bool and key_mask.is_contiguous())


def _fusable(q, k, v, key_mask, nh):
    B, L, H = q.shape
    return (ENABLED and q.is_cuda and q.dtype == k.dtype == v.dtype == torch.bfloat16 and heads_ok(H, nh) and _length_ok(L)
            and q.is_contiguous() and k.is_contiguous() and v.is_contiguous()
            and _mask_ok(key_mask) and (key_mask is None or tuple(key_mask.shape) == (B, L)))


def packed_fusable(x, nh, hidden, L, key_mask):
    """whether BertSelfAttention may run ONE query|key|value Linear and the packed kernels on input x"""
    return (ENABLED and x.is_cuda and torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16
            and heads_ok(hidden, nh) and _length_ok(L) and _mask_ok(key_mask))


def self_attention_packed(qkv, key_mask, nh, p, training):
    """qkv: bf16 [B, L, 3H] (query | key | value columns) -> context [B, L, H]"""
    if not _length_ok(qkv.shape[1]):                        # a length no enabled kernel takes: the three column blocks
        q, k, v = (t.contiguous() for t in qkv.split(qkv.shape[2] // 3, dim=-1))
        return self_attention(q, k, v, key_mask, nh, p, training)
    return _SelfAttn.apply(key_mask, nh, p if training else 0.0, 1.0 / 8.0, qkv.contiguous())


def self_attention(q, k, v, key_mask, nh, p, training):
    """q, k, v: [B, L, H]; key_mask: bool [B, L] (True = attend) or None -> context [B, L, H]."""
    B, L, H = q.shape
    hd = H // nh
    if _fusable(q, k, v, key_mask, nh):
        return _SelfAttn.apply(key_mask, nh, p if training else 0.0, 1.0 / math.sqrt(hd), q, k, v)
    bias = None if key_mask is None else key_mask[:, None, None, :]
    qh, kh, vh = (t.view(B, L, nh, hd).transpose(1, 2) for t in (q, k, v))
    o = F.scaled_dot_product_attention(qh, kh, vh, attn_mask=bias, dropout_p=p if training else 0.0)
    return o.transpose(1, 2).reshape(B, L, H)
