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
the same two autograd functions: lse and the keep bits are sized by Lp = L rounded up to 128 ([B * nh, Lp] and
[B * nh, Lp, Lp / 32]: 32 KB of keep bits per sentence x head at 512 tokens, held until the backward), and the dropout
counter is the one documented in include/glr.h.  `GLR_FUSED_ATTN_LONG` (0 / 1, default 1: DESIGN.md has the measurement
behind it - faster than torch on ragged batches, slower when every key of the padded length is live) switches only that
range; with it off those lengths run torch's scaled_dot_product_attention as every other unsupported case does."""

import math
import os

import torch
import torch.nn.functional as F

from .. import _native as N
from .rng import philox_args

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


class _SelfAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, key_mask, nh, p, scale):
        B, L, H = q.shape
        fwd, _, name, Lp = _entry(L)
        dev = q.device
        o = torch.empty_like(q)
        lse = torch.empty(B * nh, Lp, dtype=torch.float32, device=dev)
        keep = torch.empty(B * nh, Lp, Lp // 32, dtype=torch.int32, device=dev) if p > 0 else None
        seed, off, cell = philox_args(dev) if p > 0 else (0, 0, None)
        N.check(fwd(N.ptr(q), N.ptr(k), N.ptr(v), N.ptr(key_mask), B, nh, L, H, H, float(scale), float(p), seed, off,
                    cell, N.ptr(o), N.ptr(lse), N.ptr(keep), N.stream()), name + "_fwd")
        ctx.save_for_backward(q, k, v, o, lse, keep, key_mask)
        ctx.meta = (nh, float(p), float(scale))
        return o

    @staticmethod
    def backward(ctx, d_o):
        q, k, v, o, lse, keep, key_mask = ctx.saved_tensors
        nh, p, scale = ctx.meta
        B, L, H = q.shape
        _, bwd, name, _ = _entry(L)
        d_o = d_o.to(torch.bfloat16).contiguous()
        dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
        N.check(bwd(N.ptr(q), N.ptr(k), N.ptr(v), N.ptr(o), N.ptr(d_o), N.ptr(key_mask), N.ptr(lse), N.ptr(keep),
                    B, nh, L, H, H, scale, p, N.ptr(dq), N.ptr(dk), N.ptr(dv), N.stream()), name + "_bwd")
        return dq, dk, dv, None, None, None, None


class _SelfAttnPacked(torch.autograd.Function):
    """the same kernels on ONE [B, L, 3H] tensor (query | key | value columns): the output of a single fused Linear.
    The backward writes dq | dk | dv straight into the gradient of that tensor (row stride 3H on both sides)."""

    @staticmethod
    def forward(ctx, qkv, key_mask, nh, p, scale):
        B, L, H3 = qkv.shape
        H = H3 // 3
        fwd, _, name, Lp = _entry(L)
        dev = qkv.device
        o = torch.empty(B, L, H, dtype=qkv.dtype, device=dev)
        lse = torch.empty(B * nh, Lp, dtype=torch.float32, device=dev)
        keep = torch.empty(B * nh, Lp, Lp // 32, dtype=torch.int32, device=dev) if p > 0 else None
        seed, off, cell = philox_args(dev) if p > 0 else (0, 0, None)
        base = qkv.data_ptr()
        N.check(fwd(N.c_void_p(base), N.c_void_p(base + 2 * H), N.c_void_p(base + 4 * H), N.ptr(key_mask), B, nh, L, H3, H,
                    float(scale), float(p), seed, off, cell, N.ptr(o), N.ptr(lse), N.ptr(keep), N.stream()), name + "_fwd")
        ctx.save_for_backward(qkv, o, lse, keep, key_mask)
        ctx.meta = (nh, float(p), float(scale))
        return o

    @staticmethod
    def backward(ctx, d_o):
        qkv, o, lse, keep, key_mask = ctx.saved_tensors
        nh, p, scale = ctx.meta
        B, L, H3 = qkv.shape
        H = H3 // 3
        _, bwd, name, _ = _entry(L)
        d_o = d_o.to(torch.bfloat16).contiguous()
        dqkv = torch.empty_like(qkv)
        base, dbase = qkv.data_ptr(), dqkv.data_ptr()
        N.check(bwd(N.c_void_p(base), N.c_void_p(base + 2 * H), N.c_void_p(base + 4 * H), N.ptr(o), N.ptr(d_o),
                    N.ptr(key_mask), N.ptr(lse), N.ptr(keep), B, nh, L, H3, H, scale, p, N.c_void_p(dbase),
                    N.c_void_p(dbase + 2 * H), N.c_void_p(dbase + 4 * H), N.stream()), name + "_bwd")
        return dqkv, None, None, None, None


class _SelfAttnRows(torch.autograd.Function):
    """the short kernels on a packed [T, 3H] query|key|value tensor of real token rows only (models/text_rows.py):
    sentence b owns rows row_start[b] .. row_start[b + 1], every key is live.  lse / keep keep the padded shapes and the
    dropout counter its padded form, so a sentence draws the bits the padded kernel draws for it."""

    @staticmethod
    def forward(ctx, qkv, rows, nh, p, scale):
        T, H3 = qkv.shape
        H = H3 // 3
        dev = qkv.device
        o = torch.empty(T, H, dtype=qkv.dtype, device=dev)
        lse = torch.empty(rows.B * nh, 128, dtype=torch.float32, device=dev)
        keep = torch.empty(rows.B * nh, 128, 4, dtype=torch.int32, device=dev) if p > 0 else None
        seed, off, cell = philox_args(dev) if p > 0 else (0, 0, None)
        base = qkv.data_ptr()
        N.check(N.lib().glr_attn_rows_fwd(N.c_void_p(base), N.c_void_p(base + 2 * H), N.c_void_p(base + 4 * H),
                                          N.ptr(rows.row_start), rows.row_start_host.ctypes.data, rows.B, nh, H3, H,
                                          float(scale), float(p), seed, off, cell, N.ptr(o), N.ptr(lse), N.ptr(keep),
                                          N.stream()), "glr_attn_rows_fwd")
        ctx.save_for_backward(qkv, o, lse, keep)
        ctx.rows = rows
        ctx.meta = (nh, float(p), float(scale))
        return o

    @staticmethod
    def backward(ctx, d_o):
        qkv, o, lse, keep = ctx.saved_tensors
        rows = ctx.rows
        nh, p, scale = ctx.meta
        H = qkv.shape[1] // 3
        d_o = d_o.to(torch.bfloat16).contiguous()
        dqkv = torch.empty_like(qkv)
        base, dbase = qkv.data_ptr(), dqkv.data_ptr()
        N.check(N.lib().glr_attn_rows_bwd(N.c_void_p(base), N.c_void_p(base + 2 * H), N.c_void_p(base + 4 * H), N.ptr(o),
                                          N.ptr(d_o), N.ptr(rows.row_start), rows.row_start_host.ctypes.data, N.ptr(lse),
                                          N.ptr(keep), rows.B, nh, 3 * H, H, scale, p, N.c_void_p(dbase),
                                          N.c_void_p(dbase + 2 * H), N.c_void_p(dbase + 4 * H), N.stream()),
                "glr_attn_rows_bwd")
        return dqkv, None, None, None, None


def self_attention_rows(qkv, rows, nh, p, training):
    """qkv: bf16 [T, 3H] (query | key | value columns) of the packed rows of `rows` -> context [T, H]"""
    if qkv.dtype != torch.bfloat16 or qkv.shape[0] != rows.T or qkv.shape[1] != 3 * nh * 64:
        raise RuntimeError("self_attention_rows: a bf16 [T, 3 * n_heads * 64] tensor of the plan's rows is required")
    return _SelfAttnRows.apply(qkv.contiguous(), rows, nh, p if training else 0.0, 1.0 / 8.0)


def _fusable(q, k, v, key_mask, nh):
    B, L, H = q.shape
    return (ENABLED and q.is_cuda and q.dtype == k.dtype == v.dtype == torch.bfloat16 and H == nh * 64 and _length_ok(L)
            and q.is_contiguous() and k.is_contiguous() and v.is_contiguous()
            and (key_mask is None or (key_mask.dtype == torch.bool and tuple(key_mask.shape) == (B, L) and key_mask.is_contiguous())))


def packed_fusable(x, nh, hidden, L, key_mask):
    """whether BertSelfAttention may run ONE query|key|value Linear and the packed kernels on input x"""
    return (ENABLED and x.is_cuda and torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16
            and hidden == nh * 64 and _length_ok(L)
            and (key_mask is None or (key_mask.dtype == torch.bool and key_mask.is_contiguous())))


def self_attention_packed(qkv, key_mask, nh, p, training):
    """qkv: bf16 [B, L, 3H] (query | key | value columns) -> context [B, L, H]"""
    if not _length_ok(qkv.shape[1]):                        # a length no enabled kernel takes: the three column blocks
        q, k, v = (t.contiguous() for t in qkv.split(qkv.shape[2] // 3, dim=-1))
        return self_attention(q, k, v, key_mask, nh, p, training)
    return _SelfAttnPacked.apply(qkv.contiguous(), key_mask, nh, p if training else 0.0, 1.0 / 8.0)


def self_attention(q, k, v, key_mask, nh, p, training):
    """q, k, v: [B, L, H]; key_mask: bool [B, L] (True = attend) or None -> context [B, L, H]."""
    B, L, H = q.shape
    hd = H // nh
    if _fusable(q, k, v, key_mask, nh):
        return _SelfAttn.apply(q, k, v, key_mask, nh, p if training else 0.0, 1.0 / math.sqrt(hd))
    bias = None if key_mask is None else key_mask[:, None, None, :]
    qh, kh, vh = (t.view(B, L, nh, hd).transpose(1, 2) for t in (q, k, v))
    o = F.scaled_dot_product_attention(qh, kh, vh, attn_mask=bias, dropout_p=p if training else 0.0)
    return o.transpose(1, 2).reshape(B, L, H)
