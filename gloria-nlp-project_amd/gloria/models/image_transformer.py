"""The transformer over the local image regions (reference: `image_transformer` of gloria/models/gloria_model.py:52-59, run at
:93-101 on the 19 x 19 regions flattened to [S, B, E]) on the HIP path of the text encoder.

`GLoRIA.image_transformer` stays a stock `nn.TransformerEncoder`: it is the parameter container (`layers.{i}.self_attn.
in_proj_weight`, `out_proj`, `linear1/2`, `norm1/2` keep names, shapes and init, so reference checkpoints load unchanged).
`run(encoder, img_emb_l, pos)` walks `encoder.layers` and computes torch's default layer - post-LN, ReLU, eps 1e-5, no final
norm - from the building blocks of models/bert.py, on [B, S, E] token rows (the free view of the channels-last local
embeddings: no permute copies):
    qkv = linear(x16, in_proj_weight, in_proj_bias)           one packed query|key|value GEMM, 64-wide heads, scale 1/8
    ctx = attention(qkv)                                      fused_attn's packed kernels, or torch's SDPA on head views
    y   = LayerNorm(dropout(out_proj(ctx)) + x)               fused_ln.dense_drop_add_ln (glr_drop_add_ln_fwd / _bwd)
    a   = dropout(relu(linear1(y)))                           `relu_drop`: glr_relu_drop_fwd / _bwd (csrc/glr_ffn.hip), one
                                                              pass per direction, 1 bit per element saved instead of z, and
                                                              linear1's bias gradient summed on the way
    x'  = LayerNorm(dropout(linear2(a)) + y)                  dense_drop_add_ln
The residual stream is fp32, GEMM operands bf16.  Dropout draws the kernels' Philox / hash streams keyed by the CUDA
generator (models/rng.py): reproducible under torch.manual_seed, not torch's own masks.

`fusable(encoder, x)` names what takes this path (GPU, bf16 autocast, E = heads x 64 in {256, 512, 768, 1024}, default
layers); everything else - fp32 parity mode, CPU, other layers, `GLR_FUSED_IMG_TX=0` - runs `encoder(flat)` exactly as before.
`GLR_IMG_TX_ATTN=kernel|sdpa` picks the attention of 129 .. 512 regions (up to 128 always run the short kernel)."""

import os

import torch
import torch.nn.functional as F

from .. import _native as N
from . import fused_attn
from .fused_linear import linear, linear_fusable
from .fused_ln import dense_drop_add_ln
from .rng import philox_args
from .workspace import make_workspace

# plain module attributes read at every call: tests and tools flip them (like gloria_model.ENCODER_STREAMS)
ENABLED = os.environ.get("GLR_FUSED_IMG_TX", "1") != "0"
ATTN = os.environ.get("GLR_IMG_TX_ATTN", "sdpa")        # 129 .. 512 regions; the default: profiles/img_tx_ab.txt
_workspace = make_workspace("glr_ffn_workspace_floats", 1 << 19)         # (dev, R, C) -> the backward's partial column sums


def _alive_words(R, C, dev):
    """one `kept && z > 0` bit per element of the [R, C] intermediate"""
    return torch.empty(R, C // 64, dtype=torch.int64, device=dev)


class _ReluDrop(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, p, bias, keep_bits):
        # bias: linear1's bias, handed in only to RECEIVE its gradient (column sums of dz), as _DropAddLN's h_bias
        # keep_bits: False = nothing will be differentiated and p == 0: no bits are stored
        C = z.shape[-1]
        R = z.numel() // C
        dev = z.device
        a = torch.empty_like(z)
        alive = _alive_words(R, C, dev) if (keep_bits or p > 0) else None
        seed, off, cell = philox_args(dev) if p > 0 else (0, 0, None)
        N.check(N.lib().glr_relu_drop_fwd(N.ptr(z), R, C, float(p), seed, off, cell, N.ptr(a), N.ptr(alive), N.stream()),
                "glr_relu_drop_fwd")
        ctx.save_for_backward(alive)
        ctx.p = float(p)
        ctx.b = None if bias is None else (bias.dtype, tuple(bias.shape))
        return a

    @staticmethod
    def backward(ctx, dy):
        (alive,) = ctx.saved_tensors
        C = dy.shape[-1]
        R = dy.numel() // C
        dev = dy.device
        dy = dy.to(torch.bfloat16).contiguous()
        dz = torch.empty_like(dy)
        db = ws = None
        if ctx.b is not None and ctx.needs_input_grad[2]:
            if ctx.b[0] not in (torch.bfloat16, torch.float32) or ctx.b[1] != (C,):
                raise RuntimeError("relu_drop: bias must be a bf16 / fp32 vector of the feed-forward width")
            db = torch.empty(C, dtype=ctx.b[0], device=dev)
            ws = _workspace(dev, R, C)
        N.check(N.lib().glr_relu_drop_bwd(N.ptr(dy), N.ptr(alive), R, C, ctx.p, N.ptr(dz), N.ptr(ws), N.ptr(db),
                                          int(db is not None and db.dtype == torch.bfloat16), N.stream()), "glr_relu_drop_bwd")
        return dz, None, db, None


def relu_drop_ok(C):
    """a feed-forward width the kernels take"""
    return C % 256 == 0 and 256 <= C <= 4096


def relu_drop(z, p, training, bias=None):
    """dropout(relu(z)) of a contiguous bf16 [.., C] GPU tensor.  bias: the bias of the Linear that produced z when that
    Linear left its bias gradient to this op (fused_linear.linear(..., bias_grad_from_epilogue=True))."""
    if not (z.is_cuda and z.dtype == torch.bfloat16 and z.is_contiguous() and relu_drop_ok(z.shape[-1])):
        raise RuntimeError("relu_drop: a contiguous bf16 GPU tensor with a last dimension of 256 k <= 4096 is required")
    keep_bits = torch.is_grad_enabled() and z.requires_grad
    return _ReluDrop.apply(z, p if training else 0.0, bias, keep_bits)


def _layer_ok(layer, E):
    a = layer.self_attn
    return (getattr(layer, "activation_relu_or_gelu", 0) == 1 and not layer.norm_first
            and a.embed_dim == E and E == a.num_heads * 64 and E in (256, 512, 768, 1024)
            and a.in_proj_weight is not None and a.in_proj_bias is not None and a.bias_k is None and a.bias_v is None
            and not a.add_zero_attn and layer.linear1.bias is not None and layer.linear2.bias is not None
            and a.out_proj.bias is not None and relu_drop_ok(layer.linear1.out_features))


def _kernel_attention(x, nh, S):
    """whether S regions run fused_attn's packed kernels: always the short one up to 128, the long one by GLR_IMG_TX_ATTN
    (torch's SDPA where fused_attn's own switches rule them out)"""
    return ((S <= fused_attn._max_tokens() or ATTN == "kernel")
            and fused_attn.packed_fusable(x, nh, nh * 64, S, None))


def fusable(encoder, x):
    """whether run(encoder, x) takes the HIP path: x the local embeddings [B, E, h, w]"""
    if not (ENABLED and x.is_cuda and x.dim() == 4 and torch.is_autocast_enabled("cuda")
            and torch.get_autocast_dtype("cuda") == torch.bfloat16):
        return False
    if ATTN not in ("kernel", "sdpa"):
        raise RuntimeError("GLR_IMG_TX_ATTN must be kernel or sdpa, got %r" % (ATTN,))
    E, S = x.shape[1], x.shape[2] * x.shape[3]
    if encoder.norm is not None or len(encoder.layers) == 0 or not all(_layer_ok(l, E) for l in encoder.layers):
        return False
    return ATTN == "sdpa" or S <= 512                   # the kernel route takes up to 512 regions


def _attention(qkv, nh, p, training):
    B, S, E3 = qkv.shape
    if _kernel_attention(qkv, nh, S):
        return fused_attn.self_attention_packed(qkv, None, nh, p, training)
    q, k, v = qkv.view(B, S, 3, nh, 64).permute(2, 0, 3, 1, 4)           # strided [B, nh, S, 64] views of the packed rows
    o = F.scaled_dot_product_attention(q, k, v, dropout_p=p if training else 0.0)
    return o.transpose(1, 2).reshape(B, S, E3 // 3)


def _layer(layer, x32, x16):
    a, training = layer.self_attn, layer.training
    qkv = linear(x16, a.in_proj_weight, a.in_proj_bias)
    ctx = _attention(qkv, a.num_heads, a.dropout, training)
    y32, y16 = dense_drop_add_ln(a.out_proj, ctx, x32, layer.norm1, layer.dropout1.p, training)
    if y16 is None:
        y16 = y32.to(torch.bfloat16)
    l1 = layer.linear1
    from_epilogue = linear_fusable(y16, l1.weight, l1.bias)
    z = linear(y16, l1.weight, l1.bias, bias_grad_from_epilogue=from_epilogue)
    h = relu_drop(z, layer.dropout.p, training, bias=l1.bias if from_epilogue else None)
    o32, o16 = dense_drop_add_ln(layer.linear2, h, y32, layer.norm2, layer.dropout2.p, training)
    return o32, (o32.to(torch.bfloat16) if o16 is None else o16)


def run(encoder, img_emb_l, pos=None):
    """encoder over the h w regions of img_emb_l [B, E, h, w] (+ pos [h w, E], the position table) -> [B, E, h, w]"""
    b, c, h, w = img_emb_l.shape
    if not fusable(encoder, img_emb_l):
        if pos is not None:
            img_emb_l = img_emb_l + pos.reshape(h, w, c).permute(2, 0, 1).expand(b, c, h, w)
        flat = img_emb_l.reshape(b, c, h * w).permute(2, 0, 1)
        return encoder(flat).permute(1, 2, 0).reshape(b, c, h, w)
    if not img_emb_l.is_contiguous(memory_format=torch.channels_last):
        img_emb_l = img_emb_l.contiguous(memory_format=torch.channels_last)
    tokens = img_emb_l.permute(0, 2, 3, 1).reshape(b, h * w, c)         # a view: the regions' rows as they lie in memory
    x32 = tokens.float()
    if pos is not None:
        x32 = x32 + pos
    x16 = tokens if (pos is None and tokens.dtype == torch.bfloat16) else x32.to(torch.bfloat16)
    for layer in encoder.layers:
        x32, x16 = _layer(layer, x32, x16)
    return x32.view(b, h, w, c).permute(0, 3, 1, 2)
