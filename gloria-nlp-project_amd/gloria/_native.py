"""ctypes binding of libglr.so (C ABI: include/glr.h).

The product path has NO fallback: if the HIP library is missing or a call fails, a
RuntimeError is raised.  torch is used only for device memory and the current stream.
"""

import ctypes
import os
from ctypes import c_float, c_int, c_int64, c_void_p, POINTER

import numpy as np
import torch

GLR_F32, GLR_BF16 = 0, 1
AGG = {"sum": 0, "mean": 1, "max": 2}
TILE_WORDS = 64
MAX_SPAD = 384

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "lib", "libglr.so"))

SYMBOLS = {
    # name: (restype, argtypes)
    "glr_version": (c_int, []),
    "glr_region_pad": (c_int, [c_int]),
    "glr_tile_capacity": (c_int, [c_int]),
    "glr_plan_size": (c_int, [c_void_p, c_int, c_int]),
    "glr_plan_build": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int]),
    "glr_tile_k": (c_int, [c_void_p, c_void_p, c_int, ctypes.c_longlong, c_int, c_void_p]),
    "glr_pack_regions": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "glr_pack_regions_tiled": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                       c_void_p]),
    "glr_tile_gram": (c_int, [c_void_p, c_void_p, c_int, ctypes.c_longlong, c_int, c_int, c_void_p]),
    "glr_pack_words": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                               c_int, c_int, c_int, c_void_p]),
    "glr_local_attn_fwd": (c_int, [c_void_p] * 6 + [c_int] * 3 + [c_float] * 3 + [c_int, c_float, c_void_p, c_int,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
                                   # vt, gram, tp, tnorm, plan, plan_dev, B_img, D, S_eff, temp1..3, agg, eps,
                                   # sim, ld, lse, wstat, attn, attn_off, strip, pair_only, img_offset, amean, a1buf, dtype, stream
    "glr_local_attn_bwd": (c_int, [c_void_p] * 6 + [c_int] * 3 + [c_float] * 3
                           + [c_int, c_float, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                              c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
                                   # ..., sim, dsim, ld, lse, wstat, damean, dattn, attn_off, strip, img_offset,
                                   # xout, aout, baout, gamma, beta, a1buf, dtype, stream
    "glr_sumsq_blocks": (c_int, [ctypes.c_longlong]),
    "glr_gather_mt": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "glr_accum_mt": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_float, c_int, c_void_p]),
    "glr_sumsq_mt": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "glr_adam_step_mt": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float,
                                 c_float, c_float, c_float, c_int, c_void_p, c_void_p]),
    "glr_sumsq_partial": (c_int, [c_void_p, c_int, ctypes.c_longlong, c_void_p, c_void_p]),
    "glr_clip_coef": (c_int, [c_void_p, c_int, c_float, c_void_p, c_void_p]),
    "glr_adam_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, ctypes.c_longlong, c_float,
                              c_float, c_float, c_float, c_float, c_int, c_void_p, c_void_p]),
    "glr_sumsq_partial_g": (c_int, [c_void_p, c_int, ctypes.c_longlong, c_void_p, c_void_p, c_void_p]),
    "glr_sumsq_mt_g": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "glr_step_guard": (c_int, [c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p, ctypes.c_longlong, c_void_p]),
    "glr_adam_step_g": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, ctypes.c_longlong, c_float,
                                c_float, c_float, c_float, c_float, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "glr_adam_step_mt_g": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                   c_float, c_float, c_float, c_float, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "glr_adam_bias_table": (c_int, [c_float, c_float, c_int, c_void_p]),
    "glr_bn_workspace_floats": (c_int, [ctypes.c_longlong, c_int]),
    "glr_bn_act_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_longlong, c_int, c_float, c_float, c_int,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "glr_bn_act_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_longlong,
                               c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "glr_bn_sync_partial_fwd": (c_int, [c_void_p, ctypes.c_longlong, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "glr_bn_sync_apply_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, ctypes.c_longlong, c_int,
                                      c_float, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_int, c_void_p]),
    "glr_bn_sync_partial_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        ctypes.c_longlong, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "glr_bn_sync_apply_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                      c_void_p, ctypes.c_longlong, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "glr_bn_infer": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_longlong, c_int, c_float,
                             c_int, c_void_p, c_int, c_void_p]),
    "glr_bn_relu_maxpool3s2_infer": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                             c_float, c_void_p, c_void_p]),
    "glr_ln_workspace_floats": (c_int, [ctypes.c_longlong, c_int]),
    "glr_drop_add_ln_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_longlong, c_int, c_float, c_float,
                                    ctypes.c_ulonglong, ctypes.c_ulonglong, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p]),
    "glr_drop_add_ln_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_longlong,
                                    c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "glr_drop_add_ln_rows_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_longlong, c_int, c_float,
                                         c_float, ctypes.c_ulonglong, ctypes.c_ulonglong, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p]),
    "glr_embedding_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "glr_type_embedding_workspace_floats": (c_int, [ctypes.c_longlong, c_int]),
    "glr_type_embedding_bwd": (c_int, [c_void_p, c_void_p, ctypes.c_longlong, c_int, c_void_p, c_void_p, c_void_p]),
    "glr_colsum_workspace_floats": (c_int, [ctypes.c_longlong, c_int]),
    "glr_colsum_bf16": (c_int, [c_void_p, ctypes.c_longlong, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "glr_ffn_workspace_floats": (c_int, [ctypes.c_longlong, c_int]),
    "glr_relu_drop_fwd": (c_int, [c_void_p, ctypes.c_longlong, c_int, c_float, ctypes.c_ulonglong, ctypes.c_ulonglong, c_void_p,
                                  c_void_p, c_void_p, c_void_p]),
    "glr_relu_drop_bwd": (c_int, [c_void_p, c_void_p, ctypes.c_longlong, c_int, c_float, c_void_p, c_void_p, c_void_p, c_int,
                                  c_void_p]),
    "glr_attn_max_tokens": (c_int, [c_int]),
    "glr_attn_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_float,
                             ctypes.c_ulonglong, ctypes.c_ulonglong, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "glr_attn_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                             c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "glr_attn_rows_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_float,
                                  ctypes.c_ulonglong, ctypes.c_ulonglong, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "glr_attn_rows_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_int, c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "glr_attn_long_max_tokens": (c_int, []),
    "glr_attn_long_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_float,
                                  ctypes.c_ulonglong, ctypes.c_ulonglong, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "glr_attn_long_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                  c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "glr_upsample_bilinear_cl": (c_int, [c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong,
                                         c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "glr_maxpool3s2_fwd": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "glr_maxpool3s2_bwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "glr_cell_counts": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "glr_kth_value": (c_int, [c_void_p, c_int, ctypes.c_longlong, ctypes.c_longlong, c_void_p, c_void_p]),
    "glr_topk_desc": (c_int, [c_void_p, c_int, ctypes.c_longlong, c_int, c_void_p, c_void_p, c_void_p]),
    "glr_threshold_counts": (c_int, [c_void_p, c_void_p, c_void_p, c_int, ctypes.c_longlong, c_void_p, c_void_p]),
    "glr_attn_reg_fwd": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "glr_attn_reg_bwd": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "glr_image_minmax": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "glr_collate_images": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "glr_aug_geom": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "glr_aug_jitter": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "glr_u8_to_tensor": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "glr_selftest_quotient": (c_int, [c_int, c_int, c_void_p, c_void_p]),
    "glr_dual_ce_fwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "glr_dual_ce_bwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "glr_global_sim_fwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_void_p, c_int,
                                   c_void_p, c_void_p, c_void_p]),
    "glr_global_sim_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                   c_float, c_float, c_void_p, c_void_p, c_void_p]),
    "glr_wordpiece_segsum_fwd": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                         c_int, c_void_p]),
    "glr_wordpiece_segsum_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                         c_int, c_void_p]),
    "glr_wordpiece_segsum_rows_fwd": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                              c_int, c_int, c_void_p]),
    "glr_wordpiece_segsum_rows_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                              c_int, c_int, c_void_p]),
    "glr_attn_sup_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                 c_void_p, c_void_p, c_void_p]),
    "glr_cosine_fwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p]),
    "glr_cosine_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p,
                               c_void_p]),
}

_lib = None


def lib():
    """Load libglr.so (once).  Raises if it has not been built: there is no CPU path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the GLoRIA hot path needs the HIP library "
                "(build it with `python -c 'import __graft_entry__ as g; g.build()'` or `make -C csrc`)")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(handle, name)          # AttributeError if the ABI is incomplete
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def check(code, what):
    if code != 0:
        raise RuntimeError(f"libglr: {what} failed with code {code}")


def dtype_code(dt):
    if dt == torch.float32:
        return GLR_F32
    if dt == torch.bfloat16:
        return GLR_BF16
    raise TypeError(f"libglr supports float32 and bfloat16 tensors, got {dt}")


def torch_dtype(code):
    return torch.float32 if code == GLR_F32 else torch.bfloat16


def ptr(t):
    """device address of a tensor as a plain int (ctypes converts it for a c_void_p parameter) or None"""
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream():
    """the current HIP stream of the current device as a plain int (ctypes converts it for a void* parameter); the raw
    accessor avoids building a torch.cuda.Stream object per launch (the 32-pair step is bound by host time)"""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def upload(array, device):
    """host numpy array -> device tensor through PINNED staging memory, asynchronously on the current stream.  A copy
    from pageable memory is staged by the runtime and can hold the host until the stream has drained - in the middle of
    a training step that parks the host behind the whole encoder forward, and the launches that follow then run with the
    GPU idle between them (measured as 0.4 - 0.8 ms of gaps inside the K1 forward op at 256 pairs).  torch's caching
    host allocator recycles the pinned block once the copy's event has passed."""
    t = torch.from_numpy(np.ascontiguousarray(array))
    if torch.device(device).type != "cuda":
        return t.to(device)
    return t.pin_memory().to(device, non_blocking=True)


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("the GLoRIA hot path runs on the GPU only (HIP kernels); got a CPU tensor")


MAX_PAIR_SEG = 8        # GLR_MAX_PAIR_SEG: sentences per tile pair (table rows of the pair kernels)
PLAN_HEADER = 64        # GLR_PLAN_HEADER; header words: include/glr.h (GLR_PLAN_*)


class TilePlan:
    """Sentence -> word-slot packing and K1 work items: glr_plan_build into one int32 buffer (`host`), one upload, and
    the arrays of include/glr.h as views of the device copy."""

    def __init__(self, cap_lens, device, capacity=TILE_WORDS, allow_pairs=True):
        cl = np.ascontiguousarray(np.asarray(cap_lens, dtype=np.int32))
        n = int(cl.shape[0])
        L = lib()
        size = L.glr_plan_size(cl.ctypes.data_as(c_void_p), n, capacity)
        if size <= 0:
            raise ValueError(f"cap_lens must be in [1, 512] (glr_plan_size -> {size})")
        buf = np.empty(size, dtype=np.int32)
        used = L.glr_plan_build(cl.ctypes.data_as(c_void_p), n, capacity, 1 if allow_pairs else 0,
                                buf.ctypes.data_as(c_void_p), size)
        if used <= 0:
            raise ValueError(f"glr_plan_build failed ({used})")
        self.host = host = buf[:used]
        (self.n_sent, self.n_tiles, self.capacity, n_order, self.n_single, self.n_pair, self.n_long_pair,
         _) = (int(v) for v in host[:8])
        self.n_slots = self.n_tiles * TILE_WORDS
        dev = upload(host, device)
        names = ("cap_lens", "sent_slot0", "tile_first", "order", "tile_nsub", "single_tile", "pair_tile", "pair_desc")
        lens = (n, n, self.n_tiles + 1, n_order, self.n_tiles, self.n_single, self.n_pair, self.n_pair * 64)
        for name, off, ln in zip(names, host[8:16].tolist(), lens):
            setattr(self, name, dev[off:off + ln])
        if not self.n_pair:
            self.pair_desc = None
        self.cap_lens_host = cl
        self.sent_slot0_host = host[int(host[9]):int(host[9]) + n]
        self.n_words = int(cl.sum())
        self._dev = dev
        self._word_index = None

    def word_index(self, device):
        """(sentence, word, slot) of every packed word, as device int64 tensors (for scattering the
        packed word gradient back to [B, D, L])."""
        if self._word_index is None:
            si = np.repeat(np.arange(self.n_sent), self.cap_lens_host)
            wi = np.concatenate([np.arange(n) for n in self.cap_lens_host])
            slot = self.sent_slot0_host[si].astype(np.int64) + (wi // self.capacity) * TILE_WORDS + wi % self.capacity
            self._word_index = tuple(upload(a.astype(np.int64), device) for a in (si, wi, slot))
        return self._word_index

    def attn_offsets(self, s_out, device):
        off = np.zeros(self.n_sent + 1, dtype=np.int64)
        np.cumsum(self.cap_lens_host.astype(np.int64) * s_out, out=off[1:])
        return upload(off[:-1].copy(), device), off
