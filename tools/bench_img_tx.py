"""Forward + backward of the image-region transformer stage alone (gloria/models/image_transformer.py): one default
nn.TransformerEncoderLayer (E 768, 12 heads, feed-forward 2048, dropout 0.1) over the 19 x 19 regions of a channels-last bf16
[B, 768, 19, 19] tensor under bf16 autocast, parameters in the flat optimizer's dtypes (bf16 Linears and input projection,
fp32 LayerNorms), with
  stock    the nn.TransformerEncoder itself (GLR_FUSED_IMG_TX=0)
  kernel   the HIP path with fused_attn's long kernel for the 361 regions (GLR_IMG_TX_ATTN=kernel)
  sdpa     the HIP path with torch's scaled_dot_product_attention (GLR_IMG_TX_ATTN=sdpa)
alternating in one process, timed with HIP events after warm-up; medians and the min .. max spread are reported.  Then the
two feed-forward kernels alone at R = B 361 rows, C = 2048: bytes the algorithm needs (4 bytes + 1 bit per element each way)
over the event time, against the achievable HBM rate.  profiles/img_tx_ab.txt is its output.
usage: python tools/bench_img_tx.py [--iters 20] [--batches 32,256] > profiles/img_tx_ab.txt"""
import argparse
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gloria-nlp-project_amd"))
import torch
import torch.nn as nn
from gloria import _native as N
from gloria.models import image_transformer as IT
from gloria.optim import shadow_parameter_ids

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--batches", default="32,256")
args = ap.parse_args()
DEV = "cuda:0"
HBM_TBS = 6.3                     # achievable HBM rate of the MI355X (8 TB/s peak)
if not torch.cuda.is_available():
    sys.exit("bench_img_tx.py measures on the GPU: no device visible")

VARIANTS = {"stock": (False, "sdpa"), "kernel": (True, "kernel"), "sdpa": (True, "sdpa")}


def stage(enc, x, proj, variant):
    IT.ENABLED, IT.ATTN = VARIANTS[variant]
    x.grad = None
    enc.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = IT.run(enc, x)
    out.backward(proj)


def timed(fn, iters):
    """ms of each of `iters` calls (HIP events)"""
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def fmt(ts):
    return "median %8.3f  min %8.3f  max %8.3f" % (statistics.median(ts), min(ts), max(ts))


def main():
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enc = nn.TransformerEncoder(nn.TransformerEncoderLayer(768, 12), 1, enable_nested_tensor=False).to(DEV).train()
    shadows = shadow_parameter_ids(enc)
    for p in enc.parameters():
        if id(p) in shadows:
            p.data = p.data.bfloat16()
    print("# image-region transformer stage, forward + backward: 1 layer, E 768, 12 heads, ff 2048, dropout 0.1, 361 regions,")
    print("# bf16 autocast, channels-last bf16 input, bf16 Linear / in_proj parameters, fp32 LayerNorms, training mode")
    print(f"# command: python tools/bench_img_tx.py --iters {args.iters} --batches {args.batches}")
    print(f"# ms per forward + backward (HIP events, 3 warm-up rounds + {args.iters} timed rounds, the variants alternating in one process)")
    print("# the full training step of this configuration was NOT benchmarked (bench.py measures the default configuration)")
    for B in (int(b) for b in args.batches.split(",")):
        x = torch.randn(B, 768, 19, 19, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        proj = torch.randn(B, 768, 19, 19, device=DEV).contiguous(memory_format=torch.channels_last)
        times = {v: [] for v in VARIANTS}
        for rnd in range(3 + args.iters):
            for v in VARIANTS:
                t = timed(lambda: stage(enc, x, proj, v), 1)
                if rnd >= 3:
                    times[v] += t
        for v in VARIANTS:
            print("B %4d  %-7s %s" % (B, v, fmt(times[v])))
        stock = statistics.median(times["stock"])
        print("B %4d  stock spread (max - min) %.3f ms; kernel - stock %+.3f ms; sdpa - stock %+.3f ms" % (
            B, max(times["stock"]) - min(times["stock"]), statistics.median(times["kernel"]) - stock,
            statistics.median(times["sdpa"]) - stock))
        # the two feed-forward kernels alone
        R, C, p = B * 361, 2048, 0.1
        L = N.lib()
        z = torch.randn(R, C, device=DEV).bfloat16()
        a = torch.empty_like(z)
        alive = torch.empty(R, C // 64, dtype=torch.int64, device=DEV)
        ws = torch.empty(L.glr_ffn_workspace_floats(R, C), device=DEV)
        db = torch.empty(C, device=DEV, dtype=torch.bfloat16)
        calls = {
            "glr_relu_drop_fwd p=0.1": lambda: N.check(L.glr_relu_drop_fwd(N.ptr(z), R, C, p, 1, 0, None, N.ptr(a), N.ptr(alive), N.stream()), "fwd"),
            "glr_relu_drop_fwd p=0  ": lambda: N.check(L.glr_relu_drop_fwd(N.ptr(z), R, C, 0.0, 1, 0, None, N.ptr(a), N.ptr(alive), N.stream()), "fwd"),
            "glr_relu_drop_bwd      ": lambda: N.check(L.glr_relu_drop_bwd(N.ptr(z), N.ptr(alive), R, C, p, N.ptr(a), N.ptr(ws), N.ptr(db), 1, N.stream()), "bwd"),
        }
        gbytes = R * C * (2 + 2 + 1 / 8) / 1e9
        for name, fn in calls.items():
            timed(fn, 3)
            ts = timed(fn, args.iters)
            med = statistics.median(ts)
            print("R %6d C %d  %s %s ms  %.2f GB -> %.2f TB/s = %.0f %% of %.1f TB/s (HBM-bound estimate; event time includes the launch)" % (
                R, C, name, fmt(ts), gbytes, gbytes / med, 100 * gbytes / med / HBM_TBS, HBM_TBS))
        del z, a, alive


main()
