"""Three-way measurement of the image encoder's BatchNorm modes on ONE GPU with a single-rank RCCL group: forward +
backward of the image encoder under bf16 autocast (channels-last, 224 x 224 input) at 32 images - the per-rank batch of
the 8-GPU target - and at 256 images, with
  per-rank   nn.BatchNorm2d on the fused kernels (glr_bn_act_*): the default, statistics of this rank's rows
  syncbn     torch.nn.SyncBatchNorm (Trainer(sync_bn=True)): what global-batch statistics cost before sync_bn="fused"
  fused      GlobalBatchNorm2d (Trainer(sync_bn="fused")): glr_bn_sync_* with one all-gather per site and direction
alternating in one process, timed with HIP events after warm-up (the scheme of tools/bench_bn.py).
profiles/sync_bn_ab.txt is its output.
usage: python tools/bench_sync_bn.py [--iters 10] [--batches 32,256] > profiles/sync_bn_ab.txt"""
import argparse
import copy
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gloria-nlp-project_amd"))
os.environ["GLR_FORCE_DIST"] = "1"                       # a process group with one rank
import torch
import torch.distributed as dist
from gloria import builder, dist as gdist
from gloria.config import pretrain_config
from gloria.models import fused_bn as FB

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--batches", default="32,256")
args = ap.parse_args()
DEV = "cuda:0"
if not torch.cuda.is_available():
    sys.exit("bench_sync_bn.py measures on the GPU: no device visible")
if not FB.ENABLED:
    sys.exit("bench_sync_bn.py compares the fused BatchNorm kernels: unset GLR_FUSED_BN=0")


def main():
    dctx = gdist.init_from_env("nccl")
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = builder.build_img_model(pretrain_config("imagenome", batch_size=32)).to(DEV).to(memory_format=torch.channels_last)
    base.train()
    encoders = {
        "per-rank": base,
        "syncbn": torch.nn.SyncBatchNorm.convert_sync_batchnorm(copy.deepcopy(base), dctx.group),
        "fused": FB.convert_global_batchnorm(copy.deepcopy(base), dctx),
    }
    assert sum(isinstance(m, torch.nn.SyncBatchNorm) for m in encoders["syncbn"].modules()) == 53
    assert sum(type(m) is FB.GlobalBatchNorm2d for m in encoders["fused"].modules()) == 53
    print("# image encoder forward + backward, bf16 autocast, channels-last, 224 x 224 input, training mode; one GPU, single-rank "
          "RCCL group")
    print(f"# command: python tools/bench_sync_bn.py --iters {args.iters} --batches {args.batches}")
    print(f"# ms per forward + backward (HIP events, 3 warm-up + {args.iters} timed iterations, the three variants alternating in "
          "one process)")
    print("# per-rank = nn.BatchNorm2d on glr_bn_act_* (statistics of this rank's rows only); syncbn = torch.nn.SyncBatchNorm "
          "(sync_bn=True); fused = GlobalBatchNorm2d on glr_bn_sync_* (sync_bn='fused': 106 all-gathers of <= 32 KB per step)")
    print("# CAVEATS: a single-rank group understates inter-GPU collective latency - the 106 all-gathers of 'fused' here cost "
          "their launch, not a trip over xGMI - and torch.nn.SyncBatchNorm runs NO collective at world size 1 (it falls through "
          "to batch_norm + separate add / relu kernels), so 'syncbn' is its lower bound too.  Multi-rank operation is unverified "
          "on hardware.")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for batch in (int(b) for b in args.batches.split(",")):
        imgs = (torch.rand(batch, 3, 224, 224, device=DEV) * 2 - 1).contiguous(memory_format=torch.channels_last)

        def step(enc):
            for p in enc.parameters():
                p.grad = None
            with torch.autocast("cuda", dtype=torch.bfloat16):
                gl, lo = enc(imgs, get_local=True)
            (gl.float().sum() + lo.float().sum()).backward()
        tot = dict.fromkeys(encoders, 0.0)
        for it in range(3 + args.iters):
            for name, enc in encoders.items():
                ev[0].record()
                step(enc)
                ev[1].record()
                torch.cuda.synchronize()
                if it >= 3:
                    tot[name] += ev[0].elapsed_time(ev[1])
        t = {k: v / args.iters for k, v in tot.items()}
        ratio = t["fused"] / t["syncbn"]                     # within 2 %: the run-to-run spread of these timings
        verdict = "faster than" if ratio < 0.98 else "level with" if ratio <= 1.02 else "SLOWER than"
        print(f"{batch} images: per-rank {t['per-rank']:.3f} ms | syncbn {t['syncbn']:.3f} ms | fused {t['fused']:.3f} ms | "
              f"fused/syncbn {t['fused'] / t['syncbn']:.3f} ({verdict} SyncBatchNorm) | fused - per-rank "
              f"{t['fused'] - t['per-rank']:+.3f} ms ({t['fused'] / t['per-rank']:.3f}x)", flush=True)
        del imgs


try:
    main()
finally:
    if dist.is_initialized():
        dist.destroy_process_group()
