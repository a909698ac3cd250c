"""Micro-benchmark of the fused BN(+add)+ReLU kernels against torch's BatchNorm2d + add + relu (MIOpen + aten) on the
activation shapes of ResNet-50 at 299x299, batch 256, channels-last bf16.  Forward and backward are timed
separately (HIP events on the current stream); the effective rate counts the passes of the FUSED scheme
(fwd 3E / 4E with a skip connection, bwd 5E / 7E).
--eval: the eval-mode forward under torch.no_grad() instead (one launch per site, 2E / 3E; the one-launch stem; the
whole image encoder), kernels and torch's eval path alternating in one process, at batch 256 and 32
(profiles/bn_eval_ab.txt is its output).
usage: bench_bn.py [--batch 256] [--only-fused] [--shapes big] | --eval [--shapes big] [--iters 10]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gloria-nlp-project_amd"))
import torch
from gloria.models import fused_bn as FB

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--only-fused", action="store_true")
ap.add_argument("--shapes", default="all")
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--eval", action="store_true",
                help="eval-mode forward under no_grad (glr_bn_infer / fused_stem) against torch's eval path, batch 256 and 32")
args = ap.parse_args()
DEV = "cuda:0"
if not torch.cuda.is_available():
    sys.exit("bench_bn.py measures on the GPU: no device visible")


def cl(t):
    return t.bfloat16().contiguous(memory_format=torch.channels_last)


def eval_bn(c):
    bn = torch.nn.BatchNorm2d(c).to(DEV).eval()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_(0, 0.2)
        bn.running_mean.normal_(0, 0.5)
        bn.running_var.uniform_(0.05, 2.05)
    return bn


def timed_ab(variants, reps):
    """variants: name -> callable.  Each iteration times every variant in turn (alternating A/B in one process): HIP
    events around `reps` calls, 3 warm-up iterations, args.iters timed ones.  -> name -> ms per call"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    tot = dict.fromkeys(variants, 0.0)
    for it in range(3 + args.iters):
        for name, fn in variants.items():
            ev[0].record()
            for _ in range(reps):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            if it >= 3:
                tot[name] += ev[0].elapsed_time(ev[1])
    return {k: v / (args.iters * reps) for k, v in tot.items()}


def switched(on, fn):
    def call():
        FB.EVAL_ENABLED = on
        return fn()
    return call


@torch.no_grad()
def run_eval(shapes):
    print("# eval-mode forward under torch.no_grad(), channels-last bf16; ms per call (HIP events, 3 warm-up + "
          f"{args.iters} timed iterations, kernel and torch alternating); TB/s over the FUSED byte count (2E, 3E with a skip)")
    pool = torch.nn.MaxPool2d(3, stride=2, padding=1)
    for batch in (256, 32):
        reps = 1 if batch >= 256 else 5
        for c, h, w in shapes:
            x = cl(torch.randn(batch, c, h, w, device=DEV))
            bn = eval_bn(c)
            gb = x.numel() * 2 / 1e9
            for res in (False, True):
                r = cl(torch.randn(batch, c, h, w, device=DEV)) if res else None
                t = timed_ab({"kernel": switched(True, lambda: FB.fused_bn_act(bn, x, r, True)),
                              "torch": switched(False, lambda: FB.fused_bn_act(bn, x, r, True))}, reps)
                n = 3 if res else 2
                print(f"({batch},{c},{h},{w}) skip={int(res)} E={gb:.4f} GB  kernel {t['kernel']:.4f} ms ({n * gb / t['kernel']:.2f} TB/s)"
                      f" | torch {t['torch']:.4f} ms ({n * gb / t['torch']:.2f} TB/s) | kernel/torch {t['kernel'] / t['torch']:.2f}",
                      flush=True)
                del r
            if (c, h, w) == (64, 150, 150):
                t = timed_ab({"stem": switched(True, lambda: FB.fused_stem(bn, pool, x)),
                              "two": switched(True, lambda: FB.fused_maxpool(pool, FB.fused_bn_act(bn, x))),
                              "torch": switched(False, lambda: FB.fused_stem(bn, pool, x))}, reps)
                print(f"({batch},{c},{h},{w}) stem bn+relu+maxpool, bytes 1.25E: fused_stem {t['stem']:.4f} ms "
                      f"({1.25 * gb / t['stem']:.2f} TB/s) | bn_infer + maxpool kernels {t['two']:.4f} ms | torch bn + relu, maxpool "
                      f"kernel {t['torch']:.4f} ms | fused_stem/torch {t['stem'] / t['torch']:.2f}", flush=True)
            del x
    # the whole image encoder, eval forward under bf16 autocast (224 x 224 input, resized to 299 x 299 inside)
    from gloria import builder
    from gloria.config import pretrain_config
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enc = builder.build_img_model(pretrain_config("imagenome", batch_size=32)).to(DEV).to(memory_format=torch.channels_last).eval()
    for m in enc.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    parts = []
    for batch in (256, 32):
        imgs = (torch.rand(batch, 3, 224, 224, device=DEV) * 2 - 1).contiguous(memory_format=torch.channels_last)

        def fwd():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return enc(imgs, get_local=True)
        t = timed_ab({"kernel": switched(True, fwd), "torch": switched(False, fwd)}, 1)
        parts.append(f"{batch} images: kernels {t['kernel']:.3f} ms, torch eval path {t['torch']:.3f} ms ({t['kernel'] / t['torch']:.3f})")
    print("image encoder eval forward, bf16 autocast: " + "; ".join(parts), flush=True)
    FB.EVAL_ENABLED = True


def run(n, c, h, w, residual, fused):
    FB.ENABLED = fused
    x = cl(torch.randn(n, c, h, w, device=DEV)).requires_grad_(True)
    r = cl(torch.randn(n, c, h, w, device=DEV)).requires_grad_(True) if residual else None
    dy = cl(torch.randn(n, c, h, w, device=DEV))
    bn = torch.nn.BatchNorm2d(c).to(DEV).train()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    tf = tb = 0.0
    for it in range(3 + args.iters):
        x.grad = None
        if r is not None:
            r.grad = None
        ev[0].record()
        y = FB.fused_bn_act(bn, x, r, True)
        ev[1].record()
        y.backward(dy)
        ev[2].record()
        torch.cuda.synchronize()
        if it >= 3:
            tf += ev[0].elapsed_time(ev[1])
            tb += ev[1].elapsed_time(ev[2])
    return tf / args.iters, tb / args.iters


shapes = [(64, 150, 150), (64, 75, 75), (256, 75, 75), (128, 75, 75), (128, 38, 38), (512, 38, 38), (256, 38, 38),
          (256, 19, 19), (1024, 19, 19), (512, 19, 19), (512, 10, 10), (2048, 10, 10)]
if args.shapes == "big":
    shapes = [(64, 150, 150), (256, 75, 75)]
if args.eval:
    run_eval(shapes)
    sys.exit(0)
for c, h, w in shapes:
    for res in (False, True):
        gb = args.batch * c * h * w * 2 / 1e9
        ff, fb = run(args.batch, c, h, w, res, True)
        line = (f"({args.batch},{c},{h},{w}) skip={int(res)} E={gb:.3f} GB  fused fwd {ff:.3f} ms ({(4 if res else 3) * gb / ff:.2f} TB/s)"
                f" bwd {fb:.3f} ms ({(7 if res else 5) * gb / fb:.2f} TB/s)")
        if not args.only_fused:
            tf, tb = run(args.batch, c, h, w, res, False)
            line += f" | torch fwd {tf:.3f} bwd {tb:.3f} ms | fused/torch {(ff + fb) / (tf + tb):.2f}"
        print(line, flush=True)
