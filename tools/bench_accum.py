"""What gradient accumulation costs per micro-batch: the bf16 flat training step of bench.py's workload (256 pairs, one
GPU, BERT-base + ResNet-50) with accumulate_grad_batches k = 1, 2, 4 - three trainers alternating in one process, every
micro-batch timed with HIP events after warm-up - and glr_accum_mt alone over the model's real parameter set (the k = 2
optimizer's chunk and pointer tables; first = 1 and first = 0), with the bytes it moves against the HBM peak.
profiles/accum_ab.txt is its output.
usage: python tools/bench_accum.py [--windows 6] [--batch 256] > profiles/accum_ab.txt"""
import argparse
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gloria-nlp-project_amd"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")   # before the HIP runtime starts: gloria/hipgraph.py
import torch
from gloria import _native as N
from gloria import builder, miopen_env
from gloria.config import pretrain_config
from gloria.datasets.synthetic import make_batch
from gloria.trainer import Trainer

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=6, help="timed windows of 4 micro-batches per variant")
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--kernel-iters", type=int, default=20)
args = ap.parse_args()
DEV = "cuda:0"
HBM_PEAK = 8.0e12            # bytes / s: MI355X HBM3E
KS = (1, 2, 4)
if not torch.cuda.is_available():
    sys.exit("bench_accum.py measures on the GPU: no device visible")


def build(k, find):
    cfg = pretrain_config("imagenome", batch_size=args.batch)
    torch.manual_seed(1234)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = builder.build_lightning_model(cfg, builder.build_data_module(cfg))
    tr = Trainer(cfg, device=DEV, precision="bf16", miopen_benchmark=find, accumulate_grad_batches=k)
    tr.setup(model)
    model.train()
    return tr, model


def main():
    find = miopen_env.activate()
    runs = {k: build(k, find) for k in KS}
    batch = runs[1][0].to_device(make_batch(args.batch, seed=1234))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    print(f"# bf16 flat training step, {args.batch} pairs, one GPU, 12 BERT layers, synthetic batch (bench.py's workload)")
    print(f"# command: python tools/bench_accum.py --windows {args.windows} --batch {args.batch}")
    print(f"# ms per MICRO-BATCH (forward + backward + its share of the optimizer work), HIP events around every micro-batch; "
          f"2 warm-up + {args.windows} timed rounds of 4 micro-batches per variant, the variants alternating round by round "
          "(rotating order) in one process")
    samples = {k: [[] for _ in range(k)] for k in KS}            # per position in the window
    for rnd in range(2 + args.windows):
        for k in KS[rnd % 3:] + KS[:rnd % 3]:                    # the order rotates: no variant always follows the same one
            tr, model = runs[k]
            for j in range(4):
                ev[0].record()
                tr.training_step(model, batch, j)
                ev[1].record()
                torch.cuda.synchronize()
                if rnd >= 2:
                    samples[k][j % k].append(ev[0].elapsed_time(ev[1]))

    def median(xs):
        xs = sorted(xs)
        return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])
    t = {k: sum(map(sum, samples[k])) / sum(map(len, samples[k])) for k in KS}
    med = {k: median([x for pos in samples[k] for x in pos]) for k in KS}
    for k in KS:
        pos = " ".join(f"{median(v):.2f}" for v in samples[k])
        print(f"k = {k}: mean {t[k]:.3f} ms, median {med[k]:.3f} ms per micro-batch (median {med[k] / med[1]:.4f} x k = 1; "
              f"max {max(max(v) for v in samples[k]):.2f}; median by position in the window: {pos})")
    # the kernel alone, on the k = 2 optimizer's own tables with synthetic gradients in the parameters' dtypes
    opt = runs[2][0].optimizer
    n_par = sum(g.n for g in opt.groups)
    for g in opt.groups:
        for p in g.params:
            p.grad = torch.zeros_like(p)
        g.stage_grad_pointers()
    L, st = N.lib(), N.stream()
    for first in (1, 0):
        def launch():
            for g in opt.groups:
                N.check(L.glr_accum_mt(N.ptr(g.table), g.n_chunks, N.ptr(g.ptr_dev), N.dtype_code(g.sdt), N.ptr(g.grad), 0.5,
                                       first, st), "glr_accum_mt")
        for _ in range(3):
            launch()
        ev[0].record()
        for _ in range(args.kernel_iters):
            launch()
        ev[1].record()
        torch.cuda.synchronize()
        ms = ev[0].elapsed_time(ev[1]) / args.kernel_iters
        nbytes = sum(sum(p.numel() for p in g.params) * ((2 if g.sdt == torch.bfloat16 else 4) + 4 + (0 if first else 4))
                     for g in opt.groups)
        print(f"glr_accum_mt first = {first}: {ms:.4f} ms for {n_par} accumulator elements in {len(opt.groups)} launches "
              f"({sum(g.n_chunks for g in opt.groups)} workgroups), {nbytes / 1e9:.3f} GB moved -> {nbytes / ms / 1e9:.1f} TB/s "
              f"... {nbytes / (ms * 1e-3) / HBM_PEAK * 100:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak")
    for g in opt.groups:
        for p in g.params:
            p.grad = None


main()
