"""Micro-benchmark: the attention kernels (glr_attn_fwd / _bwd up to 128 tokens, glr_attn_long_fwd / _bwd up to 512)
against torch's scaled_dot_product_attention on the BERT shape of the training step (B=256, 12 heads, 97 tokens, dropout
0.1).  B and L come from the environment: `L=258 B=32 python tools/bench_attn.py` is the text leg of scope config 5;
FULL=1 makes every key live instead of the ragged prefixes of 6..41 tokens (the long kernels skip masked key blocks)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gloria-nlp-project_amd"))
import torch
from gloria.models import fused_attn as FA
B, nh, L = int(os.environ.get("B", 256)), 12, int(os.environ.get("L", 97))
H = nh * 64
dev = "cuda:0"
q, k, v = (torch.randn(B, L, H, device=dev).bfloat16().requires_grad_(True) for _ in range(3))
d_o = torch.randn(B, L, H, device=dev).bfloat16()
lens = torch.randint(6, 42, (B,), device=dev)
if os.environ.get("FULL", "0") == "1":
    lens = torch.full((B,), L, device=dev)
km = torch.arange(L, device=dev)[None, :] < lens[:, None]
for fused in (True, False):
    FA.ENABLED = FA.LONG_ENABLED = fused
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    tf = tb = 0.0
    for it in range(13):
        for t in (q, k, v): t.grad = None
        ev[0].record()
        o = FA.self_attention(q, k, v, km, nh, 0.1, True)
        ev[1].record()
        o.backward(d_o)
        ev[2].record()
        torch.cuda.synchronize()
        if it >= 3:
            tf += ev[0].elapsed_time(ev[1]); tb += ev[1].elapsed_time(ev[2])
    print(f"{'fused' if fused else 'sdpa '} fwd {tf / 10 * 1e3:.1f} us  bwd {tb / 10 * 1e3:.1f} us", flush=True)
