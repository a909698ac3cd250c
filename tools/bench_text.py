"""Micro-benchmark: the text encoder alone (BERT-base, 256 captions of 97 tokens, bf16 autocast, bf16 Linear parameters,
dropout 0.1), forward + backward per step, on the real token rows (GLR_TEXT_PACKED route, gloria/models/text_rows.py)
against the padded path - with one fixed batch, as bench.py repeats it, and cycling four batches of different seeds, as
training does: the row count T then changes every step (hipBLASLt shape lookups, allocator growth).

    python tools/bench_text.py [steps]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gloria-nlp-project_amd"))
import torch
from gloria.config import pretrain_config
from gloria.datasets.synthetic import make_batch
from gloria.models import text_model as TM
from gloria.models import text_rows as TR

B = int(os.environ.get("B", 256))
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 16
dev = torch.device("cuda", 0)
torch.manual_seed(0)
enc = TM.BertEncoder(pretrain_config("imagenome", batch_size=B)).to(dev).train()
for m in enc.modules():
    if isinstance(m, torch.nn.Linear):
        m.to(torch.bfloat16)


def device_batch(seed):
    b = make_batch(B, seed=seed, lengths="words")
    out = []
    for k in ("caption_ids", "attention_mask", "token_type_ids"):
        t = b[k].to(dev)
        t._glr_host = b[k].numpy()
        out.append(t)
    return out, int(b["attention_mask"].sum())


batches = [device_batch(s) for s in (1234, 1235, 1236, 1237)]
print("real token rows per batch:", [n for _, n in batches], "of", B * 97)


def step(batch):
    enc.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        word, sent, _ = enc(*batch)
    (word.float().square().mean() + sent.float().square().mean()).backward()


def run(packed, cycle):
    TR.ENABLED = packed
    pick = (lambda i: batches[i % 4][0]) if cycle else (lambda i: batches[0][0])
    for i in range(8):
        step(pick(i))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        step(pick(i))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


for cycle in (False, True):
    for packed in (False, True):
        ms = run(packed, cycle)
        print(f"{'cycling 4 batches' if cycle else 'fixed batch      '}  {'packed rows' if packed else 'padded     '}  "
              f"{ms:7.2f} ms per step (forward + backward)", flush=True)
print(f"allocator: {torch.cuda.max_memory_reserved() / 2 ** 20:.0f} MiB reserved at peak")
