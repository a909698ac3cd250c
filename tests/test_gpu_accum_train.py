"""Gradient accumulation through gloria.trainer.Trainer on the GPU (8 pairs, own ResNet-50 + a 2-layer BERT, dropout off):
which batches step, the flat bf16 path against an unaccumulated step, the fp32 stock path against hand-run backward
passes, the data-parallel path rehearsed on one rank, and fit()."""

import copy
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 8
DEV = "cuda:0"


def _cfg():
    from gloria.config import pretrain_config
    cfg = pretrain_config("imagenome", batch_size=B)
    cfg.set_path("model.text.bert_config", dict(num_hidden_layers=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0))
    return cfg


def _make(k, seed, precision="bf16", dist_ctx=None, setup=True):
    from gloria import builder
    from gloria.trainer import Trainer
    torch.manual_seed(seed)
    cfg = _cfg()
    model = builder.build_lightning_model(cfg, builder.build_data_module(cfg))
    tr = Trainer(cfg, device=DEV, precision=precision, dist_ctx=dist_ctx, accumulate_grad_batches=k)
    if setup:
        tr.setup(model)
        model.train()
    return tr, model


def _masters(tr):
    return [g.master.clone() for g in tr.optimizer.groups]


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_flat_path_steps_when_the_window_closes():
    """bf16 flat path, k = 2, three batches, the third the epoch's last: optimizer steps after batches 2 and 3 only.
    Without the feature every batch steps."""
    from gloria.datasets.synthetic import make_batch
    tr, model = _make(2, 21)
    assert tr.flat and tr.optimizer.accum == 2 and all(g.grad.dtype == torch.float32 for g in tr.optimizer.groups)
    m0 = _masters(tr)
    steps, calls, losses = [tr.global_step], [], []
    snaps = []
    for i in range(3):
        losses.append(float(tr.training_step(model, make_batch(B, seed=40 + i), i, last_in_epoch=(i == 2))))
        steps.append(tr.global_step)
        calls.append(tr.optimizer.calls)
        snaps.append(_masters(tr))
    assert all(np.isfinite(losses))
    assert steps == [0, 0, 1, 2] and calls == [0, 1, 2]
    assert _equal(snaps[0], m0), "the masters must not move inside a window"
    assert not _equal(snaps[1], snaps[0]) and not _equal(snaps[2], snaps[1])
    assert tr.optimizer.t == 2 and tr.skipped_steps == 0


# Run-to-run spread of the UNACCUMULATED step: three identical k = 1 runs from one seed at this shape (one step on batch
# 40, then the loss on batch 41), measured on an MI355X and recorded in profiles/accum_ab.txt.  The library backward is
# not reproducible at this shape - the first step's gradient norm itself differs by up to 40 % between identical runs (a
# randomly initialised bf16 ResNet-50 + BERT at loss ~12) - so "(g + g) / 2 = g exactly" holds inside a run only:
#   loss on the next batch: relative spread 9.7e-3 (the three pairs: 9.2e-3, 9.7e-3, 4.5e-4)      -> band 4 x = 3.9e-2
#   masters after the step: max |difference| 1.0e-4 = 2 lr (Adam's first step is ~ lr * sign(g), and the signs of
#   near-zero gradient elements flip; 40 M of 134 M elements differ)                              -> band 4 x = 4.0e-4
LOSS_SPREAD, MASTER_SPREAD = 9.7e-3, 1.0e-4


def test_same_batch_twice_equals_one_unaccumulated_step():
    """k = 2 on one batch twice against one k = 1 step on it from the same seed: (g + g) / 2 = g, so the step is the
    same step - the loss on another batch afterwards and the masters agree, inside four times the spread of two
    identical unaccumulated runs (above; the bit-exact check of the sum itself is tests/test_gpu_accum_optim.py)"""
    from gloria.datasets.synthetic import make_batch
    batch, probe = make_batch(B, seed=40), make_batch(B, seed=41)
    tr1, m1 = _make(1, 21)
    tr1.training_step(m1, batch, 0)
    tr2, m2 = _make(2, 21)
    tr2.training_step(m2, batch, 0)
    tr2.training_step(m2, batch, 1)
    assert tr1.global_step == tr2.global_step == 1 and tr1.optimizer.t == tr2.optimizer.t == 1
    names = {id(p): n for n, p in m1.named_parameters()}
    pairs = [(names[id(p)], tr1.optimizer.master_of(p), tr2.optimizer.master_of(q))
             for p, q in zip(m1.parameters(), m2.parameters()) if tr1.optimizer.master_of(p) is not None]
    worst = max(((float((a - b).abs().max()), n) for n, a, b in pairs))
    # the loss on a third batch after the step (a training step each: its forward is what is compared)
    l1 = float(tr1.training_step(m1, probe, 1))
    l2 = float(tr2.training_step(m2, probe, 2, last_in_epoch=True))
    print(f"same batch twice: norm {float(tr2.optimizer.clip_state[0]):.2f} vs {float(tr1.optimizer.clip_state[0]):.2f}; "
          f"loss {l2:.7f} vs {l1:.7f} (rel {abs(l2 - l1) / abs(l1):.2e}); masters max |diff| {worst[0]:.3e} in {worst[1]}")
    np.testing.assert_allclose(l2, l1, rtol=4 * LOSS_SPREAD)
    for n, a, b in pairs:
        np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), rtol=2e-5, atol=4 * MASTER_SPREAD, err_msg=n)


def test_stock_fp32_path_accumulates_in_place():
    """precision 32, stock Adam, k = 2: steps after batches 2 and 3; p.grad after batch 2 is the sum of the two loss / 2
    backward passes (clipped as the trainer clips it), run by hand on a twin.

    The comparison is element-wise at rtol 1e-5, which two runs of the SAME backward only meet when the library kernels
    are reproducible: measured on an MI355X, two hand-run twins differ in all 199 parameters (12.7 M elements outside
    rtol 1e-5; the attention key biases, whose true gradient is zero, are rounding noise altogether), and in none with
    torch.use_deterministic_algorithms(True).  So the test switches that on for its own duration."""
    from gloria.datasets.synthetic import make_batch
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        tr, model = _make(2, 23, precision=32, setup=False)
        twin = copy.deepcopy(model)
        tr.setup(model)
        model.train()
        assert not tr.flat
        twin.to(DEV)
        twin.gloria.img_encoder.to(memory_format=torch.channels_last)
        twin.gloria.dist = None
        twin.train()
        batches = [make_batch(B, seed=60 + i) for i in range(3)]
        w0 = [p.detach().clone() for p in model.parameters()]
        tr.training_step(model, batches[0], 0)
        assert tr.global_step == 0 and _equal([p.detach() for p in model.parameters()], w0)
        tr.training_step(model, batches[1], 1)
        assert tr.global_step == 1 and not _equal([p.detach() for p in model.parameters()], w0)
        got = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}
        for i, b in enumerate(batches[:2]):
            (twin.training_step(tr.to_device(b), i)["loss"] / 2).backward()
        torch.nn.utils.clip_grad_norm_([p for p in twin.parameters() if p.requires_grad], tr.clip)
        worst, n_grads = 0.0, 0
        for n, p in twin.named_parameters():
            assert (p.grad is None) == (got[n] is None), n
            if p.grad is not None:
                n_grads += 1
                worst = max(worst, float((got[n] - p.grad).abs().max() / p.grad.abs().max().clamp_min(1e-30)))
        print(f"stock fp32 window: {n_grads} gradients, worst max|diff| / max|grad| over parameters = {worst:.2e}")
        assert n_grads > 150
        for n, p in twin.named_parameters():          # compared on the device: 60 M elements
            if p.grad is not None:
                torch.testing.assert_close(got[n], p.grad, rtol=1e-5, atol=0, msg=lambda m, n=n: f"{n}: {m}")
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)
    tr.training_step(model, batches[2], 2, last_in_epoch=True)
    assert tr.global_step == 2 and tr.skipped_steps == 0


@pytest.mark.parametrize("overlap", ["0", "1"], ids=["after-backward", "overlapped"])
def test_data_parallel_rehearsal_accumulates(monkeypatch, overlap):
    """single-rank RCCL group: the flat reducer accumulates every bucket into the fp32 flat buffer and all-reduces it in
    the window's last cycle; k = 2, four batches, against the same run without a process group"""
    import torch.distributed as dist
    from gloria import dist as gdist
    from gloria.datasets.synthetic import make_batch
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    for k, v in dict(GLR_FORCE_DIST="1", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                     MASTER_PORT=str(port), GLR_REDUCER_OVERLAP=overlap).items():
        monkeypatch.setenv(k, v)
    batches = [make_batch(B, seed=3 + i) for i in range(4)]
    losses, steps = {}, {}
    try:
        for mode in ("plain", "dist"):
            dctx = gdist.init_from_env("nccl") if mode == "dist" else None
            tr, model = _make(2, 11, dist_ctx=dctx)
            if mode == "dist":
                assert tr.reducer is not None and all(g.grad.dtype == torch.float32 for g in tr.optimizer.groups)
            losses[mode] = [float(tr.training_step(model, b, i)) for i, b in enumerate(batches)]
            steps[mode] = (tr.global_step, tr.optimizer.calls, tr.optimizer.t)
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
    print("rehearsal losses", losses)
    assert steps["dist"] == steps["plain"] == (2, 2, 2)
    assert all(np.isfinite(losses["dist"]))
    np.testing.assert_allclose(losses["dist"], losses["plain"], rtol=2e-2)


class _DM:
    def __init__(self, n):
        from gloria.datasets.synthetic import make_batch
        self.batches = [make_batch(B, seed=80 + i) for i in range(n)]

    def train_dataloader(self):
        return (b for b in self.batches)          # a generator: no len()

    def val_dataloader(self):
        return []


def test_fit_counts_optimizer_steps():
    tr, model = _make(2, 31, setup=False)
    tr.max_epochs = 1
    hist = tr.fit(model, _DM(3))
    assert len(hist) == 3 and tr.global_step == 2 and tr.optimizer.calls == 2
    tr, model = _make(2, 31, setup=False)
    tr.max_epochs = 1
    hist = tr.fit(model, _DM(3), max_steps=1)
    assert len(hist) == 2 and tr.global_step == 1 and tr.optimizer.calls == 1
