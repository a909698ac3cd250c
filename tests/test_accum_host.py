"""Gradient accumulation without a GPU: argument checking, the window bookkeeping of Trainer.training_step / fit on a
CPU toy with a stock optimizer, and the stock GradReducer over a window of micro-batches on two gloo ranks."""

import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

WORLD = 2
LR = 0.1


def _cfg(k=None):
    from gloria.config import pretrain_config
    cfg = pretrain_config("imagenome", batch_size=4)
    cfg.set_path("lightning.trainer.precision", 32)
    cfg.set_path("lightning.trainer.gradient_clip_val", None)     # plain SGD arithmetic below
    cfg.set_path("lightning.trainer.max_epochs", 1)
    if k is not None:
        cfg.set_path("lightning.trainer.accumulate_grad_batches", k)
    return cfg


class _Toy(torch.nn.Module):
    """what Trainer needs of the Lightning module: .gloria, configure_optimizers, training_step / validation_step"""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.gloria = torch.nn.Linear(3, 2)
        self.current_epoch = 0

    def configure_optimizers(self):
        return {"optimizer": torch.optim.SGD(self.parameters(), lr=LR), "lr_scheduler": None}

    def training_step(self, batch, batch_idx):
        return {"loss": (self.gloria(batch["x"]) ** 2).mean()}

    validation_step = training_step


def _batches(n):
    g = torch.Generator().manual_seed(5)
    return [{"x": torch.randn(4, 3, generator=g)} for _ in range(n)]


class _Loader:
    """iterable without __len__: fit must find the last batch by looking ahead"""

    def __init__(self, batches):
        self.batches = batches

    def __iter__(self):
        return (b for b in self.batches)


class _DM:
    def __init__(self, batches):
        self.batches = batches

    def train_dataloader(self):
        return _Loader(self.batches)

    def val_dataloader(self):
        return _Loader([])


@pytest.mark.parametrize("bad", [0, -1, 2.5])
def test_bad_accumulate_grad_batches_raises(bad):
    from gloria.trainer import Trainer
    with pytest.raises(ValueError):
        Trainer(_cfg(), device="cpu", accumulate_grad_batches=bad)
    with pytest.raises(ValueError):
        Trainer(_cfg(bad), device="cpu")


def test_default_and_override():
    from gloria.trainer import Trainer
    assert Trainer(_cfg(), device="cpu").accumulate == 1
    assert Trainer(_cfg(4), device="cpu").accumulate == 4
    assert Trainer(_cfg(4), device="cpu", accumulate_grad_batches=2).accumulate == 2
    from gloria.config import pretrain_config
    assert "accumulate_grad_batches" in pretrain_config().lightning.trainer
    assert pretrain_config().lightning.trainer.accumulate_grad_batches is None


def _hand_window(model, batches, k):
    """one SGD step on (1/k) x the sum of the batches' gradients"""
    params = list(model.parameters())
    tot = [torch.zeros_like(p) for p in params]
    for b in batches:
        gs = torch.autograd.grad(model.training_step(b, 0)["loss"] / k, params)
        tot = [t + g for t, g in zip(tot, gs)]
    with torch.no_grad():
        for p, t in zip(params, tot):
            p.sub_(LR * t)


def test_training_step_window_bookkeeping():
    """k = 2, five batches with the epoch's end on the third: optimizer steps after batches 2, 3 (the flush of a
    one-batch window, scale still 1/2) and 5; weights otherwise untouched; the loss returned is the micro-batch's own"""
    from gloria.trainer import Trainer
    model, twin = _Toy(), _Toy()
    tr = Trainer(_cfg(2), device="cpu")
    tr.setup(model)
    model.train()
    batches = _batches(5)
    last_flags = [False, False, True, False, False]
    steps_after, snap = [], [p.detach().clone() for p in model.parameters()]
    windows = [batches[0:2], batches[2:3], batches[3:5]]
    closes = {1: 0, 2: 1, 4: 2}
    for i, (b, last) in enumerate(zip(batches, last_flags)):
        own = float(twin.training_step(b, i)["loss"].detach()) if i in (0, 2, 3) else None   # twin == model at window starts
        loss = float(tr.training_step(model, b, i, last_in_epoch=last))
        if own is not None:
            np.testing.assert_allclose(loss, own, rtol=1e-6)        # undivided
        steps_after.append(tr.global_step)
        now = [p.detach().clone() for p in model.parameters()]
        if i in closes:
            _hand_window(twin, windows[closes[i]], 2)
            for p, q in zip(now, twin.parameters()):
                np.testing.assert_allclose(p.numpy(), q.detach().numpy(), rtol=1e-6, atol=1e-8)
            assert not all(torch.equal(a, b_) for a, b_ in zip(now, snap))
        else:
            assert all(torch.equal(a, b_) for a, b_ in zip(now, snap)), f"batch {i} must not step"
        snap = now
    assert steps_after == [0, 1, 2, 2, 3]
    assert tr.skipped_steps == 0 and int(tr._record[0]) == 3       # the stock guard ran once per window


def test_k1_steps_every_batch():
    from gloria.trainer import Trainer
    model, twin = _Toy(), _Toy()
    tr = Trainer(_cfg(), device="cpu")
    tr.setup(model)
    for i, b in enumerate(_batches(3)):
        tr.training_step(model, b, i)
        _hand_window(twin, [b], 1)
        assert tr.global_step == i + 1
        for p, q in zip(model.parameters(), twin.parameters()):
            np.testing.assert_allclose(p.detach().numpy(), q.detach().numpy(), rtol=1e-6, atol=1e-8)


def test_fit_flushes_at_epoch_end_and_counts_optimizer_steps():
    from gloria.trainer import Trainer
    batches = _batches(3)
    model, twin = _Toy(), _Toy()
    tr = Trainer(_cfg(2), device="cpu")
    hist = tr.fit(model, _DM(batches))
    assert len(hist) == 3 and tr.global_step == 2 and tr._micro == 0
    _hand_window(twin, batches[:2], 2)
    _hand_window(twin, batches[2:], 2)
    for p, q in zip(model.parameters(), twin.parameters()):
        np.testing.assert_allclose(p.detach().numpy(), q.detach().numpy(), rtol=1e-6, atol=1e-8)
    # max_steps counts optimizer steps: 1 is reached after batch 2
    model = _Toy()
    tr = Trainer(_cfg(2), device="cpu")
    hist = tr.fit(model, _DM(batches), max_steps=1)
    assert len(hist) == 2 and tr.global_step == 1
    # two epochs of three batches: the window never straddles the epoch boundary
    cfg = _cfg(2)
    cfg.set_path("lightning.trainer.max_epochs", 2)
    tr = Trainer(cfg, device="cpu")
    hist = tr.fit(_Toy(), _DM(batches))
    assert len(hist) == 6 and tr.global_step == 4


# ---------------------------------------------------------------- two gloo ranks, stock GradReducer
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _net():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3), torch.nn.Linear(3, 1))


def _x(rank, micro):
    return torch.full((2, 6), float(rank + 1)) + 0.25 * micro


def _worker(rank, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(WORLD))
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    try:
        from gloria.dist import DistContext, GradReducer
        dctx = DistContext()
        lin = _net()
        half = torch.nn.Parameter(torch.ones(3))       # used in the first micro-batch only
        unused = torch.nn.Parameter(torch.ones(4))     # never receives a gradient
        plist = list(lin.parameters()) + [half, unused]
        red = GradReducer(plist, dctx, bucket_bytes=64)
        # a window of two micro-batches
        red.begin(True, False)
        (lin(_x(rank, 0)).sum() + (half * (rank + 1)).sum()).backward()
        red.finish()
        mid = [None if p.grad is None else p.grad.clone() for p in plist]      # local sums, nothing reduced yet
        red.begin(False, True)
        lin(_x(rank, 1)).sum().backward()
        red.finish()
        window = [None if p.grad is None else p.grad.clone() for p in plist]
        # a second backward inside one cycle of a window is refused
        red.begin(True, False)
        lin(_x(rank, 0)).sum().backward()
        double = False
        try:
            lin(_x(rank, 0)).sum().backward()
        except RuntimeError as e:
            double = "one backward per" in str(e)
        red.finish()
        # zero_grad() / finish() without the new call: one backward, reduced at once, unused hidden
        red.zero_grad()
        attached = all(p.grad is not None for p in plist)
        lin(_x(rank, 0)).sum().backward()
        red.finish()
        plain = [None if p.grad is None else p.grad.clone() for p in plist]
        torch.save({"mid": mid, "window": window, "double": double, "attached": attached, "plain": plain},
                   os.path.join(out, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_stock_reducer_window_on_two_gloo_ranks(tmp_path):
    mp.spawn(_worker, args=(_free_port(), str(tmp_path)), nprocs=WORLD, join=True)
    res = [torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(WORLD)]
    lin = _net()
    params = list(lin.parameters())

    def grads(x):
        return torch.autograd.grad(lin(x).sum(), params)

    local0 = [grads(_x(r, 0)) for r in range(WORLD)]
    total = [sum(grads(_x(r, m))[j] for r in range(WORLD) for m in range(2)) for j in range(len(params))]
    first_only = [sum(local0[r][j] for r in range(WORLD)) for j in range(len(params))]
    for r in range(WORLD):
        # after the first micro-batch: this rank's own gradients, not reduced
        for a, b in zip(res[r]["mid"][:len(params)], local0[r]):
            np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-6, atol=1e-7)
        # after the window: the sum over ranks and micro-batches
        for a, b in zip(res[r]["window"][:len(params)], total):
            np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-5, atol=1e-6)
        # used in one micro-batch of the window: kept, summed over ranks (1 + 2)
        assert torch.equal(res[r]["window"][-2], torch.full((3,), 3.0))
        assert res[r]["mid"][-1] is not None           # views stay attached inside the window
        assert res[r]["window"][-1] is None            # unused in both micro-batches: hidden when the window closes
        assert res[r]["double"], "a second backward inside one reducer cycle must raise"
        assert res[r]["attached"]
        for a, b in zip(res[r]["plain"][:len(params)], first_only):
            np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-5, atol=1e-6)
        assert res[r]["plain"][-1] is None and res[r]["plain"][-2] is None
