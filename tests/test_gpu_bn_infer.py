"""Eval-mode BatchNorm kernels (glr_bn_infer, glr_bn_relu_maxpool3s2_infer; gloria/models/fused_bn.py) on the GPU: each
site against an fp64 evaluation of the BatchNorm formula from the same rounded inputs, the gating of the inference
branch, the one-launch stem against the two-kernel composition (bitwise) and against fp64, the whole image encoder
against its fp32 torch path, and Trainer.evaluate against the CPU model."""

import contextlib
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# Band per element: |y - y64| <= RND[dtype] |y64| + ARITH * M,  M = |x sc| + |mean sc| + |beta| + |r|.
# RND: the ONE rounding of the output: half an ulp of bf16 (8 significand bits) is at most 2^-8 of the value; fp32 outputs
# are not rounded again (their last rounding is one of the arithmetic ones below).
# ARITH: the fp32 path takes at most ~8 roundings of 2^-24 (5.96e-8) relative to the terms of M (var + eps, sqrt, the
# division, mean sc, the subtraction, the fma, the residual add, and the partial results they feed): worst case about
# 4e-7 M, so 1e-6 leaves 2.5x.  An fp32 emulation of the formula on these inputs (CPU) stayed at 0.22 of the band for
# fp32 and at 0.995 of it for bf16: the band is tight, a second rounding to bf16 anywhere fails it.
RND = {torch.bfloat16: 2.0 ** -8, torch.float32: 0.0}
ARITH = 1e-6


def _cl(t, dtype):
    return t.to(DEV).to(dtype).contiguous(memory_format=torch.channels_last)


def _bn(c, g):
    """eval-mode BatchNorm2d with non-trivial affine parameters and running statistics"""
    bn = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g) * 0.2)
        bn.running_mean.copy_(torch.randn(c, generator=g) * 0.5)
        bn.running_var.copy_(torch.rand(c, generator=g) * 2 + 0.05)
        bn.num_batches_tracked.fill_(3)
    return bn.to(DEV).eval()


def _ref64(bn, x, r, relu):
    """(y64, M) on the CPU in fp64 from the rounded inputs: (x - mean) / sqrt(var + eps) * gamma + beta (+ r), relu"""
    v = lambda t: t.detach().double().cpu().view(1, -1, 1, 1)   # noqa: E731
    x64 = x.detach().double().cpu()
    sc = v(bn.weight) / torch.sqrt(v(bn.running_var) + bn.eps)
    y = (x64 - v(bn.running_mean)) / torch.sqrt(v(bn.running_var) + bn.eps) * v(bn.weight) + v(bn.bias)
    M = (x64 * sc).abs() + (v(bn.running_mean) * sc).abs() + v(bn.bias).abs()
    if r is not None:
        y = y + r.detach().double().cpu()
        M = M + r.detach().double().cpu().abs()
    return (torch.relu(y) if relu else y), M


def _check_band(y, y64, M, dtype, what):
    err = (y.detach().double().cpu() - y64).abs()
    band = RND[dtype] * y64.abs() + ARITH * M
    worst = float((err / band).max())
    print(f"[bn infer] {what}: worst error / band = {worst:.3f}")
    assert bool((err <= band).all()), (what, worst)


@contextlib.contextmanager
def _no_torch_bn(monkeypatch):
    """nn.BatchNorm2d.forward raises: whatever runs inside is not the torch fallback"""
    def boom(self, x):
        raise AssertionError("torch BatchNorm2d ran: the fallback, not the kernel")
    with monkeypatch.context() as mp:
        mp.setattr(torch.nn.BatchNorm2d, "forward", boom)
        yield


@contextlib.contextmanager
def _count_torch_bn(monkeypatch):
    calls = []
    orig = torch.nn.BatchNorm2d.forward

    def counted(self, x):
        calls.append(1)
        return orig(self, x)
    with monkeypatch.context() as mp:
        mp.setattr(torch.nn.BatchNorm2d, "forward", counted)
        yield calls


def _bn_buffers(module):
    return {k: v.detach().clone() for k, v in module.named_buffers()
            if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


def _assert_buffers_unchanged(module, before):
    now = dict(module.named_buffers())
    assert before
    for k, v in before.items():
        assert torch.equal(now[k], v), k


# ---------------------------------------------------------------------------------------------- 1. one site
@pytest.mark.parametrize("n,c,h,w", [(5, 8, 7, 5), (3, 64, 5, 5), (2, 256, 19, 19), (2, 2048, 3, 3)])
@pytest.mark.parametrize("residual,relu", [(False, True), (True, True), (False, False)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_bn_infer_matches_fp64(n, c, h, w, residual, relu, dtype, monkeypatch):
    from gloria.models import fused_bn as FB
    monkeypatch.setattr(FB, "ENABLED", True)
    monkeypatch.setattr(FB, "EVAL_ENABLED", True)
    g = torch.Generator().manual_seed(n * 1000 + c)
    bn = _bn(c, g)
    x = _cl(torch.randn(n, c, h, w, generator=g) * 1.5 + 0.3, dtype)
    r = _cl(torch.randn(n, c, h, w, generator=g), dtype) if residual else None
    before = _bn_buffers(bn)
    with torch.no_grad(), _no_torch_bn(monkeypatch):
        y = FB.fused_bn_act(bn, x, r, relu, fork=True)
        y2 = FB.fused_bn_act(bn, x, r, relu)
    assert isinstance(y, torch.Tensor) and y.dtype == dtype and y.shape == x.shape
    assert y.is_contiguous(memory_format=torch.channels_last) and not y.requires_grad
    assert torch.equal(y, y2)
    _assert_buffers_unchanged(bn, before)
    y64, M = _ref64(bn, x, r, relu)
    _check_band(y, y64, M, dtype, f"({n},{c},{h},{w}) res={int(residual)} relu={int(relu)} {dtype}")


# ---------------------------------------------------------------------------------------------- 2. gating
def test_bn_infer_gating(monkeypatch):
    from gloria.models import fused_bn as FB
    monkeypatch.setattr(FB, "ENABLED", True)
    monkeypatch.setattr(FB, "EVAL_ENABLED", True)
    g = torch.Generator().manual_seed(11)
    bn = _bn(64, g)
    x = _cl(torch.randn(3, 64, 6, 5, generator=g), torch.bfloat16)
    r = _cl(torch.randn(3, 64, 6, 5, generator=g), torch.bfloat16)
    # grad enabled, trainable BN parameters: torch's BatchNorm, so that the result carries a graph
    assert bn.weight.requires_grad and torch.is_grad_enabled()
    with _count_torch_bn(monkeypatch) as calls:
        e = FB.fused_bn_act(bn, x)
    assert calls and e.requires_grad
    assert torch.equal(e, torch.relu(bn(x)))
    # grad enabled, but nothing requires grad: the kernel
    bn.requires_grad_(False)
    with _no_torch_bn(monkeypatch):
        k = FB.fused_bn_act(bn, x, r)
    assert not k.requires_grad
    with torch.no_grad():
        kernel = FB.fused_bn_act(bn, x, r)
    assert torch.equal(k, kernel)
    # an input that requires grad: fallback again
    with _count_torch_bn(monkeypatch) as calls:
        FB.fused_bn_act(bn, x.clone().requires_grad_(True))
        FB.fused_bn_act(bn, x, r.clone().requires_grad_(True))
    assert len(calls) == 2
    with torch.no_grad():
        # the switch
        monkeypatch.setattr(FB, "EVAL_ENABLED", False)
        with _count_torch_bn(monkeypatch) as calls:
            off = FB.fused_bn_act(bn, x, r)
        assert len(calls) == 1 and torch.equal(off, torch.relu(bn(x) + r))
        monkeypatch.setattr(FB, "EVAL_ENABLED", True)
        monkeypatch.setattr(FB, "ENABLED", False)           # GLR_FUSED_BN=0 switches everything off
        with _count_torch_bn(monkeypatch) as calls:
            FB.fused_bn_act(bn, x, r)
        assert len(calls) == 1
        monkeypatch.setattr(FB, "ENABLED", True)
        # NCHW input
        xn = x.contiguous()
        assert not xn.is_contiguous(memory_format=torch.channels_last)
        with _count_torch_bn(monkeypatch) as calls:
            yn = FB.fused_bn_act(bn, xn)
        assert len(calls) == 1 and torch.equal(yn, torch.relu(bn(xn)))
        # SyncBatchNorm keeps its own path
        sbn = torch.nn.SyncBatchNorm.convert_sync_batchnorm(torch.nn.BatchNorm2d(64)).to(DEV).eval()
        assert not FB._infer_fusable(sbn, x, None) and FB._infer_fusable(bn, x, None)


# ---------------------------------------------------------------------------------------------- 3. stem
@pytest.mark.parametrize("b,c,h,w", [(2, 64, 5, 5), (1, 8, 6, 7), (1, 64, 1, 1), (1, 64, 2, 2), (1, 64, 150, 150)])
def test_fused_stem_is_the_composition_bitwise_and_matches_fp64(b, c, h, w, monkeypatch):
    from gloria.models import fused_bn as FB
    monkeypatch.setattr(FB, "ENABLED", True)
    monkeypatch.setattr(FB, "EVAL_ENABLED", True)
    g = torch.Generator().manual_seed(b * 100 + c + h)
    bn = _bn(c, g)
    pool = torch.nn.MaxPool2d(3, stride=2, padding=1)
    x = _cl(torch.randn(b, c, h, w, generator=g) * 1.5 + 0.3, torch.bfloat16)
    before = _bn_buffers(bn)

    def boom(*a):
        raise AssertionError("fused_maxpool ran: two launches, not the fused stem")
    with torch.no_grad():
        with _no_torch_bn(monkeypatch), monkeypatch.context() as mp:
            mp.setattr(FB, "fused_maxpool", boom)
            y = FB.fused_stem(bn, pool, x)
        with _no_torch_bn(monkeypatch):
            two = FB.fused_maxpool(pool, FB.fused_bn_act(bn, x))
    assert y.dtype == torch.bfloat16 and y.shape == (b, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1)
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y, two)                                          # (a) bitwise the two-kernel composition
    _assert_buffers_unchanged(bn, before)
    y64, M = _ref64(bn, x, None, True)                                  # (b) fp64, the band of a site max-pooled
    ref = F.max_pool2d(y64, 3, 2, 1)
    err = (y.double().cpu() - ref).abs()
    band = RND[torch.bfloat16] * ref.abs() + ARITH * F.max_pool2d(M, 3, 2, 1)
    print(f"[bn infer] stem ({b},{c},{h},{w}): worst error / band = {float((err / band).max()):.3f}")
    assert bool((err <= band).all())


def test_fused_stem_outside_the_inference_case_is_the_nested_pair(monkeypatch):
    from gloria.models import fused_bn as FB
    monkeypatch.setattr(FB, "ENABLED", True)
    g = torch.Generator().manual_seed(4)
    bn = _bn(64, g)
    pool = torch.nn.MaxPool2d(3, stride=2, padding=1)
    x = _cl(torch.randn(2, 64, 9, 8, generator=g), torch.bfloat16)
    with torch.no_grad():
        monkeypatch.setattr(FB, "EVAL_ENABLED", False)
        assert torch.equal(FB.fused_stem(bn, pool, x), FB.fused_maxpool(pool, torch.relu(bn(x))))
        monkeypatch.setattr(FB, "EVAL_ENABLED", True)
        xf = x.float()                                       # fp32: the site kernel, then torch's pool
        with _no_torch_bn(monkeypatch):
            yf = FB.fused_stem(bn, pool, xf)
        assert yf.dtype == torch.float32 and torch.equal(yf, pool(FB.fused_bn_act(bn, xf)))
    bn.train()                                               # training mode: the training kernels and their backward
    xa = x.clone().requires_grad_(True)
    y = FB.fused_stem(bn, pool, xa)
    assert type(y.grad_fn).__name__ == "_MaxPool3s2Backward"
    y.float().sum().backward()
    assert xa.grad is not None and bool(torch.isfinite(xa.grad.float()).all())


# ---------------------------------------------------------------------------------------------- 4. whole encoder
def _cfg(B, layers=1):
    from gloria.config import pretrain_config
    cfg = pretrain_config("imagenome", batch_size=B)
    cfg.set_path("model.text.bert_config", dict(vocab_size=28996, num_hidden_layers=layers, hidden_dropout_prob=0.0,
                                                attention_probs_dropout_prob=0.0))
    cfg.set_path("lightning.trainer.precision", 32)
    return cfg


def _settle_statistics(encoder, imgs, autocast=False):
    """one train-mode forward with every BatchNorm's momentum 1.0: the running statistics become this batch's"""
    bns = [m for m in encoder.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    keep = [m.momentum for m in bns]
    was = encoder.training
    encoder.train()
    for m in bns:
        m.momentum = 1.0
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        encoder(imgs, get_local=True)
    for m, k in zip(bns, keep):
        m.momentum = k
    encoder.train(was)
    assert float(bns[-1].running_mean.abs().max()) > 0


def test_image_encoder_eval_kernels_no_worse_than_torch_path(monkeypatch):
    from gloria import builder
    from gloria.models import fused_bn as FB
    monkeypatch.setattr(FB, "ENABLED", True)
    monkeypatch.setattr(FB, "EVAL_ENABLED", True)
    # bitwise repeatability below is a statement about the BatchNorm kernels: the library convolutions between them are
    # asked for their deterministic solvers.  (Without this, after the fp32 training-mode pass of _settle_statistics in
    # the same process, two bf16 eval runs differed in 475518 of 739328 local elements by 1 - 3 bf16 ulps; with it the
    # kernel path and torch's eval path both repeat exactly.  The kernels themselves repeat bitwise per site: test 1.)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    import warnings
    torch.manual_seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enc = builder.build_img_model(_cfg(2)).to(DEV).to(memory_format=torch.channels_last)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(8)).to(DEV).contiguous(memory_format=torch.channels_last)
    _settle_statistics(enc, x)
    enc.eval()
    before = _bn_buffers(enc)

    def run(autocast):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            gl, lo = enc(x, get_local=True)
        return gl.float(), lo.float()
    run(True)                                               # settles MIOpen's algorithm choice (the first call searches)
    with _count_torch_bn(monkeypatch) as calls:
        a = run(True)
        a2 = run(True)
    assert not calls                                        # all 53 sites took the kernels
    print(f"[bn infer] encoder repeat: {int((a[0] != a2[0]).sum())} global / {int((a[1] != a2[1]).sum())} local elements differ")
    assert torch.equal(a[0], a2[0]) and torch.equal(a[1], a2[1])
    _assert_buffers_unchanged(enc, before)
    monkeypatch.setattr(FB, "EVAL_ENABLED", False)
    with _count_torch_bn(monkeypatch) as calls:
        b = run(True)
        b2 = run(True)
        c = run(False)
    assert len(calls) == 3 * 53
    print(f"[bn infer] encoder repeat, torch eval path: {int((b[0] != b2[0]).sum())} global / {int((b[1] != b2[1]).sum())} local "
          "elements differ")
    rel = lambda p, q: float((p - q).norm() / q.norm())     # noqa: E731
    for name, i in (("global", 0), ("local", 1)):
        assert a[i].shape == c[i].shape and bool(torch.isfinite(a[i]).all())
        ra, rb = rel(a[i], c[i]), rel(b[i], c[i])
        print(f"[bn infer] encoder {name}: relF(kernels bf16, torch fp32) = {ra:.3e}; relF(torch bf16, torch fp32) = {rb:.3e}; "
              f"relF(kernels bf16, torch bf16) = {rel(a[i], b[i]):.3e}")
        # the kernels round less often than torch's three passes, so they may not be worse than the path they replace;
        # 1.5 covers the differing rounding pattern of two bf16 runs through 50 layers
        assert ra <= 1.5 * rb, (name, ra, rb)


# ---------------------------------------------------------------------------------------------- 5. Trainer.evaluate
@pytest.mark.parametrize("precision", [32, "bf16"])
def test_trainer_evaluate_runs_the_kernels(precision, monkeypatch):
    from gloria import builder
    from gloria.datasets.synthetic import make_batch
    from gloria.models import fused_bn as FB
    from gloria.trainer import Trainer
    from oracle import gloria_oracle as orc
    monkeypatch.setattr(FB, "ENABLED", True)
    monkeypatch.setattr(FB, "EVAL_ENABLED", True)
    B = 4
    cfg = _cfg(B)
    cfg.set_path("lightning.trainer.precision", 32 if precision == 32 else 16)
    torch.manual_seed(13)
    model = builder.build_lightning_model(cfg, builder.build_data_module(cfg))
    trainer = Trainer(cfg, device=DEV, precision=precision)
    trainer.setup(model)
    model.train()
    batches = [make_batch(B, seed=300 + i) for i in range(2)]
    imgs = make_batch(B, seed=299)["imgs"].to(DEV).contiguous(memory_format=torch.channels_last)
    _settle_statistics(model.gloria.img_encoder, imgs, autocast=precision != 32)   # bf16 runs hold bf16 shadow weights
    before = _bn_buffers(model)

    with _count_torch_bn(monkeypatch) as calls:
        gpu = trainer.evaluate(model, batches)
    assert not calls                                        # no BatchNorm fallback
    assert np.isfinite(gpu)
    assert model.training and model.gloria.img_encoder.model.bn1.training
    _assert_buffers_unchanged(model, before)
    if precision != 32:
        return
    monkeypatch.setattr(FB, "EVAL_ENABLED", False)
    off = trainer.evaluate(model, batches)
    cpu_model = copy.deepcopy(model.gloria).cpu().eval()
    tot = 0.0
    with torch.no_grad():
        for b in batches:
            il, ig, tl, tg, sents = cpu_model(b)
            tot += float(orc.calc_loss(il, ig, tl, tg, sents)[0])
    cpu = tot / len(batches)
    print(f"[bn infer] Trainer.evaluate fp32: kernels {gpu:.7f}  torch eval path {off:.7f}  CPU oracle {cpu:.7f}  "
          f"rel {abs(gpu - cpu) / abs(cpu):.2e} / {abs(off - cpu) / abs(cpu):.2e}")
    # the project's figure for a pure forward comparison of the GPU step with the CPU oracle (test_gpu_train.py)
    np.testing.assert_allclose(gpu, cpu, rtol=1e-4)
