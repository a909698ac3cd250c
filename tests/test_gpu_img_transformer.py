"""The image-region transformer on the HIP path (gloria/models/image_transformer.py) against an fp64 CPU copy of the same
nn.TransformerEncoder: per tensor (output, every parameter gradient, the input gradient) the relative Frobenius error of the
fused path must be at most twice that of torch's own autocast path on the same inputs - both round to bf16 at the GEMM
boundaries, the factor 2 allows for the different places of the remaining roundings.  Plus dropout reproducibility, the
kernels a layer issues, the no-grad call and one Trainer step of the configuration."""

import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL = dict(E=256, nh=4, ff=512, layers=2, B=3, h=3, w=5)          # 15 regions: the short attention kernel
REGIONS = dict(E=768, nh=12, ff=2048, layers=1, B=2, h=19, w=19)     # 361 regions: both attention routes


def _set_dropout(enc, p):
    for l in enc.layers:
        l.dropout.p = l.dropout1.p = l.dropout2.p = p
        l.self_attn.dropout = p


def _models(E, nh, ff, layers, p=0.0, seed=0):
    """(fp64 CPU encoder, GPU encoder with the flat optimizer's dtypes: bf16 Linears / in_proj, fp32 LayerNorms) holding
    the same bf16-representable values"""
    from gloria.optim import shadow_parameter_ids
    torch.manual_seed(seed)
    enc = nn.TransformerEncoder(nn.TransformerEncoderLayer(E, nh, dim_feedforward=ff), layers, enable_nested_tensor=False)
    _set_dropout(enc, p)
    shadows = shadow_parameter_ids(enc)
    with torch.no_grad():
        for q in enc.parameters():
            if q.dim() == 1:                                  # biases and LayerNorm weights off their 0 / 1 init
                q.add_(torch.randn_like(q) * 0.1)
            if id(q) in shadows:
                q.copy_(q.bfloat16().float())
    ref = copy.deepcopy(enc).double().train()
    gpu = copy.deepcopy(enc).to(DEV).train()
    for (_, q), (_, q0) in zip(gpu.named_parameters(), enc.named_parameters()):
        if id(q0) in shadows:
            q.data = q.data.bfloat16()
    return ref, gpu


def _inputs(E, B, h, w, with_pos, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, E, h, w, generator=g).bfloat16()
    proj = torch.randn(B, E, h, w, generator=g)
    table = (torch.randn(h * w, E, generator=g) * 0.5) if with_pos else None
    return x, proj, table


def _grads(enc, x, proj, table, dev, dtype, fused):
    """output and gradients of sum(out * proj) through image_transformer.run: {name: fp64 CPU tensor}"""
    from gloria.models import image_transformer as IT
    IT.ENABLED = fused
    wide = torch.float64 if dtype == torch.float64 else torch.float32
    try:
        xin = x.to(dev, dtype).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        pos = None if table is None else table.to(dev, wide).requires_grad_(True)
        enc.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dev != "cpu"):
            assert IT.fusable(enc, xin) == (fused and dev != "cpu")
            out = IT.run(enc, xin, pos)
        (out.to(wide) * proj.to(dev, wide)).sum().backward()
        res = {"output": out, "input.grad": xin.grad}
        if pos is not None:
            res["image_position_embeddings.grad"] = pos.grad
        for n, q in enc.named_parameters():
            res[n + ".grad"] = q.grad
        return {k: v.detach().double().cpu() for k, v in res.items()}
    finally:
        IT.ENABLED = True


def _parity(tag, shape, with_pos, attn=None):
    from gloria.models import image_transformer as IT
    ref_enc, gpu_enc = _models(shape["E"], shape["nh"], shape["ff"], shape["layers"])
    x, proj, table = _inputs(shape["E"], shape["B"], shape["h"], shape["w"], with_pos)
    keep = IT.ATTN
    if attn is not None:
        IT.ATTN = attn
    try:
        want = _grads(ref_enc, x, proj.double(), table, "cpu", torch.float64, False)
        fused = _grads(gpu_enc, x, proj, table, DEV, torch.bfloat16, True)
        stock = _grads(gpu_enc, x, proj, table, DEV, torch.bfloat16, False)
    finally:
        IT.ATTN = keep
    assert set(want) == set(fused) == set(stock)
    worst = []
    for k in sorted(want):
        nrm = float(want[k].norm())
        ef, es = float((fused[k] - want[k]).norm()) / nrm, float((stock[k] - want[k]).norm()) / nrm
        print("[img_tx %s] %-48s fused %.3e  stock %.3e  ratio %.3f" % (tag, k, ef, es, ef / es))
        if not ef <= 2.0 * es:
            worst.append((k, ef, es))
    assert not worst, worst


def test_parity_short_kernel():
    _parity("15 regions", SMALL, False)


@pytest.mark.parametrize("attn", ["kernel", "sdpa"])
def test_parity_361_regions(attn):
    _parity("361 regions " + attn, REGIONS, False, attn)


def test_parity_with_position_embeddings():
    _parity("15 regions + pos", SMALL, True)
    _parity("361 regions + pos", REGIONS, True)


def test_dropout_is_reproducible_under_manual_seed():
    from gloria.models import image_transformer as IT
    _, enc = _models(SMALL["E"], SMALL["nh"], SMALL["ff"], SMALL["layers"], p=0.1)
    x, proj, _ = _inputs(SMALL["E"], SMALL["B"], SMALL["h"], SMALL["w"], False)

    def once(seed):
        torch.manual_seed(seed)
        return _grads(enc, x, proj, None, DEV, torch.bfloat16, True)
    a, b, c = once(3), once(3), once(4)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["output"], c["output"])
    assert all(bool(torch.isfinite(v).all()) for v in a.values())
    assert IT.ENABLED


def test_kernels_of_one_fused_layer(monkeypatch):
    """one fused layer forward issues glr_relu_drop_fwd once and glr_drop_add_ln_fwd twice; the stock path none"""
    from gloria import _native as N
    from gloria.models import image_transformer as IT
    _, enc = _models(SMALL["E"], SMALL["nh"], SMALL["ff"], 1, p=0.1)
    x = _inputs(SMALL["E"], SMALL["B"], SMALL["h"], SMALL["w"], False)[0].to(DEV).contiguous(memory_format=torch.channels_last)
    names, real = [], N.check

    def check(code, what):
        names.append(what)
        return real(code, what)
    monkeypatch.setattr(N, "check", check)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = IT.run(enc, x)
    assert names.count("glr_relu_drop_fwd") == 1 and names.count("glr_drop_add_ln_fwd") == 2, names
    assert out.dtype == torch.float32 and out.shape == x.shape and out.is_contiguous(memory_format=torch.channels_last)
    del names[:]
    monkeypatch.setattr(IT, "ENABLED", False)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        IT.run(enc, x)
    assert names == []


def test_no_grad_eval_call_keeps_no_bits(monkeypatch):
    from gloria.models import image_transformer as IT
    _, enc = _models(SMALL["E"], SMALL["nh"], SMALL["ff"], SMALL["layers"], p=0.1)
    x = _inputs(SMALL["E"], SMALL["B"], SMALL["h"], SMALL["w"], False)[0].to(DEV).contiguous(memory_format=torch.channels_last)
    made, real = [], IT._alive_words

    def alive_words(R, C, dev):
        made.append((R, C))
        return real(R, C, dev)
    monkeypatch.setattr(IT, "_alive_words", alive_words)
    enc.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        assert IT.fusable(enc, x)
        quiet = IT.run(enc, x)
    assert made == []
    enc.train()
    _set_dropout(enc, 0.0)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loud = IT.run(enc, x.clone().requires_grad_(True))
    assert len(made) == SMALL["layers"]
    # the same kernels on the same values; the GEMMs in between are the library's (one bf16 ulp of the operands at most)
    rel = float((quiet - loud.detach()).norm() / loud.detach().norm())
    print("[img_tx] eval / no_grad vs train p = 0: relative difference %.3e" % rel)
    assert rel <= 2.0 ** -8


def test_local_loss_on_fp32_embeddings_under_autocast():
    """the transformer hands the loss fp32 image embeddings, the text encoder fp32 words: the fp32 loss kernels run, and
    autocast around the call must not change their operands (the gram GEMM stays fp32)"""
    from gloria.loss import gloria_loss as gl
    g = torch.Generator().manual_seed(2)
    img = (torch.randn(4, 768, 19, 19, generator=g) * 0.5).to(DEV).contiguous(memory_format=torch.channels_last)
    words = (torch.randn(4, 768, 9, generator=g) * 0.5).to(DEV)
    cap_lens = [9, 5, 2, 1]

    def losses(autocast):
        a, b = img.clone().requires_grad_(True), words.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            l0, l1 = gl.local_loss(a, b, cap_lens)[:2]
        (l0 + l1).backward()
        return torch.stack([l0.detach(), l1.detach()]).cpu(), a.grad.cpu(), b.grad.cpu()
    plain, inside = losses(False), losses(True)
    for p, q in zip(plain, inside):
        np.testing.assert_allclose(q.numpy(), p.numpy(), rtol=1e-5, atol=1e-6)


def _trainer_cfg(B):
    from gloria.config import pretrain_config
    cfg = pretrain_config("imagenome", batch_size=B)
    cfg.set_path("model.text.bert_config", dict(vocab_size=28996, num_hidden_layers=2, hidden_dropout_prob=0.0,
                                                attention_probs_dropout_prob=0.0))
    cfg.set_path("lightning.trainer.precision", 16)
    cfg.set_path("model.image_transformer", dict(num_heads=12, num_layers=1))
    cfg.set_path("model.image_position_embeddings", dict(num=19))
    return cfg


def _one_step(fused, p, seed=5):
    from gloria import builder
    from gloria.datasets.synthetic import make_batch
    from gloria.models import image_transformer as IT
    from gloria.trainer import Trainer
    B = 4
    cfg = _trainer_cfg(B)
    torch.manual_seed(seed)
    model = builder.build_lightning_model(cfg, builder.build_data_module(cfg))
    if p is not None:
        _set_dropout(model.gloria.image_transformer, p)
    tr = Trainer(cfg, device="cuda:0", flat_optimizer=True, graph_text_encoder=False)
    tr.setup(model)
    assert tr.flat
    model.train()
    watched = {n: q for n, q in model.gloria.named_parameters() if n.startswith(("image_transformer.", "position_embeddings."))}
    before = {n: tr.optimizer.master_of(q).clone() for n, q in watched.items()}
    IT.ENABLED = fused
    try:
        loss = float(tr.training_step(model, make_batch(B, seed=9), 0))
    finally:
        IT.ENABLED = True
    changed = {n: not torch.equal(before[n], tr.optimizer.master_of(q)) for n, q in watched.items()}
    return loss, changed, model


def test_trainer_step_updates_the_transformer():
    loss, changed, model = _one_step(True, None)
    assert np.isfinite(loss)
    assert len(changed) == 12 + 1 and all(changed.values()), changed
    assert model.gloria.image_transformer.layers[0].self_attn.in_proj_weight.dtype == torch.bfloat16


def test_first_step_loss_matches_the_stock_path():
    fused, _, _ = _one_step(True, 0.0)
    stock, _, _ = _one_step(False, 0.0)
    print("[img_tx] first-step loss fused %.6f stock %.6f" % (fused, stock))
    # the bf16 loss band of tests/test_gpu_parity.py (test_bf16_mode_vs_oracle_on_rounded_inputs)
    np.testing.assert_allclose(fused, stock, rtol=2e-2, atol=2e-2)
