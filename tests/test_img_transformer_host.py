"""Host side of the image-region transformer (gloria/models/image_transformer.py) without a GPU: the unfused route is the
stock module bit for bit, the module tree keeps nn.TransformerEncoder's parameter names, `fusable` refuses what the kernels do
not take, and the flat optimizer's shadow set gains the packed input projection and nothing else."""

import pytest
import torch
import torch.nn as nn


def _encoder(E=128, nh=2, layers=2, **kw):
    torch.manual_seed(0)
    return nn.TransformerEncoder(nn.TransformerEncoderLayer(E, nh, **kw), layers, enable_nested_tensor=False).eval()


@pytest.mark.parametrize("with_pos", [False, True])
def test_cpu_run_is_the_stock_module(with_pos):
    from gloria.models import image_transformer as IT
    enc = _encoder()
    B, E, h, w = 3, 128, 3, 5
    x = torch.randn(B, E, h, w).contiguous(memory_format=torch.channels_last)
    table = torch.randn(h, w, E) if with_pos else None
    xin = x if table is None else x + table.permute(2, 0, 1).expand(B, E, h, w)
    want = enc(xin.reshape(B, E, h * w).permute(2, 0, 1)).permute(1, 2, 0).reshape(B, E, h, w)
    got = IT.run(enc, x, None if table is None else table.reshape(h * w, E))
    assert torch.equal(got, want)


def test_fusable_refuses_what_the_kernels_do_not_take():
    from gloria.models import image_transformer as IT
    x = torch.randn(2, 128, 3, 5)
    assert not IT.fusable(_encoder(), x)                                                    # CPU tensors
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert not IT.fusable(_encoder(), x)
    # the layer checks, without a device: everything but the tensor's placement
    assert IT._layer_ok(_encoder(256, 4).layers[0], 256)
    assert not IT._layer_ok(_encoder(256, 4, norm_first=True).layers[0], 256)
    assert not IT._layer_ok(_encoder(256, 4, activation="gelu").layers[0], 256)
    assert not IT._layer_ok(_encoder(320, 5).layers[0], 320)                                # 64-wide heads, E not a kernel size
    assert not IT._layer_ok(_encoder(256, 8).layers[0], 256)                                # 32-wide heads
    assert not IT._layer_ok(_encoder(256, 4, dim_feedforward=300).layers[0], 256)
    assert not IT._layer_ok(_encoder(256, 4, dim_feedforward=8192).layers[0], 256)


@pytest.mark.gpu
def test_fusable_on_the_gpu():
    from gloria.models import image_transformer as IT
    x = torch.randn(2, 256, 3, 5, device="cuda:0")
    enc = _encoder(256, 4).cuda()
    assert not IT.fusable(enc, x)                                                           # fp32 without autocast
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert IT.fusable(enc, x)
        assert not IT.fusable(_encoder(256, 4, norm_first=True).cuda(), x)
        assert not IT.fusable(_encoder(256, 4, activation="gelu").cuda(), x)
        assert not IT.fusable(_encoder(320, 5).cuda(), torch.randn(2, 320, 3, 5, device="cuda:0"))
        assert not IT.fusable(nn.TransformerEncoder(enc.layers[0], 1, norm=nn.LayerNorm(256).cuda()), x)
    with torch.autocast("cuda", dtype=torch.float16):
        assert not IT.fusable(enc, x)


def _gloria(transformer):
    from gloria.config import pretrain_config
    from gloria.models.gloria_model import GLoRIA
    cfg = pretrain_config("imagenome", batch_size=2)
    cfg.set_path("model.text.bert_config", dict(vocab_size=1000, num_hidden_layers=1))
    if transformer:
        cfg.set_path("model.image_transformer", dict(num_heads=12, num_layers=2))
        cfg.set_path("model.image_position_embeddings", dict(num=19))
    return GLoRIA(cfg)


def test_state_dict_keeps_the_reference_names():
    model = _gloria(True)
    stock = nn.TransformerEncoder(nn.TransformerEncoderLayer(768, 12), 2, enable_nested_tensor=False).state_dict()
    mine = {k[len("image_transformer."):]: v for k, v in model.state_dict().items() if k.startswith("image_transformer.")}
    assert set(mine) == set(stock)
    assert all(mine[k].shape == stock[k].shape and mine[k].dtype == stock[k].dtype for k in stock)
    assert "position_embeddings.image_position_embeddings.weight" in model.state_dict()


def test_shadow_parameters_gain_the_packed_input_projection_only():
    from gloria.optim import shadow_parameter_ids
    enc = _encoder(256, 4, layers=2)
    ids = shadow_parameter_ids(enc)
    for layer in enc.layers:
        assert id(layer.self_attn.in_proj_weight) in ids and id(layer.self_attn.in_proj_bias) in ids
        assert id(layer.norm1.weight) not in ids and id(layer.norm2.bias) not in ids
    names = {n for n, p in enc.named_parameters() if id(p) in ids}
    assert names == {n for n, _ in enc.named_parameters() if ".norm" not in n}
    # the default model has no MultiheadAttention: the set is what it was, the direct parameters of Linear / Conv2d modules
    model = _gloria(False)
    want = {id(p) for m in model.modules() if isinstance(m, (nn.Linear, nn.Conv2d)) for p in m.parameters(recurse=False)}
    assert shadow_parameter_ids(model) == want
