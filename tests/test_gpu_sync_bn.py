"""Global-batch BatchNorm on the fused kernels (glr_bn_sync_*, gloria/models/fused_bn.py: GlobalBatchNorm2d) on ONE GPU:
the cross-rank math with a batch split into simulated ranks against torch's BatchNorm2d (+ add) (+ relu) on the FULL
batch, one rank against the per-rank kernels bitwise, the encoder wiring over a single-rank RCCL group, and the guards.
No multi-rank hardware run stands behind this file.

Reference and bands are those of tests/test_gpu_fused_bn.py for the same quantities: fp32 from the same rounded inputs;
y / dres 1e-2 k, dx 2e-2 k, affine gradients atol 2e-2 k after scaling by the reference's largest entry, running mean
rtol 1e-4 / atol 1e-5, running variance rtol 1e-3 / atol 1e-5; k = 1 for bf16, 1e-2 for fp32."""

import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _np(t):
    return t.detach().float().cpu().numpy()


def _cl(t, dtype):
    return t.to(DEV).to(dtype).contiguous(memory_format=torch.channels_last)


def _identity_gather(rec):
    return rec.unsqueeze(0)


def _global_bn(c, g, gather=_identity_gather, rank=0):
    from gloria.models import fused_bn as FB
    bn = FB.GlobalBatchNorm2d(c, gather=gather, rank=rank).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g) * 0.2)
    return bn


def _shared_store_gather(store, rank, P):
    """stand-in for the all-gather of P simulated ranks that run one after the other: the caller's record goes into the
    shared store under (call index, rank); the result is what the store holds for this call so far, zeros elsewhere"""
    calls = [0]

    def gather(rec):
        k = calls[0]
        calls[0] += 1
        store[(k, rank)] = rec.clone()
        return torch.stack([store.get((k, p), torch.zeros_like(rec)) for p in range(P)])
    return gather


def _assert_bands(got, want, k):
    """got / want: dicts of the quantities of the module docstring"""
    np.testing.assert_allclose(_np(got["y"]), _np(want["y"]), rtol=1e-2 * k, atol=1e-2 * k)
    np.testing.assert_allclose(_np(got["dx"]), _np(want["dx"]), rtol=2e-2 * k, atol=2e-2 * k)
    if want.get("dres") is not None:
        np.testing.assert_allclose(_np(got["dres"]), _np(want["dres"]), rtol=1e-2 * k, atol=1e-2 * k)
    for name in ("dgamma", "dbeta"):
        scale = float(want[name].abs().max()) + 1e-6
        np.testing.assert_allclose(_np(got[name]) / scale, _np(want[name]) / scale, atol=2e-2 * k)


def _assert_buffers(bn, ref):
    np.testing.assert_allclose(_np(bn.running_mean), _np(ref.running_mean), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(_np(bn.running_var), _np(ref.running_var), rtol=1e-3, atol=1e-5)
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked)


CASES = [
    # c, (n, h, w), split (images), residual, relu, fork, dtype
    (8, (3, 5, 7), (1, 2), False, True, False, torch.bfloat16),         # one channel group; unequal, odd row counts
    (64, (4, 9, 9), (2, 2), True, True, True, torch.bfloat16),          # skip path, dres, two gradients
    (512, (3, 3, 3), (1, 1, 1), False, False, False, torch.float32),    # two column blocks; P = 3; downsample site
    (2048, (4, 1, 1), (1, 3), True, True, False, torch.bfloat16),       # a rank with a single row
]


@pytest.mark.parametrize("c,nhw,split,residual,relu,fork,dtype", CASES)
def test_simulated_ranks_match_full_batch(c, nhw, split, residual, relu, fork, dtype, monkeypatch):
    """a batch split along N into P simulated ranks, each with its own GlobalBatchNorm2d (copies of one initial state),
    through the autograd function, against torch BatchNorm2d (+ add) (+ relu) on the full batch.  Three passes over the
    chunks share the record store: the first fills the forward records, the second has correct forwards and fills the
    backward records, the third is correct in both directions and is the one judged."""
    from gloria.models import fused_bn as FB
    monkeypatch.setattr(FB, "ENABLED", True)
    n, h, w = nhw
    P = len(split)
    assert sum(split) == n
    k = 1.0 if dtype == torch.bfloat16 else 1e-2
    g = torch.Generator().manual_seed(c * 10 + n)
    # well conditioned: a unit offset whose sign alternates between the images, plus small noise
    sign = torch.tensor([1.0 if i % 2 == 0 else -1.0 for i in range(n)]).view(n, 1, 1, 1)
    x = _cl(sign + 0.3 * torch.randn(n, c, h, w, generator=g), dtype)
    r = _cl(torch.randn(n, c, h, w, generator=g), dtype) if residual else None
    ga = _cl(torch.randn(n, c, h, w, generator=g), dtype)
    gb = _cl(torch.randn(n, c, h, w, generator=g), dtype) if fork else None
    proto = _global_bn(c, g)

    # reference: the full batch in fp32 from the same rounded inputs
    ref = torch.nn.BatchNorm2d(c).to(DEV).train()
    ref.load_state_dict(proto.state_dict())
    xb = x.clone().float().requires_grad_(True)              # clone: .float() of an fp32 tensor is the tensor itself
    rb = None if r is None else r.clone().float().requires_grad_(True)
    z = ref(xb)
    if rb is not None:
        z = z + rb
    yb = torch.relu(z) if relu else z
    yb.backward(ga.float() + (gb.float() if fork else 0.0))
    assert float(x.float().var(dim=(0, 2, 3), unbiased=False).min()) >= 0.25       # the conditioning the bands assume
    want = {"y": yb, "dx": xb.grad, "dres": None if rb is None else rb.grad, "dgamma": ref.weight.grad, "dbeta": ref.bias.grad}

    bounds = np.concatenate([[0], np.cumsum(split)])
    store = {}
    for _ in range(3):
        mods, outs = [], []
        for p in range(P):
            sl = slice(int(bounds[p]), int(bounds[p + 1]))
            bn = copy.deepcopy(proto)
            bn.gather, bn.rank = _shared_store_gather(store, p, P), p
            xa = x[sl].clone().requires_grad_(True)
            ra = None if r is None else r[sl].clone().requires_grad_(True)
            out = FB.fused_bn_act(bn, xa, ra, relu, fork=fork)
            if fork:
                assert isinstance(out, FB.SkipPair) and out.main.data_ptr() == out.skip.data_ptr()
                ya = out.main
                loss = (out.main.float() * ga[sl].float()).sum() + (out.skip.float() * gb[sl].float()).sum()
            else:
                ya = out
                loss = (out.float() * ga[sl].float()).sum()
            assert type(ya.grad_fn).__name__ == "_GlobalBNActBackward"
            assert ya.dtype == dtype and ya.shape == xa.shape
            saved = ya.grad_fn.saved_tensors
            stats, count = saved[4].clone(), saved[5].clone()
            loss.backward()
            mods.append(bn)
            outs.append({"y": ya.detach(), "dx": xa.grad, "dres": None if ra is None else ra.grad, "stats": stats, "count": count})
    got = {"y": torch.cat([o["y"] for o in outs]), "dx": torch.cat([o["dx"] for o in outs]),
           "dres": torch.cat([o["dres"] for o in outs]) if residual else None,
           "dgamma": sum(m.weight.grad for m in mods), "dbeta": sum(m.bias.grad for m in mods)}
    _assert_bands(got, want, k)
    for m, o in zip(mods, outs):
        _assert_buffers(m, ref)
        assert int(m.num_batches_tracked) == 1 and int(o["count"]) == n * h * w
        # every rank forms bitwise the same statistics and buffers from the same records
        assert torch.equal(o["stats"], outs[0]["stats"])
        assert torch.equal(m.running_mean, mods[0].running_mean) and torch.equal(m.running_var, mods[0].running_var)
        assert torch.equal(m.num_batches_tracked, mods[0].num_batches_tracked)
    np.testing.assert_allclose(_np(outs[0]["stats"][0]), _np(xb.detach().mean(dim=(0, 2, 3))), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("c,nhw,residual,relu,fork,dtype", [
    (64, (2, 7, 7), True, True, True, torch.bfloat16),
    (64, (2, 7, 7), True, True, True, torch.float32),
    (256, (2, 4, 4), False, True, False, torch.bfloat16),
])
def test_one_rank_is_the_per_rank_kernel_bitwise(c, nhw, residual, relu, fork, dtype, monkeypatch):
    """GlobalBatchNorm2d with an identity gather (P = 1) against nn.BatchNorm2d on the per-rank kernels: the same
    device functions sum the partials and form the statistics, so everything is equal bit for bit"""
    from gloria.models import fused_bn as FB
    monkeypatch.setattr(FB, "ENABLED", True)
    n, h, w = nhw
    g = torch.Generator().manual_seed(c + n)
    x = _cl(torch.randn(n, c, h, w, generator=g) * 1.5 + 0.3, dtype)
    r = _cl(torch.randn(n, c, h, w, generator=g), dtype) if residual else None
    ga = _cl(torch.randn(n, c, h, w, generator=g), dtype)
    gb = _cl(torch.randn(n, c, h, w, generator=g), dtype) if fork else None
    gbn = _global_bn(c, g)
    bn = torch.nn.BatchNorm2d(c).to(DEV).train()
    bn.load_state_dict(gbn.state_dict())
    res = []
    for mod, node in ((gbn, "_GlobalBNActBackward"), (bn, "_BNActBackward")):
        xa = x.clone().requires_grad_(True)
        ra = None if r is None else r.clone().requires_grad_(True)
        out = FB.fused_bn_act(mod, xa, ra, relu, fork=fork)
        if fork:
            ya = out.main
            loss = (out.main.float() * ga.float()).sum() + (out.skip.float() * gb.float()).sum()
        else:
            ya = out
            loss = (out.float() * ga.float()).sum()
        assert type(ya.grad_fn).__name__ == node
        loss.backward()
        res.append([ya.detach(), xa.grad] + ([ra.grad] if residual else [])
                   + [mod.weight.grad, mod.bias.grad, mod.running_mean, mod.running_var, mod.num_batches_tracked])
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert int(gbn.num_batches_tracked) == 1


def _band_grad(a, b):
    scale = float(b.abs().max()) + 1e-6
    np.testing.assert_allclose(_np(a) / scale, _np(b) / scale, atol=2e-2)


def test_encoder_wiring_with_a_single_rank_group(monkeypatch):
    """convert_global_batchnorm on the image encoder over a single-rank RCCL group (DistContext.all_gather_nograd is the
    gather): all 53 sites take the global-batch entry points in both directions, none the per-rank ones, and the result
    is the unconverted encoder's."""
    import socket
    import warnings
    import torch.distributed as dist
    from gloria import _native as N, builder, dist as gdist
    from gloria.config import pretrain_config
    from gloria.models import fused_bn as FB
    monkeypatch.setattr(FB, "ENABLED", True)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    for k, v in dict(GLR_FORCE_DIST="1", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                     MASTER_PORT=str(port)).items():
        monkeypatch.setenv(k, v)
    torch.manual_seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = builder.build_img_model(pretrain_config("imagenome", batch_size=2)).to(DEV).to(memory_format=torch.channels_last)
    plain.train()
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(4)).to(DEV).contiguous(memory_format=torch.channels_last)
    names = ("glr_bn_sync_partial_fwd", "glr_bn_sync_apply_fwd", "glr_bn_sync_partial_bwd", "glr_bn_sync_apply_bwd",
             "glr_bn_act_fwd", "glr_bn_act_bwd")
    calls = dict.fromkeys(names, 0)
    L = N.lib()

    def counted(name, fn):
        def call(*a):
            calls[name] += 1
            return fn(*a)
        return call
    for name in names:
        monkeypatch.setattr(L, name, counted(name, getattr(L, name)))

    def step(enc):
        enc.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            gl, lo = enc(x, get_local=True)
        (gl.float().sum() + lo.float().sum()).backward()
        return gl.detach().float(), lo.detach().float()

    # the library convolutions' deterministic solvers: at batch 2 two runs of the SAME encoder otherwise differ by more
    # than any band (measured: 0.1 absolute in the global features, 70 % of the largest conv1 gradient entry, first
    # difference at layer1.1.conv1 - bf16 noise through 50 batch-2 BatchNorms), with them they are equal bit for bit
    was_deterministic = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        dctx = gdist.init_from_env("nccl")
        assert dctx.active and dctx.world_size == 1
        step(copy.deepcopy(plain))                           # settles MIOpen's algorithm choice (the first call searches)
        conv = FB.convert_global_batchnorm(copy.deepcopy(plain), dctx)
        assert sum(type(m) is FB.GlobalBatchNorm2d for m in conv.modules()) == 53
        calls.update(dict.fromkeys(names, 0))
        ga, la = step(conv)
        torch.cuda.synchronize()
        assert [calls[nm] for nm in names] == [53, 53, 53, 53, 0, 0], calls
        calls.update(dict.fromkeys(names, 0))
        gb, lb = step(plain)
        assert [calls[nm] for nm in names] == [0, 0, 0, 0, 53, 53], calls
    finally:
        torch.backends.cudnn.deterministic = was_deterministic
        if dist.is_initialized():
            dist.destroy_process_group()
    np.testing.assert_allclose(_np(ga), _np(gb), rtol=1e-2, atol=1e-2)
    np.testing.assert_allclose(_np(la), _np(lb), rtol=1e-2, atol=1e-2)
    _band_grad(conv.model.conv1.weight.grad, plain.model.conv1.weight.grad)
    _band_grad(conv.model.layer3[-1].bn3.weight.grad, plain.model.layer3[-1].bn3.weight.grad)
    pairs = list(zip(conv.model.modules(), plain.model.modules()))
    assert sum(isinstance(b, torch.nn.BatchNorm2d) for _, b in pairs) == 53
    for a, b in pairs:
        if isinstance(b, torch.nn.BatchNorm2d):
            _assert_buffers(a, b)
            assert int(a.num_batches_tracked) == 1


def test_guards(monkeypatch):
    from gloria.models import fused_bn as FB
    monkeypatch.setattr(FB, "ENABLED", True)
    monkeypatch.setattr(FB, "EVAL_ENABLED", True)
    g = torch.Generator().manual_seed(9)
    gbn = _global_bn(64, g)
    x = _cl(torch.randn(2, 64, 6, 5, generator=g), torch.bfloat16)
    # training mode never computes per-rank statistics: NCHW is an error, and nothing was touched
    with pytest.raises(RuntimeError, match="global-batch"):
        FB.fused_bn_act(gbn, x.contiguous())
    with pytest.raises(RuntimeError, match="global-batch"):
        gbn(x.float().contiguous())
    assert int(gbn.num_batches_tracked) == 0
    monkeypatch.setattr(FB, "ENABLED", False)                # GLR_FUSED_BN=0
    with pytest.raises(RuntimeError, match="global-batch"):
        FB.fused_bn_act(gbn, x)
    monkeypatch.setattr(FB, "ENABLED", True)
    # eval mode without a graph: the inference kernel, like nn.BatchNorm2d
    bn = torch.nn.BatchNorm2d(64).to(DEV)
    with torch.no_grad():
        gbn.running_mean.normal_(0, 0.5, generator=None)
        gbn.running_var.uniform_(0.05, 2.05)
    bn.load_state_dict(gbn.state_dict())
    gbn.eval(), bn.eval()
    assert not FB._infer_fusable(gbn, x, None)               # grad enabled and parameters that require it: a graph to record
    with torch.no_grad():
        assert FB._infer_fusable(gbn, x, None) and FB._infer_fusable(bn, x, None)
        assert torch.equal(FB.fused_bn_act(gbn, x), FB.fused_bn_act(bn, x))
    # eval mode with a graph to record: torch's eval-mode batch_norm on the running buffers
    xg = x.clone().requires_grad_(True)
    ye = FB.fused_bn_act(gbn, xg, relu=False)
    assert ye.requires_grad and "BNAct" not in type(ye.grad_fn).__name__
    np.testing.assert_allclose(_np(ye), _np(bn(x)), rtol=1e-2, atol=1e-2)
    # nn.SyncBatchNorm is not this mode's business: the conversion leaves it, and no kernel takes it
    sbn = torch.nn.SyncBatchNorm.convert_sync_batchnorm(torch.nn.BatchNorm2d(64)).to(DEV).train()
    net = torch.nn.Sequential(sbn, torch.nn.BatchNorm2d(64).to(DEV))

    class Ctx:
        rank = 0

        def all_gather_nograd(self, t):
            return t
    FB.convert_global_batchnorm(net, Ctx())
    assert net[0] is sbn and type(net[1]) is FB.GlobalBatchNorm2d
    assert not FB._fusable(sbn, x, None)
    with torch.no_grad():
        assert not FB._infer_fusable(sbn.eval(), x, None)
    assert not FB._fusable(net[1].train(), x, None)           # the per-rank kernels do not take the global-batch class
