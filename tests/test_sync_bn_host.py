"""Global-batch BatchNorm on the fused kernels (gloria/models/fused_bn.py: GlobalBatchNorm2d, Trainer(sync_bn="fused"))
without a device: the module conversion, the refusal to compute per-rank statistics, the entry points' argument checks
(made-up non-NULL addresses that nothing may dereference) and the Trainer switch, under a 2-rank gloo group where a
process group is needed."""

import copy
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

EINVAL, EDTYPE = -1, -2   # include/glr.h
FAKE = 0x10000            # a non-NULL address: the calls below must return before using it
F32, BF16 = 0, 1


class _Ctx:
    """what convert_global_batchnorm reads of a DistContext"""
    rank, world_size = 1, 2

    def all_gather_nograd(self, x):
        return torch.cat([x, x], 0)


def test_convert_replaces_the_53_sites_and_shares_state():
    from gloria.models import cnn_backbones as CB, fused_bn as FB
    model, _, _ = CB.resnet_50(pretrained=False)
    plain = [m for m in model.modules() if type(m) is torch.nn.BatchNorm2d]
    assert len(plain) == 53
    keys = list(model.state_dict().keys())
    before = {n: t for n, t in list(model.named_parameters()) + list(model.named_buffers())}
    out = FB.convert_global_batchnorm(model, _Ctx())
    assert out is model
    conv = [m for m in model.modules() if type(m) is FB.GlobalBatchNorm2d]
    assert len(conv) == 53 and not [m for m in model.modules() if type(m) is torch.nn.BatchNorm2d]
    assert list(model.state_dict().keys()) == keys
    after = {n: t for n, t in list(model.named_parameters()) + list(model.named_buffers())}
    assert before.keys() == after.keys() and all(after[n] is before[n] for n in before)      # the same objects
    for old, new in zip(plain, conv):
        assert (new.num_features, new.eps, new.momentum, new.training) == (old.num_features, old.eps, old.momentum, old.training)
        assert new.weight is old.weight and new.running_var is old.running_var
        assert new.num_batches_tracked is old.num_batches_tracked
        assert new.rank == 1 and callable(new.gather)
    v = torch.arange(5, dtype=torch.float64)
    assert conv[0].gather(v).shape == (2, 5)                         # [n] -> [P, n]
    assert type(copy.deepcopy(conv[0])) is FB.GlobalBatchNorm2d


def test_convert_leaves_other_norm_classes():
    from gloria.models import fused_bn as FB
    sbn = torch.nn.SyncBatchNorm(8)
    net = torch.nn.Sequential(torch.nn.BatchNorm2d(8), sbn, torch.nn.BatchNorm1d(8), torch.nn.GroupNorm(2, 8))
    FB.convert_global_batchnorm(net, _Ctx())
    assert [type(m) for m in net] == [FB.GlobalBatchNorm2d, torch.nn.SyncBatchNorm, torch.nn.BatchNorm1d, torch.nn.GroupNorm]
    assert net[1] is sbn
    single = FB.convert_global_batchnorm(torch.nn.BatchNorm2d(8), _Ctx())      # the root itself
    assert type(single) is FB.GlobalBatchNorm2d


def test_training_mode_on_cpu_raises_and_eval_is_batchnorm():
    from gloria.models import fused_bn as FB
    g = torch.Generator().manual_seed(0)
    bn = torch.nn.BatchNorm2d(16)
    gbn = FB.convert_global_batchnorm(copy.deepcopy(bn), _Ctx())
    x = torch.randn(2, 16, 5, 7, generator=g).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="global-batch"):
        FB.fused_bn_act(gbn.train(), x)
    with pytest.raises(RuntimeError, match="global-batch"):
        gbn(x)                                                       # the module call takes the same road
    assert int(gbn.num_batches_tracked) == 0 and torch.equal(gbn.running_mean, torch.zeros(16))
    gbn.eval(), bn.eval()
    with torch.no_grad():
        assert torch.equal(FB.fused_bn_act(gbn, x), torch.relu(bn(x)))
        assert torch.equal(gbn(x), bn(x))
    xg = x.clone().requires_grad_(True)                              # eval mode with a graph to record: torch's
    FB.fused_bn_act(gbn, xg, relu=False).sum().backward()
    assert xg.grad is not None


def test_sync_entry_points_refuse_bad_arguments_before_a_launch():
    from gloria import _native as N
    Lb = N.lib()

    def pf(x=FAKE, R=10, C=64, ws=FAKE, rec=FAKE, dt=BF16):
        return Lb.glr_bn_sync_partial_fwd(x, R, C, ws, rec, dt, None)
    assert pf(x=None) == EINVAL and pf(ws=None) == EINVAL and pf(rec=None) == EINVAL
    assert pf(R=0) == EINVAL and pf(C=24) == EINVAL and pf(C=4) == EINVAL and pf(C=4096) == EINVAL
    assert pf(dt=7) == EDTYPE

    def af(x=FAKE, recs=FAKE, P=2, R=10, C=64, mean=FAKE, count=FAKE, y=FAKE, dt=F32):
        return Lb.glr_bn_sync_apply_fwd(x, None, FAKE, FAKE, recs, P, R, C, 1e-5, 0.1, 1, None, None, None, mean, FAKE, count,
                                        y, dt, None)
    assert af(x=None) == EINVAL and af(recs=None) == EINVAL and af(P=0) == EINVAL and af(mean=None) == EINVAL
    assert af(count=None) == EINVAL and af(y=None) == EINVAL and af(C=48) == EINVAL and af(R=-1) == EINVAL
    assert af(dt=2) == EDTYPE

    def pb(x=FAKE, dy=FAKE, dy2=None, y=None, R=10, C=64, res=0, rec=FAKE, dres=None, dt=BF16):
        return Lb.glr_bn_sync_partial_bwd(x, dy, dy2, y, FAKE, FAKE, FAKE, FAKE, R, C, 1, res, FAKE, rec, dres, dt, None)
    assert pb(x=None) == EINVAL and pb(dy=None) == EINVAL and pb(rec=None) == EINVAL and pb(C=12) == EINVAL
    assert pb(res=1) == EINVAL and pb(res=1, y=FAKE) == EINVAL and pb(res=1, dres=FAKE) == EINVAL      # y AND dres
    assert pb(dy2=FAKE) == EINVAL                                    # a second gradient only with a residual
    assert pb(dt=-1) == EDTYPE

    def ab(x=FAKE, dz=FAKE, recs=FAKE, P=2, rank=0, count=FAKE, R=10, C=64, out=FAKE, dx=FAKE, dt=BF16):
        return Lb.glr_bn_sync_apply_bwd(x, dz, FAKE, FAKE, FAKE, FAKE, recs, P, rank, count, R, C, 1, 0, out, dx, dt, None)
    assert ab(x=None) == EINVAL and ab(dz=None) == EINVAL and ab(recs=None) == EINVAL and ab(count=None) == EINVAL
    assert ab(P=0) == EINVAL and ab(rank=2) == EINVAL and ab(rank=-1) == EINVAL and ab(out=None) == EINVAL
    assert ab(dx=None) == EINVAL and ab(R=0) == EINVAL and ab(C=2049) == EINVAL
    assert ab(dt=3) == EDTYPE


def test_trainer_fused_mode_keeps_the_image_graph_off(monkeypatch):
    from gloria.config import pretrain_config
    from gloria.models import fused_bn as FB
    from gloria.trainer import Trainer
    cfg = pretrain_config("imagenome", batch_size=4)
    monkeypatch.setattr(FB, "ENABLED", True)
    tr = Trainer(cfg, device="cpu", sync_bn="fused", graph_image_encoder=True)
    assert tr.graph_image_encoder is False and tr.sync_bn is True and tr.sync_bn_fused is True
    assert Trainer(cfg, device="cpu", sync_bn="fused").graph_image_encoder is False
    plain = Trainer(cfg, device="cpu")
    assert plain.sync_bn is False and plain.sync_bn_fused is False and plain.graph_image_encoder is None
    old = Trainer(cfg, device="cpu", sync_bn=True)
    assert old.sync_bn is True and old.sync_bn_fused is False and old.graph_image_encoder is False
    with pytest.raises(ValueError):
        Trainer(cfg, device="cpu", sync_bn="global")


def test_trainer_fused_mode_without_kernels_is_sync_batchnorm(monkeypatch, capsys):
    from gloria.config import pretrain_config
    from gloria.models import fused_bn as FB
    from gloria.trainer import Trainer
    monkeypatch.setattr(FB, "ENABLED", False)                        # GLR_FUSED_BN=0
    tr = Trainer(pretrain_config("imagenome", batch_size=4), device="cpu", sync_bn="fused")
    assert tr.sync_bn is True and tr.sync_bn_fused is False and tr.graph_image_encoder is False
    out = capsys.readouterr().out
    assert "SyncBatchNorm" in out and len(out.strip().splitlines()) == 1


class _Stub(torch.nn.Module):
    """what Trainer.setup touches of the lightning model, with a three-layer image encoder"""

    def __init__(self):
        super().__init__()
        self.gloria = torch.nn.Module()
        self.gloria.img_encoder = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 1), torch.nn.BatchNorm2d(8), torch.nn.ReLU())

    def configure_optimizers(self):
        return {"optimizer": torch.optim.SGD(self.parameters(), lr=0.1), "lr_scheduler": None}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2")
    os.environ.pop("GLR_FORCE_DIST", None)
    dist.init_process_group("gloo", rank=rank, world_size=2)
    try:
        from gloria.config import pretrain_config
        from gloria.dist import DistContext
        from gloria.models import fused_bn as FB
        from gloria.trainer import Trainer
        FB.ENABLED = True
        res = {}
        for mode in (True, "fused", False):
            model = _Stub()
            keys = list(model.state_dict().keys())
            bn = model.gloria.img_encoder[1]
            tr = Trainer(pretrain_config("imagenome", batch_size=4), device="cpu", precision=32, dist_ctx=DistContext(),
                         sync_bn=mode, flat_optimizer=False)
            tr.setup(model)
            new = model.gloria.img_encoder[1]
            ent = {"type": type(new).__name__, "keys": list(model.state_dict().keys()) == keys,
                   "shared": new.weight is bn.weight and new.running_mean is bn.running_mean,
                   "in_optimizer": any(p is new.weight for p in tr.params)}
            if mode == "fused":
                rec = torch.full((3,), float(rank), dtype=torch.float64)
                ent["gathered"] = new.gather(rec).tolist()           # DistContext.all_gather_nograd over gloo
                ent["rank"] = new.rank
            res[str(mode)] = ent
        torch.save(res, os.path.join(out, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_trainer_modes_under_a_two_rank_gloo_group(tmp_path):
    """sync_bn=True is still torch's SyncBatchNorm conversion; "fused" converts to GlobalBatchNorm2d whose gather is the
    group's all-gather in rank order; the default converts nothing"""
    mp.spawn(_worker, args=(_free_port(), str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        res = torch.load(tmp_path / f"r{r}.pt", weights_only=False)
        assert res["True"]["type"] == "SyncBatchNorm" and res["True"]["keys"]
        assert res["False"]["type"] == "BatchNorm2d" and res["False"]["shared"]
        f = res["fused"]
        assert f["type"] == "GlobalBatchNorm2d" and f["keys"] and f["shared"] and f["in_optimizer"]
        assert f["rank"] == r and f["gathered"] == [[0.0] * 3, [1.0] * 3]
