"""BatchNorm2d (+ residual add) (+ ReLU) as ONE pair of HBM passes per direction on channels-last bf16 (or fp32) activations
(include/glr.h: glr_bn_act_fwd / glr_bn_act_bwd) for the 53 normalisation sites of the ResNet-50 image encoder
(reference: torchvision's Bottleneck through /root/reference/gloria/models/cnn_backbones.py:31-35).

Same parameters, buffers and state_dict keys as nn.BatchNorm2d: `fused_bn_act` is called WITH the nn.BatchNorm2d
module.  The kernels cover what the training step runs (GPU, channels-last, training mode, power-of-two channel counts;
bf16 under autocast and - since the end of round 3 - fp32, the parity configuration of BASELINE config 1) and what the
readers of images outside it run: eval mode where autograd records nothing (Trainer.evaluate, get_similarities,
zero-shot, retrieval, the localization callbacks: model.eval() under torch.no_grad()) is ONE launch per site with
scale / shift from the running statistics (glr_bn_infer: no statistics pass, no workspace, buffers untouched), and
`fused_stem` folds the stem's BatchNorm + ReLU into the max-pool (glr_bn_relu_maxpool3s2_infer).  Every other case
(eval mode with a graph to record, NCHW, CPU tensors of the host-logic tests) is torch's own BatchNorm + add + relu -
the same operator from the library, not a CPU fallback of the loss path.
Data-parallel runs that want the statistics of the GLOBAL batch on these kernels convert the encoder with
`convert_global_batchnorm` (Trainer(sync_bn="fused")): a `GlobalBatchNorm2d` runs each direction as the rank's own reduce
pass, one all-gather of a 2C+1-double record, and the finish + apply pass on the records of all ranks (glr_bn_sync_*);
in training mode it raises where nn.BatchNorm2d would fall back to torch.  nn.SyncBatchNorm never takes a kernel.
`GLR_FUSED_BN=0` switches all kernels off, `GLR_FUSED_BN_EVAL=0` the inference ones alone (A/B measurements)."""

import os

import torch
import torch.nn.functional as F

from .. import _native as N

ENABLED = os.environ.get("GLR_FUSED_BN", "1") != "0"
EVAL_ENABLED = os.environ.get("GLR_FUSED_BN_EVAL", "1") != "0"     # the eval-mode (inference) kernels; needs ENABLED too

# (device index, stream) -> fp32 workspace for the partial sums.  A workspace is only ever touched by launches of ONE
# stream, so stream order alone makes its reuse safe - also when the two encoders run on two streams.
_WS = {}


_WS_FLOATS = {}     # (rows, channels) -> glr_bn_workspace_floats: one ctypes call per shape, not per launch (host time)


def _workspace(dev, R, c):
    n = _WS_FLOATS.get((R, c))
    if n is None:
        n = _WS_FLOATS[(R, c)] = int(N.lib().glr_bn_workspace_floats(R, c))
    key = (dev.index, N.stream())
    ws = _WS.get(key)
    if ws is None or ws.numel() < n:
        ws = torch.empty(max(n, 1 << 20), dtype=torch.float32, device=dev)
        _WS[key] = ws
    return ws


class _BNAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, weight, bias, run_mean, run_var, nbt, eps, momentum, relu, fork):
        L = N.lib()
        n, c, h, w = x.shape
        R = n * h * w
        dev = x.device
        y = torch.empty_like(x)                              # channels_last like x
        stats = torch.empty(2, c, dtype=torch.float32, device=dev)
        ws = _workspace(dev, R, c)
        N.check(L.glr_bn_act_fwd(N.ptr(x), N.ptr(residual), N.ptr(weight), N.ptr(bias), R, c, float(eps), float(momentum),
                                 1 if relu else 0, N.ptr(run_mean), N.ptr(run_var), N.ptr(nbt), stats.data_ptr(), stats.data_ptr() + 4 * c,
                                 N.ptr(ws), N.ptr(y), N.dtype_code(x.dtype), N.stream()), "glr_bn_act_fwd")
        ctx.save_for_backward(x, y if residual is not None else None, weight, bias, stats)
        ctx.relu, ctx.has_res = bool(relu), residual is not None
        if fork:
            # a second handle on the same storage for the skip consumer of the next block: the two gradients then
            # arrive separately and are added while the backward kernel reads them (autograd would run an add kernel)
            ctx.set_materialize_grads(False)
            return y, y.detach()
        return y

    @staticmethod
    def backward(ctx, dy, dy2=None):
        x, y, weight, bias, stats = ctx.saved_tensors
        if dy is None:
            dy, dy2 = dy2, None
        if dy is None:
            return (None,) * 11
        L = N.lib()
        n, c, h, w = x.shape
        R = n * h * w
        dev = x.device
        if dy.dtype != x.dtype or not dy.is_contiguous(memory_format=torch.channels_last):
            dy = dy.to(x.dtype).contiguous(memory_format=torch.channels_last)
        if dy2 is not None and (dy2.dtype != x.dtype or not dy2.is_contiguous(memory_format=torch.channels_last)):
            dy2 = dy2.to(x.dtype).contiguous(memory_format=torch.channels_last)
        if dy2 is not None and not ctx.has_res:
            dy, dy2 = dy + dy2, None
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if ctx.has_res else None
        out = torch.empty(4, c, dtype=torch.float32, device=dev)
        ws = _workspace(dev, R, c)
        N.check(L.glr_bn_act_bwd(N.ptr(x), N.ptr(dy), N.ptr(dy2), N.ptr(y), N.ptr(weight), N.ptr(bias), stats.data_ptr(), stats.data_ptr() + 4 * c,
                                 R, c, 1 if ctx.relu else 0, 1 if ctx.has_res else 0, N.ptr(ws), N.ptr(out), N.ptr(dx),
                                 N.ptr(dres), N.dtype_code(x.dtype), N.stream()), "glr_bn_act_bwd")
        return dx, dres, out[0], out[1], None, None, None, None, None, None, None


class GlobalBatchNorm2d(torch.nn.BatchNorm2d):
    """nn.BatchNorm2d (same parameters, buffers and state_dict keys) whose training-mode statistics span the GLOBAL batch
    of a data-parallel run, on the fused kernels (glr_bn_sync_*: `_GlobalBNAct`).  Two plain attributes:
      gather  callable, fp64 device vector [n] -> [P, n]: the records of all ranks in rank order (one small all-gather)
      rank    this rank's row of that result
    Training mode runs the kernels or raises - it never computes per-rank statistics; eval mode is nn.BatchNorm2d's."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, device=None, dtype=None,
                 gather=None, rank=0):
        super().__init__(num_features, eps, momentum, affine, track_running_stats, device=device, dtype=dtype)
        self.gather, self.rank = gather, rank

    def forward(self, x):
        if self.training:
            return fused_bn_act(self, x, relu=False)
        return super().forward(x)                            # eval mode: F.batch_norm on the running buffers


def convert_global_batchnorm(module, dist_ctx):
    """Replace every nn.BatchNorm2d of the tree - exactly that class: nn.SyncBatchNorm and others stay - by a
    GlobalBatchNorm2d that SHARES its Parameter and buffer objects (optimizer state, checkpoints and state_dict keys are
    untouched), gathering over `dist_ctx` (gloria.dist.DistContext).  Returns the converted module."""
    def gather(rec):
        return dist_ctx.all_gather_nograd(rec.unsqueeze(0))

    def convert(m):
        if type(m) is torch.nn.BatchNorm2d:
            g = GlobalBatchNorm2d(m.num_features, m.eps, m.momentum, m.affine, m.track_running_stats, device="meta",
                                  gather=gather, rank=dist_ctx.rank)
            g._parameters, g._buffers = m._parameters, m._buffers
            g.training = m.training
            return g
        for name, child in m.named_children():
            new = convert(child)
            if new is not child:
                setattr(m, name, new)
        return m
    return convert(module)


class _GlobalBNAct(torch.autograd.Function):
    """_BNAct with the statistics of the global batch: each direction is the rank's own reduce pass and record, the
    all-gather of the records (`gather`), and the finish + apply pass on the records of all ranks."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, run_mean, run_var, nbt, eps, momentum, relu, fork, gather, rank):
        L = N.lib()
        n, c, h, w = x.shape
        R = n * h * w
        dev = x.device
        code = N.dtype_code(x.dtype)
        y = torch.empty_like(x)                              # channels_last like x
        stats = torch.empty(2, c, dtype=torch.float32, device=dev)
        count = torch.empty((), dtype=torch.int64, device=dev)
        rec = torch.empty(2 * c + 1, dtype=torch.float64, device=dev)
        N.check(L.glr_bn_sync_partial_fwd(N.ptr(x), R, c, N.ptr(_workspace(dev, R, c)), N.ptr(rec), code, N.stream()),
                "glr_bn_sync_partial_fwd")
        recs = _gathered(gather, rec, rank)
        N.check(L.glr_bn_sync_apply_fwd(N.ptr(x), N.ptr(residual), N.ptr(weight), N.ptr(bias), N.ptr(recs), recs.shape[0], R, c,
                                        float(eps), float(momentum), 1 if relu else 0, N.ptr(run_mean), N.ptr(run_var),
                                        N.ptr(nbt), stats.data_ptr(), stats.data_ptr() + 4 * c, N.ptr(count), N.ptr(y), code,
                                        N.stream()), "glr_bn_sync_apply_fwd")
        ctx.save_for_backward(x, y if residual is not None else None, weight, bias, stats, count)
        ctx.relu, ctx.has_res, ctx.gather, ctx.rank = bool(relu), residual is not None, gather, rank
        if fork:
            ctx.set_materialize_grads(False)                 # two handles on one output: see _BNAct
            return y, y.detach()
        return y

    @staticmethod
    def backward(ctx, dy, dy2=None):
        x, y, weight, bias, stats, count = ctx.saved_tensors
        if dy is None:
            dy, dy2 = dy2, None
        if dy is None:
            return (None,) * 13
        L = N.lib()
        n, c, h, w = x.shape
        R = n * h * w
        dev = x.device
        code = N.dtype_code(x.dtype)
        if dy.dtype != x.dtype or not dy.is_contiguous(memory_format=torch.channels_last):
            dy = dy.to(x.dtype).contiguous(memory_format=torch.channels_last)
        if dy2 is not None and (dy2.dtype != x.dtype or not dy2.is_contiguous(memory_format=torch.channels_last)):
            dy2 = dy2.to(x.dtype).contiguous(memory_format=torch.channels_last)
        if dy2 is not None and not ctx.has_res:
            dy, dy2 = dy + dy2, None
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if ctx.has_res else None
        out = torch.empty(4, c, dtype=torch.float32, device=dev)
        rec = torch.empty(2 * c, dtype=torch.float64, device=dev)
        mean, invstd = stats.data_ptr(), stats.data_ptr() + 4 * c
        N.check(L.glr_bn_sync_partial_bwd(N.ptr(x), N.ptr(dy), N.ptr(dy2), N.ptr(y), N.ptr(weight), N.ptr(bias), mean, invstd, R, c,
                                          1 if ctx.relu else 0, 1 if ctx.has_res else 0, N.ptr(_workspace(dev, R, c)),
                                          N.ptr(rec), N.ptr(dres), code, N.stream()), "glr_bn_sync_partial_bwd")
        recs = _gathered(ctx.gather, rec, ctx.rank)
        N.check(L.glr_bn_sync_apply_bwd(N.ptr(x), N.ptr(dres if ctx.has_res else dy), N.ptr(weight), N.ptr(bias), mean, invstd,
                                        N.ptr(recs), recs.shape[0], ctx.rank, N.ptr(count), R, c, 1 if ctx.relu else 0,
                                        1 if ctx.has_res else 0, N.ptr(out), N.ptr(dx), code, N.stream()),
                "glr_bn_sync_apply_bwd")
        return (dx, dres, out[0], out[1]) + (None,) * 9


def _gathered(gather, rec, rank):
    """the records of all ranks, checked before a kernel indexes them: fp64 [P, n] on rec's device, rank < P"""
    recs = gather(rec)
    if (recs.dtype != torch.float64 or recs.dim() != 2 or recs.shape[1] != rec.numel() or recs.device != rec.device
            or not 0 <= rank < recs.shape[0]):
        raise RuntimeError(f"GlobalBatchNorm2d.gather must map an fp64 vector [n] to [P, n] on its device with rank {rank} < P; "
                           f"got {tuple(recs.shape)} {recs.dtype} on {recs.device} for n = {rec.numel()}")
    return recs.contiguous()


def _global_bn_act(bn, x, residual, relu, fork):
    """GlobalBatchNorm2d in training mode: the global-batch kernels, or an error - torch's BatchNorm on this rank's rows
    would quietly be per-rank BatchNorm"""
    if not (bn.momentum is not None and callable(bn.gather) and _tensors_ok(bn, x, residual)):
        raise RuntimeError(
            "GlobalBatchNorm2d (global-batch statistics) runs on the fused kernels only: GLR_FUSED_BN on, a `gather`, "
            "channels-last bf16 / fp32 tensors on the GPU, 8 <= channels <= 2048 a power of two, affine with running "
            f"statistics and momentum; got {tuple(x.shape)} {x.dtype} on {x.device}, "
            f"channels_last={x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)}, GLR_FUSED_BN={int(ENABLED)}")
    fork = bool(fork and residual is not None and torch.is_grad_enabled())
    out = _GlobalBNAct.apply(x, residual, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.eps,
                             bn.momentum, relu, fork, bn.gather, bn.rank)
    return SkipPair(*out) if fork else out


def _operands_ok(bn, x, residual):
    """what the training and the inference kernels both ask of the module and the tensors"""
    # exactly nn.BatchNorm2d: SyncBatchNorm (Trainer(sync_bn=True)) has the same attributes but its statistics span the
    # process group - the per-rank kernels would silently turn the global-batch parity mode into per-rank BN
    return type(bn) is torch.nn.BatchNorm2d and _tensors_ok(bn, x, residual)


def _tensors_ok(bn, x, residual):
    """_operands_ok without the class test (shared with GlobalBatchNorm2d, which has kernels of its own)"""
    c = x.shape[1] if x.dim() == 4 else 0
    return (ENABLED and x.is_cuda and x.dtype in (torch.bfloat16, torch.float32) and x.dim() == 4
            and bn.affine and bn.track_running_stats and 8 <= c <= 2048 and (c & (c - 1)) == 0
            and bn.weight.dtype == torch.float32 and bn.bias.dtype == torch.float32
            and x.is_contiguous(memory_format=torch.channels_last)
            and (residual is None or (residual.dtype == x.dtype and residual.shape == x.shape
                                      and residual.is_contiguous(memory_format=torch.channels_last))))


def _fusable(bn, x, residual):
    return bn.training and bn.momentum is not None and _operands_ok(bn, x, residual)


class SkipPair:
    """(main, skip): two handles on ONE block output - the next block's convolution reads `main`, its skip connection
    `skip` - so that the two gradients reach the producing kernel separately (no autograd add in between)."""
    __slots__ = ("main", "skip")

    def __init__(self, main, skip):
        self.main, self.skip = main, skip


def _infer_fusable(bn, x, residual):
    """eval mode where autograd would record nothing: the one-launch inference kernels (glr_bn_infer) apply.  Eval mode
    WITH a graph to build (grad enabled and x / residual / weight / bias requiring grad) stays torch's: there is no
    backward for the running-statistics form."""
    return (EVAL_ENABLED and not bn.training
            and (_operands_ok(bn, x, residual) or (type(bn) is GlobalBatchNorm2d and _tensors_ok(bn, x, residual)))
            and bn.running_mean.dtype == torch.float32 and bn.running_var.dtype == torch.float32
            and (not torch.is_grad_enabled()
                 or not (x.requires_grad or bn.weight.requires_grad or bn.bias.requires_grad
                         or (residual is not None and residual.requires_grad))))


def _bn_infer(bn, x, residual, relu):
    n, c, h, w = x.shape
    y = torch.empty_like(x)                                  # channels_last like x
    N.check(N.lib().glr_bn_infer(N.ptr(x), N.ptr(residual), N.ptr(bn.weight), N.ptr(bn.bias), N.ptr(bn.running_mean),
                                 N.ptr(bn.running_var), n * h * w, c, float(bn.eps), 1 if relu else 0, N.ptr(y),
                                 N.dtype_code(x.dtype), N.stream()), "glr_bn_infer")
    return y


def fused_bn_act(bn, x, residual=None, relu=True, fork=False):
    """relu?(bn(x) (+ residual)) with nn.BatchNorm2d `bn`'s parameters and running statistics.  fork=True (fused path,
    with a residual, grad enabled): returns a SkipPair instead of a tensor.  A GlobalBatchNorm2d in training mode takes the
    global-batch kernels (or raises); in eval mode it is an nn.BatchNorm2d."""
    if isinstance(bn, GlobalBatchNorm2d) and bn.training:
        return _global_bn_act(bn, x, residual, relu, fork)
    if _fusable(bn, x, residual):
        fork = bool(fork and residual is not None and torch.is_grad_enabled())
        out = _BNAct.apply(x, residual, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.eps,
                           bn.momentum, relu, fork)
        return SkipPair(*out) if fork else out
    if _infer_fusable(bn, x, residual):
        return _bn_infer(bn, x, residual, relu)
    out = bn(x)
    if residual is not None:
        out = out + residual
    return F.relu(out) if relu else out


class _MaxPool3s2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        n, c, h, w = x.shape
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        y = torch.empty((n, c, ho, wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        idx = torch.empty((n, ho, wo, c), dtype=torch.uint8, device=x.device)
        N.check(N.lib().glr_maxpool3s2_fwd(N.ptr(x), n, h, w, c, N.ptr(y), N.ptr(idx), N.stream()), "glr_maxpool3s2_fwd")
        ctx.save_for_backward(idx)
        ctx.shape = (n, c, h, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        n, c, h, w = ctx.shape
        if dy.dtype != torch.bfloat16 or not dy.is_contiguous(memory_format=torch.channels_last):
            dy = dy.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        dx = torch.empty((n, c, h, w), dtype=torch.bfloat16, device=dy.device, memory_format=torch.channels_last)
        N.check(N.lib().glr_maxpool3s2_bwd(N.ptr(dy), N.ptr(idx), n, h, w, c, N.ptr(dx), N.stream()), "glr_maxpool3s2_bwd")
        return dx


def _pool_fusable(pool, x):
    def _is(v, k):
        return v == k or v == (k, k)
    return (ENABLED and x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4 and x.shape[1] % 8 == 0
            and x.is_contiguous(memory_format=torch.channels_last) and _is(pool.kernel_size, 3) and _is(pool.stride, 2)
            and _is(pool.padding, 1) and _is(pool.dilation, 1) and not pool.ceil_mode and not pool.return_indices)


def fused_maxpool(pool, x):
    """nn.MaxPool2d(3, stride=2, padding=1) `pool` on x; channels-last bf16 on the GPU runs the one-byte-argmax kernels."""
    if _pool_fusable(pool, x):
        return _MaxPool3s2.apply(x)
    return pool(x)


def fused_stem(bn, pool, x):
    """pool(relu(bn(x))) of the ResNet stem on the conv1 output x.  Eval mode without autograd on channels-last bf16: ONE
    launch (glr_bn_relu_maxpool3s2_infer; bitwise the two-kernel composition).  Otherwise exactly
    fused_maxpool(pool, fused_bn_act(bn, x))."""
    if _pool_fusable(pool, x) and _infer_fusable(bn, x, None):         # _pool_fusable: bf16 only, like the kernel
        n, c, h, w = x.shape
        y = torch.empty((n, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1), dtype=x.dtype, device=x.device,
                        memory_format=torch.channels_last)
        N.check(N.lib().glr_bn_relu_maxpool3s2_infer(N.ptr(x), N.ptr(bn.weight), N.ptr(bn.bias), N.ptr(bn.running_mean),
                                                     N.ptr(bn.running_var), n, h, w, c, float(bn.eps), N.ptr(y), N.stream()),
                "glr_bn_relu_maxpool3s2_infer")
        return y
    return fused_maxpool(pool, fused_bn_act(bn, x))
