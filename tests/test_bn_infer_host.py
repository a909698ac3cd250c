"""Eval-mode BatchNorm entry points (glr_bn_infer / glr_bn_relu_maxpool3s2_infer, include/glr.h) without a device: the
ABI lists them, bad arguments are refused with GLR_EINVAL before any HIP call (the pointers are made-up non-NULL
addresses that nothing may dereference), and on CPU tensors the host layer is torch's own operators, exactly."""

import ctypes

import torch

EINVAL = -1            # include/glr.h
FAKE = 0x10000         # a non-NULL address: the calls below must return before using it
BF16 = 1


def test_infer_symbols_are_exported_and_listed():
    from gloria import _native as N
    handle = ctypes.CDLL(N.LIB_PATH)
    for name in ("glr_bn_infer", "glr_bn_relu_maxpool3s2_infer"):
        assert name in N.SYMBOLS, name
        assert hasattr(handle, name), name
    assert N.lib().glr_version() == 3


def test_bn_infer_refuses_bad_arguments_before_a_launch():
    from gloria import _native as N
    Lb = N.lib()

    def call(x=FAKE, C=64, R=100, y=FAKE, gamma=FAKE, var=FAKE):
        return Lb.glr_bn_infer(x, None, gamma, FAKE, FAKE, var, R, C, 1e-5, 1, y, BF16, None)

    assert call(x=None) == EINVAL
    assert call(C=24) == EINVAL                          # not a power of two
    assert call(R=0) == EINVAL
    assert call(y=None) == EINVAL
    assert call(gamma=None) == EINVAL
    assert call(var=None) == EINVAL
    assert call(C=4) == EINVAL and call(C=4096) == EINVAL


def test_stem_infer_refuses_bad_arguments_before_a_launch():
    from gloria import _native as N
    Lb = N.lib()

    def call(x=FAKE, C=64, H=5, W=5, B=1, y=FAKE, mean=FAKE):
        return Lb.glr_bn_relu_maxpool3s2_infer(x, FAKE, FAKE, mean, FAKE, B, H, W, C, 1e-5, y, None)

    assert call(C=12) == EINVAL
    assert call(H=0) == EINVAL
    assert call(W=0) == EINVAL and call(B=0) == EINVAL
    assert call(x=None) == EINVAL and call(y=None) == EINVAL and call(mean=None) == EINVAL


def _bn(c, g):
    bn = torch.nn.BatchNorm2d(c).eval()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g) * 0.2)
        bn.running_mean.copy_(torch.randn(c, generator=g) * 0.5)
        bn.running_var.copy_(torch.rand(c, generator=g) * 2 + 0.05)
    return bn


def test_cpu_tensors_take_torch_in_eval_mode():
    from gloria.models import fused_bn as FB
    g = torch.Generator().manual_seed(0)
    bn = _bn(16, g)
    x = torch.randn(2, 16, 5, 7, generator=g).contiguous(memory_format=torch.channels_last)
    r = torch.randn(2, 16, 5, 7, generator=g).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        y = FB.fused_bn_act(bn, x, r, True, fork=True)
        assert isinstance(y, torch.Tensor)
        assert torch.equal(y, torch.relu(bn(x) + r))
        assert torch.equal(FB.fused_bn_act(bn, x, relu=False), bn(x))


def test_cpu_stem_takes_torch():
    from gloria.models import fused_bn as FB
    g = torch.Generator().manual_seed(1)
    bn = _bn(8, g)
    pool = torch.nn.MaxPool2d(3, stride=2, padding=1)
    x = torch.randn(2, 8, 6, 7, generator=g).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        assert torch.equal(FB.fused_stem(bn, pool, x), pool(torch.relu(bn(x))))
        xb = x.bfloat16()
        assert torch.equal(FB.fused_stem(bn, pool, xb), pool(torch.relu(bn(xb))))
    bn.train()                                             # training mode goes the same way
    y = FB.fused_stem(bn, pool, x)
    assert y.shape == (2, 8, 3, 4) and y.requires_grad


def test_eval_switch_is_a_module_attribute():
    from gloria.models import fused_bn as FB
    assert isinstance(FB.EVAL_ENABLED, bool) and isinstance(FB.ENABLED, bool)
