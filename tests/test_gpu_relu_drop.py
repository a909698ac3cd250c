"""glr_relu_drop_fwd / _bwd (csrc/glr_ffn.hip: a = dropout(relu(z)) of the image-region transformer's feed-forward middle)
through the C ABI: outputs bit for bit against the formulas of include/glr.h with the kernel's OWN bits decoded from their
layout (element 4 (l + 64 i) + c of a row = bit l of word 4 i + c), the column sums against an fp64 sum of the kernel's own
dz with the worst-case bound of an fp32 summation, and the mask as a pure function of (key, row, column)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(5, 256, 0.5), (97, 2048, 0.1), (1000, 2048, 0.0), (130, 1024, 0.25), (722, 2048, 0.1)]


def _decode(words, R, C):
    """uint64 words [R, C/64] -> bool [R, C]"""
    w = words.cpu().numpy().view(np.uint64).reshape(R, C // 64)
    lanes = np.arange(64, dtype=np.uint64)
    bits = ((w[:, :, None] >> lanes[None, None, :]) & np.uint64(1)).astype(bool)       # [R, word, lane]
    out = np.zeros((R, C), dtype=bool)
    for word in range(C // 64):
        i, c = word // 4, word % 4
        out[:, 4 * (np.arange(64) + 64 * i) + c] = bits[:, word, :]
    return torch.from_numpy(out)


def _scale(p):
    """s = 1.0f / (1.0f - p) in fp32, as the host side of the kernels computes it"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def _fwd(z, p, seed=1234, off=8, cell=None, want_bits=True):
    from gloria import _native as N
    R, C = z.shape
    a = torch.full_like(z, 7.0)
    alive = torch.zeros(R, C // 64, dtype=torch.int64, device=DEV) if want_bits else None
    N.check(N.lib().glr_relu_drop_fwd(N.ptr(z), R, C, p, seed, off, N.ptr(cell), N.ptr(a), N.ptr(alive), N.stream()), "fwd")
    return a, alive


def _bwd(dy, alive, p, mode):
    """mode: None = no column sums, 0 = fp32, 1 = bf16"""
    from gloria import _native as N
    L = N.lib()
    R, C = dy.shape
    dz = torch.full_like(dy, 7.0)
    n_ws = L.glr_ffn_workspace_floats(R, C)
    assert n_ws > 0
    ws = torch.empty(n_ws, device=DEV)
    out = None if mode is None else torch.empty(C, device=DEV, dtype=torch.bfloat16 if mode else torch.float32)
    N.check(L.glr_relu_drop_bwd(N.ptr(dy), N.ptr(alive), R, C, p, N.ptr(dz), N.ptr(ws), N.ptr(out), int(bool(mode)), N.stream()),
            "bwd")
    return dz, out


def _inputs(R, C):
    g = torch.Generator().manual_seed(R * 7 + C)
    z = (torch.randn(R, C, generator=g) * 1.3).to(DEV).bfloat16()
    dy = torch.randn(R, C, generator=g).to(DEV).bfloat16()
    return z, dy


@pytest.mark.parametrize("R,C,p", CASES)
def test_forward_matches_spec(R, C, p):
    z, _ = _inputs(R, C)
    z[0, :8] = 0.0                                            # zeros (and -0) are not alive
    z[0, 8:16] = -0.0
    a, alive = _fwd(z, p)
    bits = _decode(alive, R, C).to(DEV)
    assert not (bits & ~(z > 0)).any()                        # alive is a subset of z > 0
    want = torch.where(bits, (z.float().clamp_min(0) * _scale(p)).bfloat16(), torch.zeros_like(z))
    assert torch.equal(a.view(torch.int16), want.view(torch.int16))
    if p == 0:
        assert torch.equal(bits, z > 0)                       # ReLU bits only
        a0, _ = _fwd(z, 0.0, want_bits=False)                 # the no-grad call: nothing but a is written
        assert torch.equal(a0.view(torch.int16), a.view(torch.int16))
    # keep rate on an all-positive z: every bit is a dropout bit
    zp = z.abs() + 1.0
    _, ap = _fwd(zp, p)
    frac = _decode(ap, R, C).float().mean().item()
    sigma = (p * (1 - p) / (R * C)) ** 0.5
    print("keep rate R=%d C=%d p=%g: %.6f (bound %.6f)" % (R, C, p, frac - (1 - p), 5 * sigma + 1e-3))
    assert abs(frac - (1 - p)) < 5 * sigma + 1e-3, (frac, 1 - p)


@pytest.mark.parametrize("R,C,p", CASES)
def test_backward_matches_spec(R, C, p):
    z, dy = _inputs(R, C)
    _, alive = _fwd(z, p)
    bits = _decode(alive, R, C).to(DEV)
    dz, s32 = _bwd(dy, alive, p, 0)
    want = torch.where(bits, (dy.float() * _scale(p)).bfloat16(), torch.zeros_like(dy))
    assert torch.equal(dz.view(torch.int16), want.view(torch.int16))
    dz_b, s16 = _bwd(dy, alive, p, 1)
    dz_c, _ = _bwd(dy, alive, p, None)
    assert torch.equal(dz_b.view(torch.int16), dz.view(torch.int16)) and torch.equal(dz_c.view(torch.int16), dz.view(torch.int16))
    # column sums of the ROUNDED dz: any fp32 summation order of R terms is within R 2^-24 sum |term| of the exact sum
    ref = dz.double().sum(0)
    bound = R * 2.0 ** -24 * dz.double().abs().sum(0)
    err32 = (s32.double() - ref).abs()
    err16 = (s16.double() - ref).abs()
    print("dzsum R=%d C=%d p=%g: max err/bound fp32 %.3g bf16 %.3g" % (
        R, C, p, float((err32 / bound.clamp_min(1e-30)).max()), float((err16 / (bound + 2.0 ** -8 * ref.abs()).clamp_min(1e-30)).max())))
    assert (err32 <= bound).all()
    assert (err16 <= bound + 2.0 ** -8 * ref.abs()).all()
    # two identical calls are bit-equal
    dz2, s32b = _bwd(dy, alive, p, 0)
    assert torch.equal(dz2.view(torch.int16), dz.view(torch.int16)) and torch.equal(s32b.view(torch.int32), s32.view(torch.int32))


def test_mask_is_a_function_of_key_row_and_column():
    R, C, p = 200, 2048, 0.1
    z = (torch.randn(R, C, device=DEV).abs() + 0.5).bfloat16()
    a, m = _fwd(z, p, 7, 0)
    a2, m2 = _fwd(z, p, 7, 0)
    assert torch.equal(m, m2) and torch.equal(a.view(torch.int16), a2.view(torch.int16))
    _, mc = _fwd(z, p, 7, 4)
    _, md = _fwd(z, p, 8, 0)
    assert not torch.equal(m, mc) and not torch.equal(m, md)
    # not a function of R or the launch geometry: the first 64 rows of the 200-row call are the 64-row call
    a64, m64 = _fwd(z[:64].contiguous(), p, 7, 0)
    assert torch.equal(m[:64], m64) and torch.equal(a[:64].view(torch.int16), a64.view(torch.int16))
    # key from a device cell {seed, offset base} (+ the site offset passed by value)
    cell = torch.tensor([7, 0], dtype=torch.int64, device=DEV)
    _, me = _fwd(z, p, 123, 0, cell)
    cell.copy_(torch.tensor([7, 4], dtype=torch.int64))
    _, mf = _fwd(z, p, 0, 0, cell)
    cell.copy_(torch.tensor([7, 0], dtype=torch.int64))
    _, mg = _fwd(z, p, 0, 4, cell)
    assert torch.equal(me, m) and torch.equal(mf, mc) and torch.equal(mg, mc)


def test_bad_shapes_are_refused_without_a_launch():
    from gloria import _native as N
    L = N.lib()
    z = torch.zeros(4, 8192, device=DEV, dtype=torch.bfloat16)
    a = torch.full_like(z, 7.0)
    alive = torch.zeros(4, 128, dtype=torch.int64, device=DEV)
    ws = torch.empty(1 << 16, device=DEV)
    out = torch.full((8192,), 7.0, device=DEV)
    for C in (192, 8192):
        assert L.glr_ffn_workspace_floats(4, C) == 0
        assert L.glr_relu_drop_fwd(N.ptr(z), 4, C, 0.1, 1, 0, None, N.ptr(a), N.ptr(alive), N.stream()) == -1     # GLR_EINVAL
        assert L.glr_relu_drop_bwd(N.ptr(z), N.ptr(alive), 4, C, 0.1, N.ptr(a), N.ptr(ws), N.ptr(out), 0, N.stream()) == -1
    assert L.glr_relu_drop_fwd(N.ptr(z), 4, 256, 0.1, 1, 0, None, N.ptr(a), None, N.stream()) == -1   # dropout needs the bits
    assert L.glr_relu_drop_fwd(N.ptr(z), 0, 256, 0.0, 1, 0, None, N.ptr(a), None, N.stream()) == -1
    torch.cuda.synchronize()
    assert bool((a == 7.0).all()) and bool((out == 7.0).all()) and bool((alive == 0).all())           # nothing was written
