"""glr_accum_mt through the C ABI: the gradient-accumulation kernel that adds one micro-batch's gradients (bf16 or fp32,
one tensor per parameter, named by a pointer table) into the fp32 flat accumulator of gloria.optim._Group.

Layout as _Group builds it: parameters padded to 8 elements, chunks of 16384.  The sizes cover a tail-only chunk (1, 7),
a vector-only chunk (8, 2048), a chunk tail after vectors (13, 2049), the second trip of a thread's loop (> 2048
elements per chunk), and several chunks per parameter (16397: a 13-element last chunk; 49152: three full ones).  One
parameter has no gradient (a null pointer)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CHUNK = 16384
SIZES = [1, 7, 8, 13, 2048, 21, 2049, 16384, 16397, 49152]
NULL = 5                      # position of the parameter without a gradient
SENTINEL = 12345.0
TAIL = 64                     # accumulator elements past the last parameter
EINVAL, EDTYPE = -1, -2
REC = 24                      # bytes per chunk-table entry


class _Layout:
    def __init__(self):
        self.offsets, off = [], 0
        for n in SIZES:
            self.offsets.append(off)
            off += (n + 7) // 8 * 8
        self.n = off
        ent, self.chunk_start = [], []
        for i, (n, o) in enumerate(zip(SIZES, self.offsets)):
            self.chunk_start.append(len(ent))
            ent += [(i, min(CHUNK, n - c0), c0, o + c0) for c0 in range(0, n, CHUNK)]
        self.chunk_start.append(len(ent))
        tab = np.zeros(len(ent), dtype=np.dtype([("param", "<i4"), ("count", "<i4"), ("poff", "<i8"), ("foff", "<i8")]))
        for k, e in enumerate(ent):
            tab[k] = e
        self.n_chunks = len(ent)
        self.table = torch.from_numpy(tab.view(np.uint8).copy()).to(DEV)
        self.slot = torch.zeros(self.n + TAIL, dtype=torch.bool)          # elements that belong to a parameter
        for n, o in zip(SIZES, self.offsets):
            self.slot[o:o + n] = True

    def acc(self):
        return torch.full((self.n + TAIL,), SENTINEL, dtype=torch.float32, device=DEV)


@pytest.fixture(scope="module")
def layout():
    return _Layout()


@pytest.fixture(scope="module")
def sources():
    """dtype -> three micro-batches of seeded normal gradients (x3, x0.3, x3), one tensor per parameter; read-only"""
    out = {}
    for dt in (torch.bfloat16, torch.float32):
        g = torch.Generator(DEV).manual_seed(17)
        out[dt] = [[(torch.randn(n, device=DEV, generator=g) * mag).to(dt) for n in SIZES] for mag in (3.0, 0.3, 3.0)]
    return out


def _ptrs(grads, null=NULL):
    return torch.tensor([0 if i == null else t.data_ptr() for i, t in enumerate(grads)], dtype=torch.int64, device=DEV)


def _call(lay, ptrs, dt, acc, scale, first, c0=0, c1=None):
    from gloria import _native as N
    c1 = lay.n_chunks if c1 is None else c1
    code = N.lib().glr_accum_mt(lay.table.data_ptr() + c0 * REC, c1 - c0, N.ptr(ptrs), N.dtype_code(dt), N.ptr(acc),
                                scale, first, N.stream())
    torch.cuda.synchronize()
    return code


def _flat(lay, grads, fn):
    """fn(gradient of parameter i as a CPU tensor) laid out in the accumulator's order (zeros elsewhere)"""
    out = torch.zeros(lay.n + TAIL, dtype=torch.float64)
    for i, (t, o) in enumerate(zip(grads, lay.offsets)):
        if i != NULL:
            out[o:o + t.numel()] = fn(t.cpu())
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("scale", [1.0, 0.5, 1.0 / 3.0], ids=["1", "0.5", "third"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_three_calls(layout, sources, dt, scale):
    lay, (g1, g2, g3) = layout, sources[dt]
    acc = lay.acc()
    real = lay.slot.clone()
    o, n = lay.offsets[NULL], SIZES[NULL]
    real[o:o + n] = False                               # slots of parameters WITH a gradient

    def untouched(a):
        rest = a[~lay.slot]
        assert rest.numel() > TAIL and bool((rest == SENTINEL).all()), "padding or the tail past the last chunk written"

    # call 1: first - every slot written with scale * g, one rounding; the null parameter's slot zeroed
    assert _call(lay, _ptrs(g1), dt, acc, scale, 1) == 0
    a = acc.cpu()
    untouched(a)
    assert bool((_bits(a[o:o + n]) == 0).all()), "first: the slot of a parameter without a gradient must be +0"
    s32 = float(np.float32(scale))                      # what the kernel is handed
    want = (_flat(lay, g1, lambda t: t.double()) * s32).float()      # fp32 x fp32 is exact in fp64: one rounding
    assert torch.equal(_bits(a[real]), _bits(want[real]))
    acc[o:o + n] = 7.0                                  # marker: calls 2 and 3 must leave this slot alone

    # calls 2 and 3: fmaf(scale, g, acc)
    assert _call(lay, _ptrs(g2), dt, acc, scale, 0) == 0
    a2 = acc.cpu()
    assert _call(lay, _ptrs(g3), dt, acc, scale, 0) == 0
    a3 = acc.cpu()
    for a in (a2, a3):
        untouched(a)
        assert bool((a[o:o + n] == 7.0).all()), "a parameter without a gradient keeps its slot"
    f = [_flat(lay, g, lambda t: t.double()) for g in (g1, g2, g3)]
    if scale in (1.0, 0.5):
        # a power-of-two scale commutes with rounding: torch's fp32 sums in the kernel's order, bit for bit
        s = torch.tensor(scale, dtype=torch.float32)
        p = [s * x.float() for x in f]
        assert torch.equal(_bits(a2[real]), _bits((p[0] + p[1])[real]))
        assert torch.equal(_bits(a3[real]), _bits(((p[0] + p[1]) + p[2])[real]))
    # three roundings of at most half an ulp of a partial sum (|partial| <= sum |g| / 3 x scale x 3), one of slack
    ref = scale * (f[0] + f[1] + f[2])
    bound = 4 * 2.0 ** -24 * (f[0].abs() + f[1].abs() + f[2].abs()) * scale
    err = (a3.double() - ref).abs()
    worst = float((err[real] / bound[real].clamp_min(1e-300)).max())
    print(f"accum {dt} scale {scale}: max err / bound = {worst:.3f}")
    assert bool((err[real] <= bound[real]).all())


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_sub_range_of_the_table(layout, sources, dt):
    """(chunk_table + c0, c1 - c0), as the data-parallel reducer calls it for one bucket: only that range is written"""
    lay, g1 = layout, sources[dt][0]
    i0, i1 = 4, 9                                       # includes the null parameter and the 2-chunk one
    c0, c1 = lay.chunk_start[i0], lay.chunk_start[i1]
    acc = lay.acc()
    assert _call(lay, _ptrs(g1), dt, acc, 0.5, 1, c0, c1) == 0
    a = acc.cpu()
    inside = torch.zeros_like(lay.slot)
    for i in range(i0, i1):
        inside[lay.offsets[i]:lay.offsets[i] + SIZES[i]] = True
    assert bool((a[~inside] == SENTINEL).all())
    want = (_flat(lay, g1, lambda t: t.double()) * 0.5).float()
    assert torch.equal(_bits(a[inside]), _bits(want[inside]))
    # and an added micro-batch on the same range
    assert _call(lay, _ptrs(g1), dt, acc, 0.5, 0, c0, c1) == 0
    a = acc.cpu()
    assert bool((a[~inside] == SENTINEL).all())
    assert torch.equal(_bits(a[inside]), _bits((want + want)[inside]))


def test_bad_arguments_launch_nothing(layout, sources):
    from gloria import _native as N
    lay, g1 = layout, sources[torch.float32][0]
    acc, ptrs = lay.acc(), _ptrs(g1)
    L, st = N.lib(), N.stream()
    tab, n = lay.table.data_ptr(), lay.n_chunks
    f32 = N.dtype_code(torch.float32)
    assert L.glr_accum_mt(None, n, N.ptr(ptrs), f32, N.ptr(acc), 1.0, 1, st) == EINVAL
    assert L.glr_accum_mt(tab, n, None, f32, N.ptr(acc), 1.0, 1, st) == EINVAL
    assert L.glr_accum_mt(tab, n, N.ptr(ptrs), f32, None, 1.0, 1, st) == EINVAL
    assert L.glr_accum_mt(tab, 0, N.ptr(ptrs), f32, N.ptr(acc), 1.0, 1, st) == EINVAL
    assert L.glr_accum_mt(tab, -3, N.ptr(ptrs), f32, N.ptr(acc), 1.0, 1, st) == EINVAL
    for bad in (float("inf"), -float("inf"), float("nan")):
        assert L.glr_accum_mt(tab, n, N.ptr(ptrs), f32, N.ptr(acc), bad, 1, st) == EINVAL
    assert L.glr_accum_mt(tab, n, N.ptr(ptrs), 7, N.ptr(acc), 1.0, 1, st) == EDTYPE
    torch.cuda.synchronize()
    assert bool((acc == SENTINEL).all())
