"""gloria.optim.ShadowAdam(accumulate=k): windows of k micro-batches summed into the fp32 flat accumulators by
glr_accum_mt, one guarded clip + Adam step per window - against torch.optim.Adam + clip_grad_norm_ fed the ordered fp32
reference sum, inside the bands tests/test_gpu_train.py uses for the same norm / Adam kernels."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _toy(seed=0):
    torch.manual_seed(seed)
    m = torch.nn.Sequential()
    m.emb = torch.nn.Embedding(50, 24, padding_idx=0)
    m.conv = torch.nn.Conv2d(3, 8, 3, padding=1, bias=False)
    m.bn = torch.nn.BatchNorm2d(8)
    m.fc1 = torch.nn.Linear(24, 40)
    m.ln = torch.nn.LayerNorm(40)
    m.fc2 = torch.nn.Linear(40, 7)
    m.free = torch.nn.Parameter(torch.randn(13))
    m = m.to(DEV)
    m.conv.to(memory_format=torch.channels_last)
    return m


def _flat_opt(model, **kw):
    from gloria.optim import ShadowAdam, shadow_parameter_ids
    return ShadowAdam(list(model.parameters()), lr=1e-2, betas=(0.5, 0.999), weight_decay=1e-3, max_grad_norm=0.25,
                      shadow_ids=shadow_parameter_ids(model), **kw)


def _ref_opt(model):
    return torch.optim.Adam(list(model.parameters()), lr=1e-2, betas=(0.5, 0.999), weight_decay=1e-3)


def _hand_grads(params, gen, mag, poison=None):
    """a seeded gradient per parameter in the parameter's dtype and strides (what autograd hands over); returns the
    values as fp32"""
    vals = []
    for i, p in enumerate(params):
        grad = (torch.randn(p.shape, device=DEV, generator=gen) * mag).to(p.dtype)
        if poison is not None and i == poison[0]:
            grad.view(-1)[poison[1]] = float("nan")
        p.grad = torch.empty_strided(p.shape, p.stride(), dtype=p.dtype, device=DEV).copy_(grad)
        vals.append(grad.float())
    return vals


def _state(opt):
    out = [opt.record.clone()]
    for g in opt.groups:
        out += [g.master.clone(), g.exp_avg.clone(), g.exp_avg_sq.clone()]
        if g.shadow_buf is not None:
            out.append(g.shadow_buf.clone())
    return out


def _same(a, b):
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


def _accumulate(opt, scale, first, buckets):
    if not buckets:
        opt.accumulate(scale, first)
        return
    for grp in opt.groups:                 # as the data-parallel reducer does: bucket by bucket
        half = len(grp.params) // 2
        grp.accumulate(0, half, scale, first)
        grp.accumulate(half, len(grp.params), scale, first)


def _acc_views(opt, params):
    where = {id(p): (g, i) for g in opt.groups for i, p in enumerate(g.params)}
    return [where[id(p)][0].view(where[id(p)][0].grad, where[id(p)][1]) for p in params]


def _compare(opt, ref, pa, pb, norm):
    np.testing.assert_allclose(float(opt.clip_state[0]), float(norm), rtol=1e-5)
    for p, q in zip(pa, pb):
        m = opt.master_of(p)
        np.testing.assert_allclose(m.cpu().numpy(), q.detach().cpu().numpy(), rtol=2e-5, atol=1e-7)
        if p.dtype == torch.bfloat16:
            assert torch.equal(p.detach(), m.to(torch.bfloat16))
        np.testing.assert_allclose(opt.state[p]["exp_avg"].cpu().numpy(), ref.state[q]["exp_avg"].cpu().numpy(),
                                   rtol=2e-5, atol=1e-8)
        np.testing.assert_allclose(opt.state[p]["exp_avg_sq"].cpu().numpy(), ref.state[q]["exp_avg_sq"].cpu().numpy(),
                                   rtol=2e-5, atol=1e-10)


def _ref_step(ref, pb, sums):
    for q, s in zip(pb, sums):
        q.grad = s.contiguous(memory_format=torch.channels_last) if q.dim() == 4 else s.clone()
    norm = torch.nn.utils.clip_grad_norm_(pb, 0.25)
    ref.step()
    return norm


@pytest.mark.parametrize("k,buckets", [(2, False), (4, False), (2, True)], ids=["k2", "k4", "k2-buckets"])
def test_windows_match_torch_adam_on_the_reference_sum(k, buckets):
    a, b = _toy(), _toy()
    pa, pb = list(a.parameters()), list(b.parameters())
    opt, ref = _flat_opt(a, accumulate=k, flat_grads=buckets), _ref_opt(b)
    assert a.fc1.weight.dtype == torch.bfloat16 and a.emb.weight.dtype == torch.float32
    assert all(g.grad is not None and g.grad.dtype == torch.float32 for g in opt.groups)      # fp32 in the shadow group too
    assert {g.sdt for g in opt.groups} == {torch.bfloat16, torch.float32}
    gen = torch.Generator(DEV).manual_seed(1)
    s = torch.tensor(1.0 / k, dtype=torch.float32, device=DEV)        # a power of two: s * g is exact
    n = 0
    for w in range(3):
        sums, before = None, _state(opt)
        for j in range(k):
            vals = _hand_grads(pa, gen, 0.3 if n % 2 else 3.0)
            n += 1
            sums = [s * v for v in vals] if j == 0 else [t + s * v for t, v in zip(sums, vals)]
            _accumulate(opt, 1.0 / k, j == 0, buckets)
            assert all(p.grad is None for p in pa)                    # released after the launch
            assert _same(_state(opt), before), "nothing but the accumulator changes inside a window"
        for got, want in zip(_acc_views(opt, pa), sums):
            assert torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))   # bit for bit
        norm = _ref_step(ref, pb, sums)
        opt.step()
        assert opt.calls == w + 1 and opt.t == w + 1
        _compare(opt, ref, pa, pb, norm)


def test_window_with_a_nan_is_skipped_whole_and_located():
    from gloria import nonfinite as NF
    k = 2
    a, b = _toy(), _toy()
    pa, pb = list(a.parameters()), list(b.parameters())
    opt, ref = _flat_opt(a, accumulate=k), _ref_opt(b)
    bad_param = next(i for i, p in enumerate(pa) if p is a.fc1.weight)
    gen = torch.Generator(DEV).manual_seed(2)
    s = torch.tensor(0.5, dtype=torch.float32, device=DEV)
    for w in range(3):
        before = _state(opt)
        sums = None
        for j in range(k):
            poison = (bad_param, 5) if (w, j) == (1, 0) else None      # the FIRST micro-batch: the NaN must survive the add
            vals = _hand_grads(pa, gen, 3.0, poison)
            sums = [s * v for v in vals] if j == 0 else [t + s * v for t, v in zip(sums, vals)]
            opt.accumulate(0.5, j == 0)
        opt.step()
        rec = opt.record.tolist()
        if w == 1:
            after = _state(opt)
            assert _same(after[1:], before[1:]), "a skipped window changes nothing"
            assert rec[NF.SKIPPED] == 1 and rec[NF.APPLIED] == 1 and rec[NF.LAST_CALL] == 2 and rec[NF.LAST_COUNT] == 1
            p, e = opt.locate(rec[NF.LAST_PARTIAL], rec[NF.LAST_OFFSET])
            assert p is a.fc1.weight and e == 5
            continue
        norm = _ref_step(ref, pb, sums)
        assert rec[NF.SKIPPED] == (1 if w == 2 else 0) and rec[NF.APPLIED] == (2 if w == 2 else 1)
        _compare(opt, ref, pa, pb, norm)          # the third window applies as Adam's step 2
    assert opt.calls == 3 and opt.t == 2


def test_accumulate_1_is_the_optimizer_as_it_was():
    from gloria.optim import ShadowAdam
    a, b = _toy(), _toy()
    pa, pb = list(a.parameters()), list(b.parameters())
    oa, ob = _flat_opt(a), _flat_opt(b, accumulate=1)
    for o in (oa, ob):
        assert o.accum == 1 and not o.flat_grads and all(g.grad is None for g in o.groups)    # no accumulator
        assert all(g.gdt == g.sdt for g in o.groups)
    with pytest.raises(RuntimeError):
        ob.accumulate(1.0, True)
    for bad in (0, -2, 2.5):
        with pytest.raises(ValueError):
            ShadowAdam(list(_toy().parameters()), lr=1e-2, accumulate=bad)
    for step in range(2):
        ga, gb = torch.Generator(DEV).manual_seed(30 + step), torch.Generator(DEV).manual_seed(30 + step)
        oa.zero_grad()
        ob.zero_grad()
        _hand_grads(pa, ga, 3.0)
        _hand_grads(pb, gb, 3.0)
        oa.step()
        ob.step()
    assert oa.t == ob.t == 2
    for p, q in zip(pa, pb):
        assert torch.equal(oa.master_of(p), ob.master_of(q)) and torch.equal(p.detach(), q.detach())
    # data-parallel form: the bf16 bucket stays bf16
    oc = _flat_opt(_toy(), flat_grads=True)
    assert {g.grad.dtype for g in oc.groups} == {torch.bfloat16, torch.float32}
