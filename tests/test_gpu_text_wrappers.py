"""The Python wrappers of the text encoder's kernels (gloria/models/fused_attn.py, fused_ln.py, text_model.py, bert.py)
against the entry points they call: the same pointers, leading dimensions, buffer shapes and dropout key give the same
bits, and the generator advances by one draw per dropout site.  The kernels themselves are tested through ctypes elsewhere;
this file pins what stands between a module's forward and the C ABI."""

import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NH, H = 2, 128


def _seed(s):
    """torch.manual_seed(s) -> the (seed, offset) the next dropout site draws"""
    torch.manual_seed(s)
    g = torch.cuda.default_generators[0]
    return g.initial_seed() & 0xFFFFFFFFFFFFFFFF, g.get_offset()


def _offset():
    return torch.cuda.default_generators[0].get_offset()


def _prefix_mask(lengths, L):
    return (torch.arange(L)[None, :] < torch.tensor(lengths)[:, None]).to(DEV)


def _rows(lengths, L):
    from gloria.models.text_rows import PackedRows, plan_rows
    mask = (np.arange(L)[None, :] < np.asarray(lengths)[:, None]).astype(np.int64)
    row_start, row_ids = plan_rows(mask, np.where(mask != 0, 0, -1), 128)
    return PackedRows(row_start, row_ids, len(lengths), L, torch.device(DEV))


# ------------------------------------------------------------------------------------------------ attention
def _attn_direct(name, qkv_ptrs, ld, src, dims, Lp, o_shape, d_o, p, seed, off):
    """`name`_fwd / _bwd on three base pointers of row stride ld.  src: (key mask pointer,) or (row_start pointer, its host
    copy); dims: (B, nh, L) or (B, nh).  Returns o and the gradient: [3, *o_shape] for ld = H, else one [.., 3H] tensor."""
    from gloria import _native as N
    L_ = N.lib()
    o = torch.empty(o_shape, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(dims[0] * NH, Lp, dtype=torch.float32, device=DEV)
    keep = torch.empty(dims[0] * NH, Lp, Lp // 32, dtype=torch.int32, device=DEV) if p > 0 else None
    key = (seed, off) if p > 0 else (0, 0)
    N.check(getattr(L_, name + "_fwd")(*qkv_ptrs, *src, *dims, ld, H, 0.125, p, *key, None, N.ptr(o), N.ptr(lse), N.ptr(keep),
                                       N.stream()), name + "_fwd")
    if ld == H:
        d = torch.empty((3,) + tuple(o_shape), dtype=torch.bfloat16, device=DEV)
        d_ptrs = tuple(N.ptr(t) for t in d)
    else:
        d = torch.empty(tuple(o_shape[:-1]) + (3 * H,), dtype=torch.bfloat16, device=DEV)
        d_ptrs = (d.data_ptr(), d.data_ptr() + 2 * H, d.data_ptr() + 4 * H)
    N.check(getattr(L_, name + "_bwd")(*qkv_ptrs, N.ptr(o), N.ptr(d_o), *src, N.ptr(lse), N.ptr(keep), *dims, ld, H, 0.125, p,
                                       *d_ptrs, N.stream()), name + "_bwd")
    return o, d


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_split_attention_wrapper_equals_the_entry_points(p):
    """self_attention on q, k, v [3, 33, 128] (33 rows: past a 32-row wave edge), ragged prefix masks: o and dq, dk, dv are
    glr_attn_fwd / _bwd's with ld = H on the three tensors and the key drawn from the generator; one draw when p > 0"""
    from gloria import _native as N
    from gloria.models import fused_attn as FA
    B, L = 3, 33
    g = torch.Generator().manual_seed(33)
    q, k, v = (torch.randn(B, L, H, generator=g).bfloat16().to(DEV).requires_grad_(True) for _ in range(3))
    d_o = torch.randn(B, L, H, generator=g).bfloat16().to(DEV)
    key_mask = _prefix_mask([33, 17, 1], L)
    assert FA._fusable(q, k, v, key_mask, NH)
    seed, off = _seed(41)
    o = FA.self_attention(q, k, v, key_mask, NH, p, True)
    assert _offset() - off == (4 if p > 0 else 0)
    o.backward(d_o)
    assert _offset() - off == (4 if p > 0 else 0)
    want_o, want_d = _attn_direct("glr_attn", (N.ptr(q), N.ptr(k), N.ptr(v)), H, (N.ptr(key_mask),), (B, NH, L), 128,
                                  (B, L, H), d_o, p, seed, off)
    assert type(o.grad_fn).__name__.startswith("_SelfAttn")
    assert torch.equal(o, want_o)
    for name, t, w in zip("qkv", (q, k, v), want_d):
        assert torch.equal(t.grad, w) and float(w.float().abs().sum()) > 0, name


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("L", [33, 130])
def test_packed_attention_wrapper_equals_the_entry_points(L, p, monkeypatch):
    """self_attention_packed on [3, L, 384]: base, base + 2H, base + 4H bytes with ld = 3H on both sides; 33 tokens run
    glr_attn_*, 130 (two 128-token blocks) glr_attn_long_* with lse / keep sized by Lp = 256"""
    from gloria.models import fused_attn as FA
    monkeypatch.setattr(FA, "LONG_ENABLED", True)
    B = 3
    g = torch.Generator().manual_seed(L)
    qkv = torch.randn(B, L, 3 * H, generator=g).bfloat16().to(DEV).requires_grad_(True)
    d_o = torch.randn(B, L, H, generator=g).bfloat16().to(DEV)
    key_mask = _prefix_mask([L, L // 2 + 1, 1], L)
    seed, off = _seed(42)
    o = FA.self_attention_packed(qkv, key_mask, NH, p, True)
    assert _offset() - off == (4 if p > 0 else 0)
    o.backward(d_o)
    assert _offset() - off == (4 if p > 0 else 0)
    base = qkv.data_ptr()
    from gloria import _native as N
    want_o, want_d = _attn_direct("glr_attn" if L <= 128 else "glr_attn_long", (base, base + 2 * H, base + 4 * H), 3 * H,
                                  (N.ptr(key_mask),), (B, NH, L), (L + 127) // 128 * 128, (B, L, H), d_o, p, seed, off)
    assert type(o.grad_fn).__name__.startswith("_SelfAttn")
    assert torch.equal(o, want_o)
    assert torch.equal(qkv.grad, want_d) and float(want_d.float().abs().sum()) > 0


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_rows_attention_wrapper_equals_the_entry_points(p):
    """self_attention_rows on the 54 rows of sentences of 1, 33 and 20 tokens (plan of L = 40): glr_attn_rows_fwd / _bwd
    with the plan's row_start on the device and on the host, lse / keep in their padded shapes"""
    from gloria import _native as N
    from gloria.models import fused_attn as FA
    rows = _rows([1, 33, 20], 40)
    T = rows.T
    assert T == 54
    g = torch.Generator().manual_seed(54)
    qkv = torch.randn(T, 3 * H, generator=g).bfloat16().to(DEV).requires_grad_(True)
    d_o = torch.randn(T, H, generator=g).bfloat16().to(DEV)
    seed, off = _seed(43)
    o = FA.self_attention_rows(qkv, rows, NH, p, True)
    assert _offset() - off == (4 if p > 0 else 0)
    o.backward(d_o)
    assert _offset() - off == (4 if p > 0 else 0)
    base = qkv.data_ptr()
    rs = np.ascontiguousarray(rows.row_start_host, dtype=np.int32)
    rs_d = torch.from_numpy(rs).to(DEV)
    want_o, want_d = _attn_direct("glr_attn_rows", (base, base + 2 * H, base + 4 * H), 3 * H, (N.ptr(rs_d), rs.ctypes.data), (3, NH),
                                  128, (T, H), d_o, p, seed, off)
    assert type(o.grad_fn).__name__.startswith("_SelfAttn")
    assert torch.equal(o, want_o)
    assert torch.equal(qkv.grad, want_d) and float(want_d.float().abs().sum()) > 0


# ------------------------------------------------------------------------------------------------ sub-layer epilogue
def _ln_inputs():
    R, Hl = 5, 256
    g = torch.Generator().manual_seed(5)
    h = (torch.randn(R, Hl, generator=g) * 1.3).bfloat16().to(DEV).requires_grad_(True)
    inp = (torch.randn(R, Hl, generator=g) * 0.8 + 0.1).to(DEV).requires_grad_(True)
    ln = torch.nn.LayerNorm(Hl, eps=1e-12).to(DEV)
    with torch.no_grad():
        ln.weight.copy_(torch.rand(Hl, generator=g) + 0.5)
        ln.bias.copy_(torch.randn(Hl, generator=g) * 0.2)
    d32, d16 = torch.randn(R, Hl, generator=g).to(DEV), torch.randn(R, Hl, generator=g).bfloat16().to(DEV)
    row_ids = torch.tensor([7, 2, 300, 0, 41], dtype=torch.int32, device=DEV)
    return h, inp, ln, d32, d16, row_ids


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("with_rows", [False, True])
def test_epilogue_wrapper_equals_the_entry_points(with_rows, p):
    """drop_add_ln on h bf16 / inp fp32 [5, 256], without and with row_ids: y32, y16 and the gradients of h, inp, gamma and
    beta are glr_drop_add_ln_fwd (or _rows_fwd) and _bwd's with the key drawn from the generator"""
    from gloria import _native as N
    from gloria.models import fused_ln as FL
    L_ = N.lib()
    h, inp, ln, d32, d16, row_ids = _ln_inputs()
    R, Hl = h.shape
    ids = row_ids if with_rows else None
    assert FL._fusable(h, inp, ln)
    seed, off = _seed(44)
    y32, y16 = FL.drop_add_ln(h, inp, ln, p, True, row_ids=ids)
    assert _offset() - off == (4 if p > 0 else 0)
    torch.autograd.backward([y32, y16], [d32, d16])
    assert _offset() - off == (4 if p > 0 else 0)
    o32, o16 = torch.empty(R, Hl, device=DEV), torch.empty(R, Hl, device=DEV, dtype=torch.bfloat16)
    st = torch.empty(R, 2, device=DEV)
    m = torch.empty(R, Hl // 64, dtype=torch.int64, device=DEV) if p > 0 else None
    key = (seed, off) if p > 0 else (0, 0)
    if ids is None:
        N.check(L_.glr_drop_add_ln_fwd(N.ptr(h), N.ptr(inp), N.ptr(ln.weight), N.ptr(ln.bias), R, Hl, ln.eps, p, *key, None, N.ptr(o32),
                                       N.ptr(o16), N.ptr(st), N.ptr(m), N.stream()), "glr_drop_add_ln_fwd")
    else:
        N.check(L_.glr_drop_add_ln_rows_fwd(N.ptr(h), N.ptr(inp), N.ptr(ln.weight), N.ptr(ln.bias), N.ptr(ids), R, Hl, ln.eps, p, *key,
                                            None, N.ptr(o32), N.ptr(o16), N.ptr(st), N.ptr(m), N.stream()), "glr_drop_add_ln_rows_fwd")
    d_inp, d_h = torch.empty(R, Hl, device=DEV), torch.empty(R, Hl, device=DEV, dtype=torch.bfloat16)
    dgb = torch.empty(2, Hl, device=DEV)
    ws = torch.empty(L_.glr_ln_workspace_floats(R, Hl), device=DEV)
    N.check(L_.glr_drop_add_ln_bwd(N.ptr(d32), N.ptr(d16), N.ptr(h), N.ptr(inp), N.ptr(ln.weight), N.ptr(st), N.ptr(m), R, Hl, p,
                                   N.ptr(d_inp), N.ptr(d_h), N.ptr(ws), N.ptr(dgb), FL.c_off(dgb, Hl), None, 0, N.stream()),
            "glr_drop_add_ln_bwd")
    assert torch.equal(y32, o32) and torch.equal(y16, o16)
    assert torch.equal(h.grad, d_h) and torch.equal(inp.grad, d_inp)
    assert torch.equal(ln.weight.grad, dgb[0]) and torch.equal(ln.bias.grad, dgb[1])
    assert float(d_h.float().abs().sum()) > 0 and float(dgb.abs().sum()) > 0


def test_row_ids_on_the_unfused_epilogue_are_an_error(monkeypatch):
    """NEW behaviour: with the fused kernels off, a call that carries row_ids raises instead of drawing torch's dropout
    stream in place of the padded path's masks; the same call without row_ids is torch's own operators"""
    from gloria.models import fused_ln as FL
    h, inp, ln, _, _, row_ids = _ln_inputs()
    monkeypatch.setattr(FL, "ENABLED", False)
    y, y16 = FL.drop_add_ln(h, inp, ln, 0.1, True)
    assert y16 is None and y.shape == h.shape
    with pytest.raises(RuntimeError):
        FL.drop_add_ln(h, inp, ln, 0.1, True, row_ids=row_ids)


# ------------------------------------------------------------------------------------------------ K5
def _k5(dst, rows, mean_layers, layers):
    from gloria.models import text_model as TM
    return TM.WordpieceSegSumFn.apply(dst, rows, mean_layers, *layers)


@pytest.mark.parametrize("mean_layers", [False, True])
@pytest.mark.parametrize("packed", [False, True])
def test_k5_wrapper_equals_the_entry_points(packed, mean_layers):
    """WordpieceSegSumFn on two bf16 layers, B = 3, L = 8, D = 48, padded [B, L, D] and on the plan's [T, D] rows: word_emb,
    sent_emb and d_hidden are the four glr_wordpiece_segsum* entry points'"""
    from gloria import _native as N
    L_ = N.lib()
    B, L, D, nl = 3, 8, 48, 2
    lengths = [8, 3, 5]
    dst = np.full((B, L), -1, dtype=np.int32)
    dst[0] = [0, 1, 1, 2, 3, 3, 3, 4]
    dst[1, :3] = [0, 1, 2]
    dst[2, :5] = [0, 0, 1, -1, 2]
    rows = _rows(lengths, L) if packed else None
    g = torch.Generator().manual_seed(48)
    shape = (rows.T, D) if packed else (B, L, D)
    layers = [torch.randn(shape, generator=g).bfloat16().to(DEV).requires_grad_(True) for _ in range(nl)]
    dw, ds = torch.randn(B, D, L, generator=g).to(DEV), torch.randn(B, D, generator=g).to(DEV)
    dst_d = torch.from_numpy(dst).to(DEV)
    word, sent = _k5(dst_d, rows, mean_layers, layers)
    torch.autograd.backward([word, sent], [dw, ds])
    w, s = torch.empty(B, D, L, device=DEV), torch.empty(B, D, device=DEV)
    dh = torch.empty(shape, dtype=torch.bfloat16, device=DEV)
    ptrs = (ctypes.c_void_p * nl)(*[h.data_ptr() for h in layers])
    code, mean = N.dtype_code(torch.bfloat16), int(mean_layers)
    if packed:
        rs = N.ptr(rows.row_start)
        N.check(L_.glr_wordpiece_segsum_rows_fwd(ptrs, nl, code, N.ptr(dst_d), rs, N.ptr(w), N.ptr(s), B, L, D, mean, N.stream()), "fwd")
        N.check(L_.glr_wordpiece_segsum_rows_bwd(N.ptr(dw), N.ptr(ds), N.ptr(dst_d), rs, N.ptr(dh), code, B, L, D, nl, mean, N.stream()),
                "bwd")
    else:
        N.check(L_.glr_wordpiece_segsum_fwd(ptrs, nl, code, N.ptr(dst_d), N.ptr(w), N.ptr(s), B, L, D, mean, N.stream()), "fwd")
        N.check(L_.glr_wordpiece_segsum_bwd(N.ptr(dw), N.ptr(ds), N.ptr(dst_d), N.ptr(dh), code, B, L, D, nl, mean, N.stream()), "bwd")
    assert word.shape == (B, D, L) and torch.equal(word, w) and torch.equal(sent, s) and float(w.abs().sum()) > 0
    for h in layers:
        assert h.grad.dtype == torch.bfloat16 and torch.equal(h.grad, dh)
    assert float(dh.float().abs().sum()) > 0
    if packed:
        with pytest.raises(RuntimeError):
            _k5(dst_d[:, :-1].contiguous(), rows, mean_layers, layers)


# ------------------------------------------------------------------------------------------------ one layer loop
LOOP_LENS = [40, 7, 23]


def _bert(p_drop, bf16):
    from gloria.models import bert as BT
    torch.manual_seed(3)
    cfg = BT.BertConfig(vocab_size=1000, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512,
                        hidden_dropout_prob=p_drop, attention_probs_dropout_prob=p_drop)
    model = BT.BertModel(cfg).to(DEV).train()
    for m in model.modules():                # both sides compute with the same (bf16-representable) Linear parameters
        if isinstance(m, torch.nn.Linear):
            m.to(torch.bfloat16)
            if not bf16:
                m.to(torch.float32)
    return model


def _grads(model, hidden, weights):
    model.zero_grad(set_to_none=True)
    sum((h.float() * w).sum() for h, w in zip(hidden, weights)).backward()
    return {n: q.grad.detach().double() for n, q in model.named_parameters() if q.grad is not None}


def _rel(a, ref):
    den = float(ref.norm())
    return float((a - ref).norm()) / den if den else float((a - ref).norm())


def test_the_three_callers_of_the_layer_loop_agree(monkeypatch):
    """BertModel (2 layers, hidden 256, 4 heads), ids [3, 40], 40 / 7 / 23 live tokens, bf16 autocast, train mode, dropout
    0.1, one seed: hidden[-2:] of BertModel.forward equals BertStackPath(encoder, 2) on the embedding output bit for bit, and
    at the real rows encode_rows on the plan's rows.  Parameter gradients of the rows route sum across rows in another
    order: per tensor the distance to the padded route is at most 3 E_pad, E_pad the padded route's relative Frobenius
    error against the unfused fp32 path at dropout 0 (the bound of test_gpu_text_rows, derived there)."""
    from gloria.models import bert as BT
    from gloria.models import fused_attn as FA, fused_embed as FE, fused_linear as FLin, fused_ln as FL
    B, L = 3, 40
    g = torch.Generator().manual_seed(40)
    ids = torch.randint(5, 1000, (B, L), generator=g).to(DEV)
    am = _prefix_mask(LOOP_LENS, L).long()
    rows = _rows(LOOP_LENS, L)
    idx = rows.row_ids64
    weights = [(torch.randn(B, L, 256, generator=g).to(DEV) * am[:, :, None]) for _ in range(2)]
    weights_rows = [w.view(B * L, 256)[idx] for w in weights]

    def padded(model, autocast):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            torch.manual_seed(9)
            return model(ids, am)[2]

    # E_pad at dropout 0: the fused bf16 padded path against torch's own operators in fp32
    ref_model = _bert(0.0, bf16=False)
    for mod in (FA, FL, FLin, FE):
        monkeypatch.setattr(mod, "ENABLED", False)
    ref = _grads(ref_model, padded(ref_model, False)[-2:], weights)
    monkeypatch.undo()
    pad0_model = _bert(0.0, bf16=True)
    pad0 = _grads(pad0_model, padded(pad0_model, True)[-2:], weights)
    assert set(ref) == set(pad0)
    e_pad = {n: _rel(pad0[n], ref[n]) for n in ref}

    model = _bert(0.1, bf16=True)
    hidden = padded(model, True)
    assert len(hidden) == 3
    g_pad = _grads(model, hidden[-2:], weights)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        torch.manual_seed(9)
        x = model.embeddings(ids, None)
        assert torch.equal(x, hidden[0])
        stack = BT.BertStackPath(model.encoder, 2).train()(x, (am != 0)[:, None, None, :])
        torch.manual_seed(9)
        x = model.embeddings(ids, None)
        packed = BT.encode_rows(model.encoder, x, rows, 2)
        torch.manual_seed(9)
        first = BT.encode_rows(model.encoder, model.embeddings(ids, None), rows, 3)[0]
    assert len(stack) == 2 and len(packed) == 2
    for a, b, c in zip(hidden[-2:], stack, packed):
        assert torch.equal(a, b)
        assert c.shape == (rows.T, 256) and torch.equal(a.view(B * L, 256)[idx], c)
    assert torch.equal(first, hidden[0].view(B * L, 256)[idx])     # the gathered embedding output counts as the first
    g_rows = _grads(model, packed, weights_rows)
    assert set(g_rows) == set(g_pad)
    far = []
    for n in sorted(g_pad):
        d = _rel(g_rows[n], g_pad[n])
        print("%-56s %12.4e %12.4e" % (n, d, 3 * e_pad[n]))
        if not d <= 3 * e_pad[n]:
            far.append((n, d, 3 * e_pad[n]))
    assert not far, far
