"""The text encoder's real-token route (gloria/models/text_rows.py): the row-indexed kernels against the padded kernels
they share their bodies with - bit for bit at the real rows - and the whole encoder, its routing and one training run
against the padded path."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = -7.5             # exact in bf16 and fp32


def _plan(lengths, L):
    from gloria.models.text_rows import plan_rows
    mask = (np.arange(L)[None, :] < np.asarray(lengths)[:, None]).astype(np.int64)
    return plan_rows(mask, np.where(mask != 0, 0, -1), 128)


def _guarded(rows, cols, dtype, guard=4, fill=CANARY):
    """(buffer of rows + 2 * guard rows filled with the canary value, address of row `guard`)"""
    buf = torch.full((rows + 2 * guard, cols), fill, dtype=dtype, device=DEV)
    return buf, buf.data_ptr() + guard * cols * buf.element_size()


def _guards_intact(buf, rows, used_cols, guard=4):
    return bool((buf[:guard] == CANARY).all() and (buf[guard + rows:] == CANARY).all()
                and (buf[guard:guard + rows, used_cols:] == CANARY).all())


# ------------------------------------------------------------------------------------------------ attention
ATTN_LENS = [1, 31, 32, 33, 64, 65, 97, 128]


def _attn_inputs(extra):
    nh, H, Lp = 2, 128, 128
    B = len(ATTN_LENS)
    ld, ld_o = 3 * H + extra, H + extra
    row_start, row_ids = _plan(ATTN_LENS, Lp)
    g = torch.Generator().manual_seed(11 + extra)
    qkv_pad = torch.randn(B, Lp, ld, generator=g).bfloat16().to(DEV)          # pad rows hold data: nothing may read it
    do_pad = torch.randn(B, Lp, ld_o, generator=g).bfloat16().to(DEV)
    live = torch.zeros(B * Lp, dtype=torch.bool)
    live[torch.from_numpy(row_ids.astype(np.int64))] = True
    do_pad.view(B * Lp, ld_o)[~live.to(DEV)] = 0                               # zero d_o at pad rows
    key_mask = live.view(B, Lp).to(DEV)
    idx = torch.from_numpy(row_ids.astype(np.int64)).to(DEV)
    return dict(nh=nh, H=H, Lp=Lp, B=B, ld=ld, ld_o=ld_o, row_start=row_start, idx=idx, T=int(row_ids.shape[0]),
                qkv_pad=qkv_pad, do_pad=do_pad, key_mask=key_mask,
                qkv=qkv_pad.view(B * Lp, ld)[idx].contiguous(), do=do_pad.view(B * Lp, ld_o)[idx].contiguous())


def _attn_padded(c, p, seed, off):
    from gloria import _native as N
    L_ = N.lib()
    B, nh, H, Lp, ld, ld_o = c["B"], c["nh"], c["H"], c["Lp"], c["ld"], c["ld_o"]
    o = torch.zeros(B, Lp, ld_o, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(B * nh, 128, device=DEV)
    keep = torch.zeros(B * nh, 128, 4, dtype=torch.int32, device=DEV) if p > 0 else None
    base = c["qkv_pad"].data_ptr()
    N.check(L_.glr_attn_fwd(base, base + 2 * H, base + 4 * H, N.ptr(c["key_mask"]), B, nh, Lp, ld, ld_o, 0.125, p, seed, off, None,
                            N.ptr(o), N.ptr(lse), N.ptr(keep), N.stream()), "glr_attn_fwd")
    d = torch.zeros(B, Lp, ld, dtype=torch.bfloat16, device=DEV)
    db = d.data_ptr()
    N.check(L_.glr_attn_bwd(base, base + 2 * H, base + 4 * H, N.ptr(o), N.ptr(c["do_pad"]), N.ptr(c["key_mask"]), N.ptr(lse),
                            N.ptr(keep), B, nh, Lp, ld, ld_o, 0.125, p, db, db + 2 * H, db + 4 * H, N.stream()), "glr_attn_bwd")
    return o, lse, keep, d


def _attn_rows(c, p, seed, off):
    from gloria import _native as N
    L_ = N.lib()
    B, nh, H, ld, ld_o, T = c["B"], c["nh"], c["H"], c["ld"], c["ld_o"], c["T"]
    rs = np.ascontiguousarray(c["row_start"], dtype=np.int32)
    rs_d = torch.from_numpy(rs).to(DEV)
    o_buf, o_ptr = _guarded(T, ld_o, torch.bfloat16)
    lse_buf, lse_ptr = _guarded(B * nh, 128, torch.float32)
    keep_buf, keep_ptr = _guarded(B * nh, 512, torch.int32, fill=-7) if p > 0 else (None, None)
    base = c["qkv"].data_ptr()
    N.check(L_.glr_attn_rows_fwd(base, base + 2 * H, base + 4 * H, N.ptr(rs_d), rs.ctypes.data, B, nh, ld, ld_o, 0.125, p, seed, off,
                                 None, o_ptr, lse_ptr, keep_ptr, N.stream()), "glr_attn_rows_fwd")
    d_buf, d_ptr = _guarded(T, ld, torch.bfloat16)
    N.check(L_.glr_attn_rows_bwd(base, base + 2 * H, base + 4 * H, o_ptr, N.ptr(c["do"]), N.ptr(rs_d), rs.ctypes.data, lse_ptr,
                                 keep_ptr, B, nh, ld, ld_o, 0.125, p, d_ptr, d_ptr + 2 * H, d_ptr + 4 * H, N.stream()),
            "glr_attn_rows_bwd")
    torch.cuda.synchronize()
    return o_buf, lse_buf, keep_buf, d_buf


@pytest.mark.parametrize("extra", [0, 8])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention_rows_equal_padded_kernels_bit_for_bit(extra, p):
    """sentence lengths 1 .. 128 around every 32-row wave block edge, unsorted, in one batch; ld = 3H (packed) and
    ld = 3H + 8 (eight canary columns per row): o, lse, keep words, dq, dk, dv at the real rows equal glr_attn_fwd / _bwd on
    the padded copy (L = 128, prefix key mask, zero d_o at pad rows, same key) bit for bit; nothing outside the T rows
    or the head columns is written; a rerun gives the same bits"""
    c = _attn_inputs(extra)
    B, nh, H, Lp, T, idx = c["B"], c["nh"], c["H"], c["Lp"], c["T"], c["idx"]
    seed, off = 0x1234567887654321, 0x1_0000_0008
    o_p, lse_p, keep_p, d_p = _attn_padded(c, p, seed, off)
    o_b, lse_b, keep_b, d_b = _attn_rows(c, p, seed, off)
    G = 4
    assert torch.isfinite(o_p.float()).all() and torch.isfinite(d_p.float()).all()
    assert torch.equal(o_b[G:G + T, :H], o_p.view(B * Lp, -1)[idx, :H])
    assert torch.equal(d_b[G:G + T, :3 * H], d_p.view(B * Lp, -1)[idx, :3 * H])
    assert d_b[G:G + T, :3 * H].float().abs().sum() > 0
    for b, n in enumerate(ATTN_LENS):
        for hd in range(nh):
            bh = b * nh + hd
            assert torch.equal(lse_b[G + bh, :n], lse_p[bh, :n]), (b, hd)
            if p > 0:
                assert torch.equal(keep_b[G + bh].view(128, 4)[:n], keep_p[bh, :n]), (b, hd)
    assert _guards_intact(o_b, T, H) and _guards_intact(d_b, T, 3 * H) and _guards_intact(lse_b, B * nh, 128)
    if p > 0:
        assert bool((keep_b[:G] == -7).all() and (keep_b[G + B * nh:] == -7).all())
        frac = np.mean([float(np.unpackbits(keep_p[b * nh, :n].cpu().numpy().view(np.uint8)).mean())
                        for b, n in enumerate(ATTN_LENS) if n >= 64])
        assert abs(frac - 0.9) < 0.02                                          # the bits are dropout bits
    again = _attn_rows(c, p, seed, off)
    for a, b_ in zip((o_b, lse_b, keep_b, d_b), again):
        if a is not None:
            assert torch.equal(a[G:-G], b_[G:-G])


def test_attention_rows_reject_bad_plans_without_writing():
    from gloria import _native as N
    L_ = N.lib()
    c = _attn_inputs(0)
    B, nh, H, ld, ld_o, T = c["B"], c["nh"], c["H"], c["ld"], c["ld_o"], c["T"]
    good = np.ascontiguousarray(c["row_start"], dtype=np.int32)
    good_d = torch.from_numpy(good).to(DEV)
    empty = good.copy(); empty[3:] -= (good[3] - good[2])                       # n_2 = 0
    long_ = good.copy(); long_[-1] += 1                                         # n_7 = 129
    base = c["qkv"].data_ptr()
    o = torch.full((T + 8, ld_o), CANARY, dtype=torch.bfloat16, device=DEV)
    lse = torch.full((B * nh, 128), CANARY, device=DEV)
    keep = torch.full((B * nh, 128, 4), -7, dtype=torch.int32, device=DEV)
    d = torch.full((T + 8, ld), CANARY, dtype=torch.bfloat16, device=DEV)
    for dev_rs, host_rs in ((good_d, empty), (good_d, long_), (None, good), (good_d, None)):
        hp = None if host_rs is None else host_rs.ctypes.data
        assert L_.glr_attn_rows_fwd(base, base + 2 * H, base + 4 * H, N.ptr(dev_rs), hp, B, nh, ld, ld_o, 0.125, 0.1, 1, 0, None,
                                    N.ptr(o), N.ptr(lse), N.ptr(keep), N.stream()) == -1
        assert L_.glr_attn_rows_bwd(base, base + 2 * H, base + 4 * H, N.ptr(o), N.ptr(c["do"]), N.ptr(dev_rs), hp, N.ptr(lse),
                                    N.ptr(keep), B, nh, ld, ld_o, 0.125, 0.1, N.ptr(d), d.data_ptr() + 2 * H, d.data_ptr() + 4 * H,
                                    N.stream()) == -1
    torch.cuda.synchronize()
    assert bool((o == CANARY).all() and (lse == CANARY).all() and (keep == -7).all() and (d == CANARY).all())


# ------------------------------------------------------------------------------------------------ LN epilogue
def _philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays holding 32-bit values"""
    M = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) for v in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return c0, c1, c2, c3


def _decode_mask(mask, R, H):
    """uint64 words [R, H/64] -> bool [R, H] (element 4 (l + 64 i) + c of a row = bit l of word 4 i + c)"""
    w = mask.cpu().numpy().view(np.uint64).reshape(R, H // 64)
    lanes = np.arange(64, dtype=np.uint64)
    bits = ((w[:, :, None] >> lanes[None, None, :]) & np.uint64(1)).astype(bool)
    out = np.zeros((R, H), dtype=bool)
    for word in range(H // 64):
        i, c = word // 4, word % 4
        out[:, 4 * (np.arange(64) + 64 * i) + c] = bits[:, word, :]
    return out


def test_ln_epilogue_rows_draw_the_bits_of_their_original_rows():
    """37 packed rows with scattered, non-monotone row_ids (one of them past 2^32 / (H / 4): the counter's high word):
    y32, y16, mask words, d_inp, d_h equal the padded kernel's rows bit for bit (rows the padded tensor holds), every
    mask word equals Philox4x32-10 at the original row's counter (all rows, the far one included), and d-gamma, d-beta
    and the bias gradient - cross-row sums, the only order that changes - sit in test_gpu_fused_ln's band against fp64"""
    from gloria import _native as N
    from gloria.models import fused_ln as FL
    L_ = N.lib()
    H, R, Rp, p, eps = 256, 37, 300, 0.1, 1e-12
    seed, off = 0x9E3779B97F4A7C15, 0x2_0000_0010
    far = (1 << 32) // (H // 4) + 5
    rng = np.random.default_rng(3)
    ids = rng.permutation(Rp)[:R].astype(np.int64)
    ids[17] = far
    assert (np.diff(ids) < 0).any() and far * (H // 4) >= 1 << 32
    near = np.nonzero(ids < Rp)[0]
    g = torch.Generator().manual_seed(9)
    h_pad = (torch.randn(Rp, H, generator=g) * 1.3).bfloat16().to(DEV)
    inp_pad = (torch.randn(Rp, H, generator=g) * 0.8 + 0.1).to(DEV)
    w = (torch.rand(H, generator=g) + 0.5).to(DEV)
    b = (torch.randn(H, generator=g) * 0.2).to(DEV)
    d32_pad, d16_pad = torch.randn(Rp, H, generator=g).to(DEV), torch.randn(Rp, H, generator=g).bfloat16().to(DEV)
    src = torch.from_numpy(np.where(ids < Rp, ids, 0)).to(DEV)                   # the far row borrows the data of row 0
    h, inp, d32, d16 = (t[src].contiguous() for t in (h_pad, inp_pad, d32_pad, d16_pad))
    ids_d = torch.from_numpy(ids.astype(np.int32)).to(DEV)

    def run(h, inp, d32, d16, R, ids_d):
        o32, o16 = torch.empty(R, H, device=DEV), torch.empty(R, H, device=DEV, dtype=torch.bfloat16)
        st, m = torch.empty(R, 2, device=DEV), torch.zeros(R, H // 64, dtype=torch.int64, device=DEV)
        if ids_d is None:
            N.check(L_.glr_drop_add_ln_fwd(N.ptr(h), N.ptr(inp), N.ptr(w), N.ptr(b), R, H, eps, p, seed, off, None, N.ptr(o32),
                                           N.ptr(o16), N.ptr(st), N.ptr(m), N.stream()), "fwd")
        else:
            N.check(L_.glr_drop_add_ln_rows_fwd(N.ptr(h), N.ptr(inp), N.ptr(w), N.ptr(b), N.ptr(ids_d), R, H, eps, p, seed, off,
                                                None, N.ptr(o32), N.ptr(o16), N.ptr(st), N.ptr(m), N.stream()), "rows fwd")
        d_inp, d_h = torch.empty(R, H, device=DEV), torch.empty(R, H, device=DEV, dtype=torch.bfloat16)
        dgb, dhs = torch.empty(2, H, device=DEV), torch.empty(H, device=DEV)
        ws = torch.empty(L_.glr_ln_workspace_floats(R, H), device=DEV)
        N.check(L_.glr_drop_add_ln_bwd(N.ptr(d32), N.ptr(d16), N.ptr(h), N.ptr(inp), N.ptr(w), N.ptr(st), N.ptr(m), R, H, p,
                                       N.ptr(d_inp), N.ptr(d_h), N.ptr(ws), N.ptr(dgb), FL.c_off(dgb, H), N.ptr(dhs), 0, N.stream()), "bwd")
        return o32, o16, m, d_inp, d_h, dgb, dhs, st

    pad = run(h_pad, inp_pad, d32_pad, d16_pad, Rp, None)
    got = run(h, inp, d32, d16, R, ids_d)
    assert L_.glr_drop_add_ln_rows_fwd(N.ptr(h), N.ptr(inp), N.ptr(w), N.ptr(b), None, R, H, eps, p, seed, off, None, N.ptr(got[0]),
                                       N.ptr(got[1]), N.ptr(got[7]), N.ptr(got[2]), N.stream()) == -1      # null row_ids
    near_d, near_src = torch.from_numpy(near).to(DEV), torch.from_numpy(ids[near]).to(DEV)
    for name, a, ref in zip(("y32", "y16", "mask", "d_inp", "d_h"), got[:5], pad[:5]):
        assert torch.equal(a[near_d], ref[near_src]), name
    # every mask word against Philox itself: counter = original row * (H / 4) + quad, (offset) in the upper counter words
    quad = np.arange(H // 4, dtype=np.uint64)
    ctr = ids.astype(np.uint64)[:, None] * np.uint64(H // 4) + quad[None, :]
    M = np.uint64(0xFFFFFFFF)
    rnd = _philox4x32_10(ctr & M, ctr >> np.uint64(32), np.full_like(ctr, off & 0xFFFFFFFF), np.full_like(ctr, off >> 32),
                         seed & 0xFFFFFFFF, seed >> 32)
    thr = np.uint64(int(np.float32(p) * np.float32(4294967296.0)))
    want = np.zeros((R, H), dtype=bool)
    for c_ in range(4):
        want[:, 4 * np.arange(H // 4) + c_] = rnd[c_] >= thr
    keep = _decode_mask(got[2], R, H)
    assert np.array_equal(keep, want)
    assert not torch.equal(got[2][17], pad[2][0])          # the far row holds row 0's data and draws its own bits
    # cross-row sums against fp64 (and the far row's outputs with them: its data is row 0's, its mask its own)
    k64 = torch.from_numpy(keep).to(DEV)
    hr, ir = h.double().requires_grad_(True), inp.double().requires_grad_(True)
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    y = torch.nn.functional.layer_norm(hr * k64 / (1 - p) + ir, (H,), wr, br, eps)
    (y * (d32.double() + d16.double())).sum().backward()
    np.testing.assert_allclose(got[0].cpu().numpy(), y.detach().cpu().numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(got[3].cpu().numpy(), ir.grad.cpu().numpy(), rtol=2e-4, atol=2e-4)
    scale = float(wr.grad.abs().max())
    np.testing.assert_allclose(got[5][0].cpu().numpy() / scale, wr.grad.cpu().numpy() / scale, atol=1e-4)
    scale = float(br.grad.abs().max())
    np.testing.assert_allclose(got[5][1].cpu().numpy() / scale, br.grad.cpu().numpy() / scale, atol=1e-4)
    ref_hs = got[4].double().sum(0)                  # column sums of the bf16 d_h the kernel wrote
    scale = float(ref_hs.abs().max())
    np.testing.assert_allclose(got[6].cpu().numpy() / scale, ref_hs.cpu().numpy() / scale, atol=2e-3)
    ref_hs = hr.grad.sum(0)
    scale = float(ref_hs.abs().max())
    np.testing.assert_allclose(got[6].cpu().numpy() / scale, ref_hs.cpu().numpy() / scale, atol=2e-3)


# ------------------------------------------------------------------------------------------------ K5
@pytest.mark.parametrize("D", [48, 256])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_wordpiece_segsum_rows_equal_padded_k5(D, dtype):
    """B = 5, L = 40, four layers, word pieces merged up to the ragged end of a sentence: word_emb and sent_emb are
    bitwise the padded K5's, d_hidden is bitwise its packed rows, and nothing behind the T rows is written"""
    import ctypes
    from gloria import _native as N
    L_ = N.lib()
    B, L, nl = 5, 40, 4
    lengths = [40, 7, 1, 23, 39]
    rng = np.random.default_rng(D)
    dst = np.full((B, L), -1, dtype=np.int32)
    for b_, n in enumerate(lengths):
        starts = rng.random(n) < 0.6
        starts[0] = True
        if n >= 3:
            starts[n - 1] = False                                                # the last word ends in a merged piece
        dst[b_, :n] = np.cumsum(starts) - 1
    dst[3, 20:23] = -1                                                           # dropped tokens inside the prefix
    row_start, row_ids = _plan(lengths, L)
    assert dst[0, 39] == dst[0, 38] and dst[4, 38] == dst[4, 37] and dst[1, 6] == dst[1, 5]
    idx = torch.from_numpy(row_ids.astype(np.int64)).to(DEV)
    T = int(row_ids.shape[0])
    g = torch.Generator().manual_seed(D + 1)
    pads = [torch.randn(B, L, D, generator=g).to(dtype).to(DEV) for _ in range(nl)]
    packs = [h.view(B * L, D)[idx].contiguous() for h in pads]
    dst_d, rs_d = torch.from_numpy(dst).to(DEV), torch.from_numpy(row_start).to(DEV)
    code = N.dtype_code(dtype)

    def fwd(hs, rows):
        word, sent = torch.empty(B, D, L, device=DEV), torch.empty(B, D, device=DEV)
        ptrs = (ctypes.c_void_p * nl)(*[h.data_ptr() for h in hs])
        if rows:
            N.check(L_.glr_wordpiece_segsum_rows_fwd(ptrs, nl, code, N.ptr(dst_d), N.ptr(rs_d), N.ptr(word), N.ptr(sent), B, L, D, 1,
                                                     N.stream()), "rows fwd")
        else:
            N.check(L_.glr_wordpiece_segsum_fwd(ptrs, nl, code, N.ptr(dst_d), N.ptr(word), N.ptr(sent), B, L, D, 1, N.stream()), "fwd")
        return word, sent

    (w_p, s_p), (w_r, s_r) = fwd(pads, False), fwd(packs, True)
    assert torch.equal(w_p, w_r) and torch.equal(s_p, s_r) and w_p.abs().sum() > 0
    dw, ds = torch.randn(B, D, L, generator=g).to(DEV), torch.randn(B, D, generator=g).to(DEV)
    dh_p = torch.empty(B, L, D, dtype=dtype, device=DEV)
    N.check(L_.glr_wordpiece_segsum_bwd(N.ptr(dw), N.ptr(ds), N.ptr(dst_d), N.ptr(dh_p), code, B, L, D, nl, 1, N.stream()), "bwd")
    buf, ptr = _guarded(T, D, dtype)
    N.check(L_.glr_wordpiece_segsum_rows_bwd(N.ptr(dw), N.ptr(ds), N.ptr(dst_d), N.ptr(rs_d), ptr, code, B, L, D, nl, 1, N.stream()),
            "rows bwd")
    assert torch.equal(buf[4:4 + T], dh_p.view(B * L, D)[idx]) and _guards_intact(buf, T, D)
    assert L_.glr_wordpiece_segsum_rows_bwd(N.ptr(dw), N.ptr(ds), N.ptr(dst_d), None, ptr, code, B, L, D, nl, 1, N.stream()) == -1


# ------------------------------------------------------------------------------------------------ whole encoder
ENC_LENS = [3, 7, 16, 33, 39, 40]


def _encoder(p_drop, bf16, layers=2):
    from gloria.config import pretrain_config
    from gloria.models import text_model as TM
    cfg = pretrain_config("imagenome", batch_size=len(ENC_LENS))
    cfg.set_path("model.text.bert_config", dict(vocab_size=2000, hidden_size=256, num_hidden_layers=layers, num_attention_heads=4,
                                                intermediate_size=512, hidden_dropout_prob=p_drop,
                                                attention_probs_dropout_prob=p_drop))
    torch.manual_seed(7)
    enc = TM.BertEncoder(cfg).to(DEV).train()
    for m in enc.modules():                  # both sides compute with the same (bf16-representable) Linear parameters
        if isinstance(m, torch.nn.Linear):
            m.to(torch.bfloat16)
            if not bf16:
                m.to(torch.float32)
    return enc


def _enc_batch(lengths=ENC_LENS, L=40):
    from gloria.datasets.synthetic import make_batch
    b = make_batch(len(lengths), seed=5, word_num=L, vocab_size=2000, lengths=[n - 2 for n in lengths])
    out = {}
    for k in ("caption_ids", "attention_mask", "token_type_ids"):
        out[k] = b[k].to(DEV)
        out[k]._glr_host = b[k].numpy()
    assert sorted(b["attention_mask"].sum(1).tolist()) == sorted(lengths)
    return out


def _enc_run(enc, batch, packed, autocast, capture=None):
    """one forward + backward from a fixed generator state -> {name: tensor} of the outputs and every parameter gradient"""
    from gloria.models import text_model as TM
    from gloria.models import text_rows as TR
    calls = []
    real = TM.encode_rows
    TM.encode_rows = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    prev, TR.ENABLED = TR.ENABLED, packed
    hooks = []
    if capture is not None:
        l0 = enc.model.encoder.layer[0]
        # the bits the first layer stored for its backward: keep words of the attention, mask words of the two epilogues
        hooks = [l0.attention.self.register_forward_hook(lambda m, i, o: capture.__setitem__("attn", o.grad_fn.saved_tensors[3])),
                 l0.attention.output.register_forward_hook(lambda m, i, o: capture.__setitem__("ln1", o[0].grad_fn.saved_tensors[4])),
                 l0.output.register_forward_hook(lambda m, i, o: capture.__setitem__("ln2", o[0].grad_fn.saved_tensors[4]))]
    try:
        enc.zero_grad(set_to_none=True)
        torch.manual_seed(123)
        ctx = torch.autocast("cuda", dtype=torch.bfloat16) if autocast else torch.autocast("cuda", enabled=False)
        with ctx:
            word, sent, _ = enc(batch["caption_ids"], batch["attention_mask"], batch["token_type_ids"])
        g = torch.Generator().manual_seed(77)
        gw, gs = torch.randn(word.shape, generator=g).to(DEV), torch.randn(sent.shape, generator=g).to(DEV)
        ((word.float() * gw).sum() + (sent.float() * gs).sum()).backward()
    finally:
        TM.encode_rows, TR.ENABLED = real, prev
        for h in hooks:
            h.remove()
    assert bool(calls) == bool(packed), "the route taken is not the route asked for"
    out = {"word_emb": word.detach().double(), "sent_emb": sent.detach().double()}
    for n, q in enc.named_parameters():
        out["grad " + n] = None if q.grad is None else q.grad.detach().double()
    return out


def _rel(a, ref):
    if a is None or ref is None:
        assert a is None and ref is None, "a gradient is None on one side only"
        return None
    den = float(ref.norm())
    num = float((a - ref).norm())
    if den == 0.0:
        assert num == 0.0
        return 0.0
    return num / den


def test_encoder_on_real_rows_is_as_close_to_fp32_as_the_padded_path(monkeypatch):
    """BertEncoder (2 layers, hidden 256, 4 heads, intermediate 512), B = 6, L = 40, lengths 3 .. 40, training mode.
    Dropout 0: relative Frobenius error per tensor (outputs and every parameter gradient) against the unfused fp32 torch
    path: E_pack <= 1.5 E_pad (identical arithmetic apart from summation order; 1.5 absorbs noise on small tensors).
    Dropout 0.1, same generator state: the first layer's stored dropout bits are equal, and the packed-to-padded distance
    per tensor is <= 3 E_pad (two roundings of the same quantity: 2, times the same 1.5)."""
    from gloria.models import fused_attn as FA, fused_embed as FE, fused_linear as FLin, fused_ln as FL
    batch = _enc_batch()
    ref_enc = _encoder(0.0, bf16=False)
    for mod in (FA, FL, FLin, FE):
        monkeypatch.setattr(mod, "ENABLED", False)
    ref = _enc_run(ref_enc, batch, packed=False, autocast=False)
    monkeypatch.undo()
    enc = _encoder(0.0, bf16=True)
    pad = _enc_run(enc, batch, packed=False, autocast=True)
    pack = _enc_run(enc, batch, packed=True, autocast=True)
    assert set(ref) == set(pad) == set(pack)
    e_pad, worst = {}, []
    print("\ndropout 0: relative Frobenius error against the unfused fp32 path")
    print("%-64s %12s %12s %8s" % ("tensor", "E_pad", "E_pack", "ratio"))
    for n in sorted(ref):
        e_pad[n], e_pack = _rel(pad[n], ref[n]), _rel(pack[n], ref[n])
        if e_pad[n] is None:
            assert pack[n] is None
            print("%-64s %12s %12s" % (n, "None", "None"))
            continue
        print("%-64s %12.4e %12.4e %8.3f" % (n, e_pad[n], e_pack, e_pack / e_pad[n] if e_pad[n] else 0.0))
        if not e_pack <= 1.5 * e_pad[n]:
            worst.append((n, e_pad[n], e_pack))
    # dropout 0.1: the same masks by construction
    encd = _encoder(0.1, bf16=True)
    cap_pad, cap_pack = {}, {}
    padd = _enc_run(encd, batch, packed=False, autocast=True, capture=cap_pad)
    packd = _enc_run(encd, batch, packed=True, autocast=True, capture=cap_pack)
    from gloria.models.text_rows import plan_rows
    mask_h = batch["attention_mask"]._glr_host
    row_start, row_ids = plan_rows(mask_h, np.where(mask_h != 0, 0, -1), 128)
    idx = torch.from_numpy(row_ids.astype(np.int64)).to(DEV)
    for site in ("ln1", "ln2"):
        m_pad, m_pack = cap_pad[site], cap_pack[site]
        assert m_pack.shape[0] == idx.shape[0] and torch.equal(m_pack, m_pad[idx]), site
    k_pad, k_pack = cap_pad["attn"], cap_pack["attn"]
    n_tok = np.diff(row_start)
    for b_, n in enumerate(n_tok):
        for hd in range(4):
            assert torch.equal(k_pack[b_ * 4 + hd, :n], k_pad[b_ * 4 + hd, :n]), (b_, hd)
    print("dropout 0.1: packed-to-padded relative distance (bound 3 E_pad)")
    far = []
    for n in sorted(padd):
        d = _rel(packd[n], padd[n])
        if d is None:
            print("%-64s %12s" % (n, "None"))
            continue
        print("%-64s %12.4e %12.4e" % (n, d, 3 * e_pad[n]))
        if not d <= 3 * e_pad[n]:
            far.append((n, d, 3 * e_pad[n]))
    assert not worst, worst
    assert not far, far


def test_routing_keeps_the_padded_path_when_packing_does_not_apply(monkeypatch):
    """an all-full batch, the switch off, and a captured text graph all run today's path"""
    from gloria.models import text_rows as TR
    enc = _encoder(0.0, bf16=True)
    full = _enc_batch(lengths=[24] * 4, L=24)
    ragged = _enc_batch()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert enc._packed_rows(full["caption_ids"], full["attention_mask"]) == (None, None)
        assert enc._packed_rows(ragged["caption_ids"], ragged["attention_mask"])[0] is not None
        bare = ragged["attention_mask"].clone()                                  # no host copy of the mask: no sync, no packing
        assert enc._packed_rows(ragged["caption_ids"], bare) == (None, None)
        monkeypatch.setattr(TR, "ENABLED", False)
        assert enc._packed_rows(ragged["caption_ids"], ragged["attention_mask"]) == (None, None)
        monkeypatch.setattr(TR, "ENABLED", True)
    assert enc._packed_rows(ragged["caption_ids"], ragged["attention_mask"]) == (None, None)      # no autocast
    a = _enc_run(enc, full, packed=False, autocast=True)
    real, TR.ENABLED = TR.ENABLED, True
    try:
        enc.zero_grad(set_to_none=True)
        torch.manual_seed(123)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            word, sent, _ = enc(full["caption_ids"], full["attention_mask"], full["token_type_ids"])
    finally:
        TR.ENABLED = real
    assert torch.equal(word.detach().double(), a["word_emb"]) and torch.equal(sent.detach().double(), a["sent_emb"])
    monkeypatch.setenv("GLR_TEXT_PACKED", "0")
    assert TR._switch() is False
    monkeypatch.setenv("GLR_TEXT_PACKED", "1")
    assert TR._switch() is True
    # a captured graph for this shape keeps its path (the capture wants as many layers as hidden states are read: 4)
    from gloria import hipgraph
    if hipgraph.usable("text encoder"):
        enc = _encoder(0.0, bf16=True, layers=4)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            assert enc.enable_graph(ragged["caption_ids"], ragged["attention_mask"], ragged["token_type_ids"], torch.bfloat16)
            assert enc._packed_rows(ragged["caption_ids"], ragged["attention_mask"]) == (None, None)
            graph = enc._graph
            object.__setattr__(enc, "_graph", None)
            assert enc._packed_rows(ragged["caption_ids"], ragged["attention_mask"])[0] is not None
            object.__setattr__(enc, "_graph", graph)


def test_training_losses_with_the_switch_on_and_off(monkeypatch):
    """B = 8, two BERT layers, three different batches, text graph off: the losses of the packed and the padded route sit in
    the band of one step through two execution paths (tests/test_gpu_train.py: rtol 1e-3 on the first loss, 4e-2 after)"""
    from gloria import builder
    from gloria.config import pretrain_config
    from gloria.datasets.synthetic import make_batch
    from gloria.models import text_model as TM
    from gloria.models import text_rows as TR
    from gloria.trainer import Trainer
    B = 8
    batches = [make_batch(B, seed=40 + i) for i in range(3)]
    calls = []
    real = TM.encode_rows
    monkeypatch.setattr(TM, "encode_rows", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    losses = {}
    for mode in (False, True):
        monkeypatch.setattr(TR, "ENABLED", mode)
        torch.manual_seed(21)
        c = pretrain_config("imagenome", batch_size=B)
        c.set_path("model.text.bert_config", dict(num_hidden_layers=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0))
        model = builder.build_lightning_model(c, builder.build_data_module(c))
        tr = Trainer(c, device=DEV, precision="bf16", flat_optimizer=True, graph_text_encoder=False)
        tr.setup(model)
        model.train()
        n0 = len(calls)
        losses[mode] = [float(tr.training_step(model, b, i)) for i, b in enumerate(batches)]
        assert (len(calls) - n0) == (3 if mode else 0)
    print("\nlosses padded", losses[False], "packed", losses[True])
    np.testing.assert_allclose(losses[True][0], losses[False][0], rtol=1e-3)
    np.testing.assert_allclose(losses[True], losses[False], rtol=4e-2)
