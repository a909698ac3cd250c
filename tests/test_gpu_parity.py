"""GPU parity tests: the HIP path (through the C ABI of libglr.so) against
  (1) the golden outputs of the real reference (tests/golden, made by oracle/gen_golden.py),
  (2) the CPU oracle on the same seeded inputs, incl. the edge cases the domain has,
  (3) size-independent properties at the bench size (B = 256).

Tolerances: fp32 mode 1e-4 (north star); bf16 mode is checked against the oracle evaluated on the
bf16-rounded inputs with the tolerance written next to each check.
"""

import numpy as np
import pytest
import torch

import golden_inputs as gi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def gl():
    from gloria.loss import gloria_loss
    return gloria_loss


def orc():
    from oracle import gloria_oracle
    return gloria_oracle


def g(a, grad=False):
    x = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return x.requires_grad_(True) if grad else x


def check(golden, key, arr, rtol=1e-4, atol=1e-4):
    arr = arr.detach().float().cpu().numpy()
    assert tuple(golden[key + ".shape"]) == tuple(arr.shape), key
    np.testing.assert_allclose(gi.subsample(arr), golden[key + ".sample"], rtol=rtol, atol=atol, err_msg=key)


# ------------------------------------------------------------------ (1) golden vectors, fp32 mode

@pytest.mark.parametrize("name", list(gi.ATTN_CASES))
def test_attention_fn_golden(golden, name):
    gd = golden("attention")
    q, ctx, temp1, na = gi.attn_inputs(name)
    wc, attn = gl().attention_fn(g(q), g(ctx), temp1, no_attn_vec=None if na is None else g(na))
    check(gd, f"attn/{name}/weighted", wc, rtol=1e-4, atol=1e-5)
    check(gd, f"attn/{name}/map", attn, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("name", list(gi.ATTN_CASES))
def test_attention_fn_output_grads_golden(golden, name):
    """gradients of attention_fn's own outputs (weighted context + maps) against the reference's autograd:
    PairAttnFn.backward with both upstream gradients live"""
    gd = golden("attention_grad")
    q, ctx, temp1, na = gi.attn_inputs(name)
    tq, tc = g(q, True), g(ctx, True)
    tna = None if na is None else g(na, True)
    wc, attn = gl().attention_fn(tq, tc, temp1, no_attn_vec=tna)
    gw, ga = gi.attn_upstream(name, tuple(wc.shape), tuple(attn.shape))
    ((wc * g(gw)).sum() + (attn * g(ga)).sum()).backward()
    check(gd, f"attn_grad/{name}/grad_query", tq.grad, rtol=2e-3, atol=2e-5)
    check(gd, f"attn_grad/{name}/grad_context", tc.grad, rtol=2e-3, atol=2e-5)
    if tna is not None:
        check(gd, f"attn_grad/{name}/grad_no_attn", tna.grad, rtol=2e-3, atol=2e-4)


@pytest.mark.parametrize("which", ["weighted", "map"])
@pytest.mark.parametrize("name", ["a1_tiny", "a3_noattn_n96"])
def test_attention_fn_single_output_grads_vs_oracle(name, which):
    """Backpropagate ONE of attention_fn's two outputs (the other reaches PairAttnFn.backward as None) and compare
    the input gradients with fp64 autograd through the oracle, in the bands of
    test_attention_fn_output_grads_golden; the forward is bit-identical without gradient tracking."""
    q, ctx, temp1, na = gi.attn_inputs(name)
    tq, tc = g(q, True), g(ctx, True)
    tna = None if na is None else g(na, True)
    outs = gl().attention_fn(tq, tc, temp1, no_attn_vec=tna)
    with torch.no_grad():
        quiet = gl().attention_fn(tq, tc, temp1, no_attn_vec=tna)
    plain = gl().attention_fn(g(q), g(ctx), temp1, no_attn_vec=None if na is None else g(na))
    for o, a, b in zip(outs, quiet, plain):
        assert not a.requires_grad and not b.requires_grad
        assert torch.equal(o, a) and torch.equal(o, b)
    k = ("weighted", "map").index(which)
    up = gi.attn_upstream(name, tuple(outs[0].shape), tuple(outs[1].shape))[k]
    (outs[k] * g(up)).sum().backward()
    rq, rc = torch.from_numpy(q).double().requires_grad_(True), torch.from_numpy(ctx).double().requires_grad_(True)
    rna = None if na is None else torch.from_numpy(na).double().requires_grad_(True)
    (orc().attention_fn(rq, rc, temp1, no_attn_vec=rna)[k] * torch.from_numpy(up).double()).sum().backward()
    cases = [("grad_query", tq, rq, 2e-5), ("grad_context", tc, rc, 2e-5)]
    if na is not None:
        cases.append(("grad_no_attn", tna, rna, 2e-4))
    errs = [(label, t.grad.double().cpu().numpy(), r.grad.numpy(), atol) for label, t, r, atol in cases]
    for label, got, want, atol in errs:
        d = np.abs(got - want)
        print(f"[{name} {which}] {label}: max |d| / max |ref| = {d.max() / np.abs(want).max():.3e}, "
              f"worst |d| / (atol + rtol |ref|) = {(d / (atol + 2e-3 * np.abs(want))).max():.3e}")
    for label, got, want, atol in errs:
        np.testing.assert_allclose(got, want, rtol=2e-3, atol=atol, err_msg=label)


@pytest.mark.parametrize("name", [n for n, c in gi.LOCAL_CASES.items() if c["aux"] is None])
def test_local_loss_golden(golden, name):
    gd = golden("local")
    cfg = gi.LOCAL_CASES[name]
    img, words, cap_lens, na = gi.local_inputs(name)
    timg, twords = g(img, True), g(words, True)
    tna = None if na is None else g(na, True)
    l0, l1, nal, kl, ent, maps = gl().local_loss(timg, twords, cap_lens, agg=cfg["agg"], no_attn_vec=tna)
    ref = gd[f"local/{name}/losses"]
    np.testing.assert_allclose([float(l0), float(l1)], ref[:2], rtol=1e-4, atol=1e-4)
    assert len(maps) == cfg["B"] and all(m.shape == (1, n, cfg["H"], cfg["W"]) for m, n in zip(maps, cap_lens))
    check(gd, f"local/{name}/maps", torch.cat([m.reshape(-1) for m in maps]), rtol=1e-4, atol=1e-6)
    sim, _, _ = gl().local_similarity(timg, twords, cap_lens, agg=cfg["agg"], no_attn_vec=tna)
    check(gd, f"local/{name}/sim", sim, rtol=1e-4, atol=1e-4)
    (l0 + l1).backward()
    check(gd, f"local/{name}/grad_img", timg.grad, rtol=2e-3, atol=2e-6)
    check(gd, f"local/{name}/grad_words", twords.grad, rtol=2e-3, atol=2e-6)
    if tna is not None:
        check(gd, f"local/{name}/grad_no_attn", tna.grad, rtol=2e-3, atol=2e-6)


@pytest.mark.parametrize("name", [n for n, c in gi.LOCAL_CASES.items() if c["aux"] is not None])
def test_local_loss_with_attention_regularisers_golden(golden, name):
    """The reference's training flags (--no_attn_vec + no-attention / divergence / entropy regularisers,
    gloria_loss.py:108-114, 129-139, 172-199): all five losses and the gradients of their sum against the
    outputs of the real reference, fp32 mode."""
    gd = golden("local")
    cfg = gi.LOCAL_CASES[name]
    img, words, cap_lens, na = gi.local_inputs(name)
    timg, twords, tna = g(img, True), g(words, True), g(na, True)
    aux = cfg["aux"]
    l0, l1, nal, kl, ent, maps = gl().local_loss(timg, twords, cap_lens, agg=cfg["agg"], no_attn_vec=tna,
                                                 no_attn_loss_weight=aux[0], attention_divergence_loss_weight=aux[1],
                                                 attention_entropy_loss_weight=aux[2])
    got = [float(x.detach()) for x in (l0, l1, nal, kl, ent)]
    np.testing.assert_allclose(got, gd[f"local/{name}/losses"], rtol=1e-4, atol=1e-4)
    check(gd, f"local/{name}/maps", torch.cat([m.reshape(-1) for m in maps]), rtol=1e-4, atol=1e-6)
    (l0 + l1 + nal + kl + ent).backward()
    check(gd, f"local/{name}/grad_img", timg.grad, rtol=2e-3, atol=2e-6)
    check(gd, f"local/{name}/grad_words", twords.grad, rtol=2e-3, atol=2e-6)
    check(gd, f"local/{name}/grad_no_attn", tna.grad, rtol=2e-3, atol=2e-6)


@pytest.mark.parametrize("no_attn", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_attention_regularisers_vs_oracle(dtype, no_attn):
    """Regularisers through the production kernels (bf16: pair kernel + single-tile backward; fp32: 32-word
    tiles) at 361/362 regions with ragged sentences, against the oracle on the same (rounded) inputs."""
    B, D, H, W, L = 12, 768, 19, 19, 97
    cap_lens = [70, 40, 33, 23, 22, 17, 11, 9, 5, 5, 2, 1]
    seed = 4242
    img, words = g(gi.normal(seed, B, D, H, W)).to(dtype), g(gi.normal(seed + 1, B, D, L)).to(dtype)
    na = g(gi.normal(seed + 2, D, std=1.0)).to(dtype) if no_attn else None
    w = (1.0, 0.1, 1.0) if no_attn else (None, 0.1, 1.0)      # the no-attention score needs the extra column
    ti, tw = img.clone().requires_grad_(True), words.clone().requires_grad_(True)
    tn = None if na is None else na.clone().requires_grad_(True)
    out = gl().local_loss(ti, tw, cap_lens, no_attn_vec=tn, no_attn_loss_weight=w[0],
                          attention_divergence_loss_weight=w[1], attention_entropy_loss_weight=w[2])
    sum(x for x in out[:5] if torch.is_tensor(x)).backward()
    ri, rw = img.float().cpu().requires_grad_(True), words.float().cpu().requires_grad_(True)
    rn = None if na is None else na.float().cpu().requires_grad_(True)
    ref = orc().local_loss(ri, rw, cap_lens, no_attn_vec=rn, no_attn_loss_weight=w[0],
                           attention_divergence_loss_weight=w[1], attention_entropy_loss_weight=w[2])
    sum(x for x in ref[:5] if torch.is_tensor(x)).backward()
    f32 = dtype == torch.float32
    for k in (2, 3, 4):                                       # no-attention, divergence, entropy
        if torch.is_tensor(ref[k]):
            np.testing.assert_allclose(float(out[k].detach()), float(ref[k]), rtol=1e-4 if f32 else 2e-2,
                                       atol=1e-5 if f32 else 2e-3)
    rt, at = (2e-3, 1e-5) if f32 else (0.1, 2e-3)        # fp32: sums over 12 x 237 words x 362 regions, 1e-5 absolute noise floor
    pairs = [(ti.grad, ri.grad), (tw.grad, rw.grad)] + ([] if tn is None else [(tn.grad, rn.grad)])
    for a, b in pairs:
        a, b = a.float().cpu().numpy(), b.numpy()
        if f32:
            np.testing.assert_allclose(a, b, rtol=rt, atol=at)
        else:                                                 # bf16 operands: relative error of the whole tensor
            assert np.linalg.norm(a - b) / np.linalg.norm(b) < 0.05


@pytest.mark.parametrize("name", list(gi.SIM_CASES))
def test_sim_matrix_golden(golden, name):
    gd = golden("sim")
    img, words, cap_lens, _ = gi.local_inputs(name)
    sim, _, _ = gl().local_similarity(g(img), g(words), cap_lens, want_attn=False)
    ref = gd[f"sim/{name}/sim"]
    np.testing.assert_allclose(sim.cpu().numpy(), ref, rtol=1e-4, atol=1e-4)
    l0, l1 = gl().dual_cross_entropy(sim)
    np.testing.assert_allclose([float(l0), float(l1)], gd[f"sim/{name}/losses"], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("name", list(gi.GLOBAL_CASES))
def test_global_loss_golden(golden, name):
    gd = golden("global")
    img, txt = gi.global_inputs(name)
    ti, tt = g(img, True), g(txt, True)
    l0, l1 = gl().global_loss(ti, tt)
    np.testing.assert_allclose([float(l0), float(l1)], gd[f"global/{name}/losses"], rtol=1e-4, atol=1e-4)
    (l0 + l1).backward()
    zero_row = gi.GLOBAL_CASES[name][2]
    if zero_row is None:
        check(gd, f"global/{name}/grad_img", ti.grad, rtol=1e-3, atol=1e-6)
    else:  # see tests/test_oracle_golden.py: the clamped row is a 1e9-scaled cancellation
        ref = gd[f"global/{name}/grad_img.sample"].reshape(ti.shape)
        got = ti.grad.cpu().numpy()
        keep = np.arange(ti.shape[0]) != zero_row
        np.testing.assert_allclose(got[keep], ref[keep], rtol=1e-3, atol=1e-6)
        scale = np.abs(ref[zero_row]).max()
        np.testing.assert_allclose(got[zero_row] / scale, ref[zero_row] / scale, atol=2e-2)
    check(gd, f"global/{name}/grad_txt", tt.grad, rtol=1e-3, atol=1e-6)


@pytest.mark.parametrize("shape", [(32, 256, 768), (5, 13, 70), (33, 31, 100), (256, 64, 768)])
def test_global_similarity_rectangular_vs_oracle(shape):
    """K3 (fp32 MFMA) on block-row shapes of the data-parallel layout and on sizes that are no multiple of the
    32-wide tiles / 8-wide k groups, forward and both gradients, incl. an eps-clamped zero row"""
    Bi, Bt, D = shape
    img, txt = gi.normal(901 + Bi, Bi, D), gi.normal(902 + Bt, Bt, D)
    img[Bi // 2] = 0.0
    a, t = g(img, True), g(txt, True)
    sim = gl().global_similarity(a, t)
    ra, rt = torch.from_numpy(img).requires_grad_(True), torch.from_numpy(txt).requires_grad_(True)
    want = orc().global_similarity_matrix(ra, rt)
    np.testing.assert_allclose(sim.detach().cpu().numpy(), want.detach().numpy(), rtol=1e-5, atol=1e-5)
    w = torch.from_numpy(gi.normal(903, Bi, Bt))
    (sim * w.to(DEV)).sum().backward()
    (want * w).sum().backward()
    keep = np.arange(Bi) != Bi // 2
    np.testing.assert_allclose(a.grad.cpu().numpy()[keep], ra.grad.numpy()[keep], rtol=1e-4, atol=1e-6)
    zr, zw = a.grad.cpu().numpy()[Bi // 2], ra.grad.numpy()[Bi // 2]          # (temp3 / eps)-scaled row
    np.testing.assert_allclose(zr / np.abs(zw).max(), zw / np.abs(zw).max(), atol=1e-4)
    np.testing.assert_allclose(t.grad.cpu().numpy() / np.abs(rt.grad.numpy()).max(),
                               rt.grad.numpy() / np.abs(rt.grad.numpy()).max(), atol=1e-5)


# ------------------------------------------------------------------ (2) oracle on seeded inputs, edge cases

EDGE = {
    # name: (B, D, H, W, L, cap_lens, no_attn, agg)
    "all_ones": (5, 64, 5, 5, 8, [1, 1, 1, 1, 1], False, "sum"),
    "tile_exact_64_65": (4, 128, 7, 9, 97, [64, 65, 63, 1], False, "sum"),
    "ragged_noattn_mean": (6, 768, 19, 19, 97, [96, 50, 14, 14, 3, 1], True, "mean"),
    "one_pair": (1, 64, 3, 3, 5, [4], False, "sum"),
    "max_agg": (4, 192, 19, 19, 40, [40, 17, 9, 2], False, "max"),
    "stress_s197_n256": (3, 768, 14, 14, 256, [256, 130, 77], True, "sum"),
}


@pytest.mark.parametrize("name", list(EDGE))
def test_edge_cases_vs_oracle(name):
    B, D, H, W, L, cap_lens, na_flag, agg = EDGE[name]
    seed = gi.case_seed(name)
    img, words = gi.normal(seed, B, D, H, W), gi.normal(seed + 1, B, D, L)
    na = gi.normal(seed + 2, D, std=1.0) if na_flag else None
    o = orc()
    tna = None if na is None else torch.from_numpy(na)
    want, a2, seg = o.local_similarity_matrix(torch.from_numpy(img), torch.from_numpy(words), cap_lens, agg=agg,
                                              no_attn_vec=tna, return_attn=True)
    sim, attn, plan = gl().local_similarity(g(img), g(words), cap_lens, agg=agg,
                                            no_attn_vec=None if na is None else g(na))
    np.testing.assert_allclose(sim.cpu().numpy(), want.numpy(), rtol=1e-4, atol=1e-4)
    # diagonal maps
    shift = 1 if na_flag else 0
    off = 0
    woff = np.concatenate([[0], np.cumsum(cap_lens)])
    flat = attn.cpu().numpy()
    for b in range(B):
        n = cap_lens[b]
        ref = a2[b, woff[b]:woff[b] + n, shift:].numpy().reshape(-1)
        np.testing.assert_allclose(flat[off:off + ref.size], ref, rtol=1e-4, atol=1e-6)
        off += ref.size


def test_bf16_mode_vs_oracle_on_rounded_inputs():
    """bf16 operands, fp32 accumulate.  Compared with the fp32 oracle evaluated on the SAME
    bf16-rounded inputs; tolerance BF16_SIM_ATOL (derivation next to its definition) on logits of magnitude ~10-60."""
    name = "s1_b64_mix"
    img, words, cap_lens, _ = gi.local_inputs(name)
    ib, wb = g(img).bfloat16(), g(words).bfloat16()
    sim, _, _ = gl().local_similarity(ib, wb, cap_lens, want_attn=False)
    want = orc().local_similarity_matrix(ib.float().cpu(), wb.float().cpu(), cap_lens)
    err = (sim.cpu() - want).abs().max().item()
    print(f"[bf16 {name}] max |sim - oracle| = {err:.4f}")
    assert err < BF16_SIM_ATOL, err
    l_hip = [float(x) for x in gl().dual_cross_entropy(sim)]
    l_ref = [float(x) for x in orc().dual_ce(want)]
    np.testing.assert_allclose(l_hip, l_ref, rtol=2e-2, atol=2e-2)


BF16_CASES = {
    # name: (B, D, H, W, L, cap_lens, no_attn)   -- BASELINE config 5 in ITS dtype, and the ragged multi-tile shape
    # 197 regions (S_pad 256: the non-FULL single-tile kernel in both directions), 256 / 130 / 77 words = sentences of
    # 4 / 3 / 2 word tiles (nsub > 1: two sweeps forward, multi-tile rho backward)
    "cfg5_s197_n256": (3, 768, 14, 14, 256, [256, 130, 77], True),
    # 362 regions (S_pad 384): 96 / 70 / 65 words own a tile pair (long-pair path of the pair kernels, forward and
    # backward); the short ones share an ordinary pair
    "ragged_s362_multitile": (6, 768, 19, 19, 97, [96, 70, 65, 33, 5, 1], True),
    "ragged_s361_pairs": (8, 768, 19, 19, 97, [40, 33, 31, 22, 17, 9, 2, 1], False),
}

# Expected bf16-mode deviation from the fp32 oracle ON THE SAME bf16-ROUNDED INPUTS.  The only extra rounding inside
# K1 is the bf16 image of e2 = exp(temp1 a1) that feeds the second MFMA contraction (relative 2^-9 per element,
# independent signs): Z, <T, c> and |c|^2 are sums over S ~ 200..362 such terms, so each moves by about
# 2^-9 / sqrt(S) ~ 1e-4 relative (the weighted context is dominated by a few regions only for peaked attention, where
# the bound is 2^-9 = 2e-3); cos inherits that, sim = temp3 log sum_w exp(temp2 cos_w) amplifies it by at most
# temp3 temp2 = 50: |d sim| <~ 50 * 2e-3 = 0.1 worst case, ~0.01 typical.  Gradients carry the same relative error
# plus the bf16 rounding of the backward's X / a2 GEMM operands (2^-9 each): ~1 % relative Frobenius worst case.
BF16_SIM_ATOL = 0.02          # observed on MI355X (round 2): 0.002 .. 0.006 over the four bf16 cases
BF16_MAP_RTOL = 2e-2          # attention maps: a2 = e2 / Z with the bf16 image of e2 (2^-8 relative) over the fp32 Z
BF16_GRAD_REL = 0.02          # observed: 0.004 .. 0.007 relative Frobenius error


@pytest.mark.parametrize("name", list(BF16_CASES))
def test_bf16_shapes_forward_backward_vs_oracle(name):
    """bf16 operands at the shapes of BASELINE config 5 and ragged multi-tile captions, forward AND backward, against
    the fp32 oracle on the bf16-rounded inputs (tolerances derived above)."""
    B, D, H, W, L, cap_lens, na_flag = BF16_CASES[name]
    seed = gi.case_seed(name)
    img = torch.from_numpy(gi.normal(seed, B, D, H, W)).bfloat16()
    words = torch.from_numpy(gi.normal(seed + 1, B, D, L)).bfloat16()
    na = torch.from_numpy(gi.normal(seed + 2, D, std=1.0)).bfloat16() if na_flag else None
    ti, tw = img.to(DEV).requires_grad_(True), words.to(DEV).requires_grad_(True)
    tn = None if na is None else na.to(DEV).requires_grad_(True)
    sim, attn, _ = gl().local_similarity(ti, tw, cap_lens, no_attn_vec=tn)
    ri, rw = img.float().requires_grad_(True), words.float().requires_grad_(True)
    rn = None if na is None else na.float().requires_grad_(True)
    want, a2, _ = orc().local_similarity_matrix(ri, rw, cap_lens, no_attn_vec=rn, return_attn=True)
    err = (sim.detach().cpu() - want.detach()).abs().max().item()
    print(f"[bf16 {name}] max |sim - oracle| = {err:.4f}")
    assert err < BF16_SIM_ATOL, err
    shift = 1 if na_flag else 0
    woff = np.concatenate([[0], np.cumsum(cap_lens)])
    flat, off = attn.detach().cpu().numpy(), 0
    for b in range(B):
        n = cap_lens[b]
        ref = a2[b, woff[b]:woff[b] + n, shift:].detach().numpy().reshape(-1)
        np.testing.assert_allclose(flat[off:off + ref.size], ref, rtol=BF16_MAP_RTOL, atol=2e-5)
        off += ref.size
    gsim = torch.from_numpy(gi.normal(seed + 5, *sim.shape, std=1.0))
    (sim * gsim.to(DEV)).sum().backward()
    (want * gsim).sum().backward()
    pairs = [("img", ti.grad, ri.grad), ("words", tw.grad, rw.grad)] + ([] if tn is None else [("no_attn", tn.grad, rn.grad)])
    for label, a, b in pairs:
        a, b = a.float().cpu().numpy(), b.numpy()
        rel = np.linalg.norm(a - b) / np.linalg.norm(b)
        print(f"[bf16 {name}] grad {label}: relative Frobenius error {rel:.4f}")
        assert rel < BF16_GRAD_REL, (label, rel)


def test_bf16_mixed_work_items_forward_backward_vs_oracle():
    """One bf16 plan at 361 regions whose work items are of several kinds at once: a 200-word sentence (four tiles, one
    single-tile-kernel item worked in sweeps), two long pairs (100 and 70 words: one sentence owning two tiles), and two
    ordinary pairs (64 + 64 words; 40 + 33 + 23 + 9 + 5 + 2 + 1 words over two tiles), forward and backward at D = 256 (the
    ordinary pairs' forward runs one workgroup per tile).  sim and both gradients against the oracle on the rounded
    inputs, in the bf16 bands of test_attention_regularisers_vs_oracle."""
    B, D, H, W, L = 12, 256, 19, 19, 200
    cap_lens = [200, 100, 70, 64, 64, 40, 33, 23, 9, 5, 2, 1]
    seed = 4343
    img, words = g(gi.normal(seed, B, D, H, W)).bfloat16(), g(gi.normal(seed + 1, B, D, L)).bfloat16()
    ti, tw = img.clone().requires_grad_(True), words.clone().requires_grad_(True)
    sim, _, _ = gl().local_similarity(ti, tw, cap_lens, want_attn=False)
    ri, rw = img.float().cpu().requires_grad_(True), words.float().cpu().requires_grad_(True)
    want = orc().local_similarity_matrix(ri, rw, cap_lens)
    print(f"[bf16 mixed items] max |sim - oracle| = {(sim.detach().cpu() - want.detach()).abs().max().item():.4f}")
    gsim = torch.from_numpy(gi.normal(seed + 5, *sim.shape, std=1.0))
    (sim * gsim.to(DEV)).sum().backward()
    (want * gsim).sum().backward()
    rels = [(label, np.linalg.norm(a.float().cpu().numpy() - b.numpy()) / np.linalg.norm(b.numpy()))
            for label, a, b in (("img", ti.grad, ri.grad), ("words", tw.grad, rw.grad))]
    for label, rel in rels:
        print(f"[bf16 mixed items] grad {label}: relative Frobenius error {rel:.4f}")
    np.testing.assert_allclose(sim.detach().cpu().numpy(), want.detach().numpy(), rtol=2e-2, atol=2e-3)
    for label, rel in rels:
        assert rel < 0.05, (label, rel)


# ------------------------------------------------------------------ (3) properties at the bench size

def _bench_inputs(B=256, seed=77):
    img = gi.normal(seed, B, 768, 19, 19)
    words = gi.normal(seed + 1, B, 768, 97)
    lens = sorted((int(x) for x in np.random.default_rng(seed + 2).integers(5, 41, size=B)), reverse=True)
    return g(img), g(words), lens


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_properties_b256(dtype):
    img, words, lens = _bench_inputs()
    img, words = img.to(dtype), words.to(dtype)
    f = gl().local_similarity
    sim, _, _ = f(img, words, lens, want_attn=False)
    assert torch.isfinite(sim).all()
    # determinism: bitwise identical on a second launch
    sim2, _, _ = f(img, words, lens, want_attn=False)
    assert torch.equal(sim, sim2)
    # sentence permutation equivariance (different tile packing, same numbers up to rounding)
    perm = torch.randperm(len(lens), generator=torch.Generator().manual_seed(3))
    simp, _, _ = f(img, words[perm.to(DEV)], [lens[i] for i in perm.tolist()], want_attn=False)
    tol = 1e-4 if dtype == torch.float32 else 5e-2
    assert (simp - sim[:, perm.to(DEV)]).abs().max().item() < tol
    # image sharding: block rows computed separately (the data-parallel layout) are the same rows
    rows = [f(img[r * 64:(r + 1) * 64], words, lens, want_attn=False, img_offset=r * 64)[0] for r in range(4)]
    assert torch.equal(torch.cat(rows, 0), sim)
    # loss is at most log(B) + something sane and the CE gradient rows sum to ~0
    l0, l1 = gl().dual_cross_entropy(sim.clone().requires_grad_(True))
    assert torch.isfinite(l0) and torch.isfinite(l1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_b256_rows_vs_oracle(dtype):
    """The bench shape itself (256 x 256 pairs, 19 x 19 regions, the metric's caption lengths: the `k_local_attn_t1`
    launch of 24 064 workgroups and the pair backward) against the oracle, forward AND backward: sim[b, i] depends on
    image b and sentence i only, so the oracle evaluates 24 image rows spread over the batch against ALL 256 sentences
    (a sixteenth of the full CPU cost) and the loss of the comparison touches exactly those rows."""
    img, words, lens = _bench_inputs()
    rows = torch.tensor(sorted({0, 1, 7, 31, 32, 63, 64, 65, 100, 127, 128, 129, 160, 191, 192, 200, 222, 240, 254, 255, 17, 45, 90, 140}))
    assert len(rows) == 24
    ti = img.to(dtype).requires_grad_(True)
    tw = words.to(dtype).requires_grad_(True)
    sim, _, _ = gl().local_similarity(ti, tw, lens, want_attn=False)
    ri = ti.detach()[rows.to(DEV)].float().cpu().requires_grad_(True)
    rw = tw.detach().float().cpu().requires_grad_(True)
    want = orc().local_similarity_matrix(ri, rw, lens)
    got = sim[rows.to(DEV)].detach().float().cpu()
    err = (got - want.detach()).abs().max().item()
    print(f"[{dtype} B=256 rows] max |sim - oracle| = {err:.5f}")
    assert err < (BF16_SIM_ATOL if dtype == torch.bfloat16 else 2e-3), err
    gsim = torch.from_numpy(gi.normal(991, *want.shape, std=1.0))
    weight = torch.zeros(sim.shape, dtype=torch.float32)
    weight[rows] = gsim
    (sim.float() * weight.to(DEV)).sum().backward()
    (want * gsim).sum().backward()
    tol = BF16_GRAD_REL if dtype == torch.bfloat16 else 2e-4
    for label, a, b in (("img rows", ti.grad[rows.to(DEV)], ri.grad), ("words", tw.grad, rw.grad)):
        a, b = a.float().cpu().numpy(), b.numpy()
        rel = np.linalg.norm(a - b) / np.linalg.norm(b)
        print(f"[{dtype} B=256 rows] grad {label}: relative Frobenius error {rel:.5f}")
        assert rel < tol, (label, rel)
    others = torch.ones(256, dtype=torch.bool)
    others[rows] = False
    assert float(ti.grad[others.to(DEV)].abs().max()) == 0.0          # images outside the loss get exactly zero


def test_dual_ce_matches_torch():
    sim = torch.randn(256, 256, device=DEV, generator=torch.Generator(DEV).manual_seed(5)) * 8
    a = sim.clone().requires_grad_(True)
    l0, l1 = gl().dual_cross_entropy(a)
    (1.3 * l0 + 0.7 * l1).backward()
    b = sim.clone().requires_grad_(True)
    lab = torch.arange(256, device=DEV)
    r0 = torch.nn.functional.cross_entropy(b, lab)
    r1 = torch.nn.functional.cross_entropy(b.t(), lab)
    (1.3 * r0 + 0.7 * r1).backward()
    np.testing.assert_allclose([float(l0), float(l1)], [float(r0), float(r1)], rtol=1e-5)
    np.testing.assert_allclose(a.grad.cpu().numpy(), b.grad.cpu().numpy(), rtol=1e-4, atol=1e-7)


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError):
        gl().local_loss(torch.zeros(2, 64, 3, 3), torch.zeros(2, 64, 5), [2, 2])
