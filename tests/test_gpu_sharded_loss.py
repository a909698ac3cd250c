"""The loss kernels on block rows at NON-ZERO image offsets: what a data-parallel rank r > 0 runs.

Rank r owns b_loc images, all-gathers every sentence and calls K1 (LocalSimFn), K6 (glr_attn_reg_*), K4
(glr_attn_sup_fwd) and K2 (glr_dual_ce_*) with img_offset = row0 = first = r * b_loc.  Here the P ranks run one after
another in ONE process, without a process group: a stub stands in for gloria.dist.DistContext and the MODEL'S OWN glue
(GLoRIA.calc_loss -> _calc_local_loss_sharded, GLoRIA._calc_global_loss) makes the calls.  `all_gather_grad` hands
every rank the same full leaf, so autograd sums the ranks' gradients the way the reduce-scatter would.

Two references:
  (A) the same inputs through the unsharded GL.local_loss / attention_supervision_loss: the SAME workgroups do the
      same work, only the grid changes, so the forward quantities are compared bit for bit;
  (B) oracle/gloria_oracle.py in fp64 on the same (rounded) inputs, in the project's bands for the same quantities
      unsharded (the bf16 constants are imported from test_gpu_parity.py).
Cases, caption lengths and the tile plans they rely on: tests/sharded_cases.py (checked on the host by
tests/test_sharded_cases_host.py).  Every result is computed once per case and shared by the tests."""

import functools

import numpy as np
import pytest
import torch

import golden_inputs as gi
import sharded_cases as sc
from test_gpu_parity import BF16_MAP_RTOL, BF16_SIM_ATOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

LOCAL = [(name, D, world, na) for name, c in sc.CASES.items() for D in c["D"] for world in c["worlds"]
         for na in c["no_attn"]]
LOCAL_IDS = [f"{n}-D{D}-P{w}-{'na' if na else 'plain'}" for n, D, w, na in LOCAL]


def _mods():
    from gloria import _native as N
    from gloria.loss import gloria_loss as GL
    from oracle import gloria_oracle as orc
    return N, GL, orc


# ------------------------------------------------------------------ the ranks of one process

class _StubDist:
    """What the sharded glue needs of gloria.dist.DistContext.  all_gather_grad returns the shared full leaf;
    all_gather_ints the full list; all_gather_nograd the concatenation of all ranks' rows, collected in a first pass
    (`collecting`, under no_grad), during which a rank sees its own rows inside a matrix of zeros."""
    active = True

    def __init__(self, world, ints=None):
        self.world_size, self.rank, self.ints = world, 0, ints
        self.full_leaf = None
        self.rows = [None] * world
        self.collecting = True

    def all_gather_grad(self, x):
        assert x.shape[0] * self.world_size == self.full_leaf.shape[0] and x.shape[1:] == self.full_leaf.shape[1:]
        return self.full_leaf

    def all_gather_ints(self, values):
        per = len(self.ints) // self.world_size
        assert list(values) == list(self.ints[self.rank * per:(self.rank + 1) * per])
        return list(self.ints)

    def all_gather_nograd(self, rows):
        if self.collecting:
            assert not torch.is_grad_enabled()
            self.rows[self.rank] = rows.detach().clone()
            n = rows.shape[0]
            full = rows.new_zeros(n * self.world_size, rows.shape[1])
            full[self.rank * n:(self.rank + 1) * n] = rows
            return full
        assert all(r is not None for r in self.rows)
        return torch.cat(self.rows, 0)


def _bare_gloria(dctx, na_param, weights, seg_weight):
    """a GLoRIA without encoders (the way tests/test_dist_gloo.py builds one): only the loss glue is under test"""
    from gloria.models.gloria_model import GLoRIA
    g = GLoRIA.__new__(GLoRIA)
    torch.nn.Module.__init__(g)
    g.dist = dctx
    g.temp1, g.temp2, g.temp3 = sc.TEMPS
    g.no_attn_vec = na_param
    g.local_loss_weight, g.global_loss_weight = 1.0, 0
    g.no_attn_loss_weight, g.attention_divergence_loss_weight, g.attention_entropy_loss_weight = weights
    g.segmentation_loss_weight = seg_weight
    return g


class _Sents(list):
    cap_lens = None


class _Spy:
    """records what the named functions of gloria_loss return while the glue calls them"""

    def __init__(self, GL, *names):
        self.GL, self.names, self.calls, self.orig = GL, names, {n: [] for n in names}, {}

    def __enter__(self):
        for n in self.names:
            self.orig[n] = getattr(self.GL, n)

            def rec(*a, _n=n, **k):
                out = self.orig[_n](*a, **k)
                self.calls[_n].append(out)
                return out
            setattr(self.GL, n, rec)
        return self

    def __exit__(self, *a):
        for n in self.names:
            setattr(self.GL, n, self.orig[n])
        return False


def _leaves(name, D, no_attn):
    img, words, na = sc.inputs(name, D, no_attn)
    li, lw = img.to(DEV).requires_grad_(True), words.to(DEV).requires_grad_(True)
    ln = None if na is None else torch.nn.Parameter(na.to(DEV))
    return li, lw, ln


def _labels(name):
    from gloria.datasets.synthetic import make_batch
    c = sc.CASES[name]
    return make_batch(c["B"], seed=c["seed"] + 9, segmentation=True)["segmentation_labels"]


def _tensor_sum(parts):
    return sum(x for x in parts if torch.is_tensor(x))


def _det(x):
    return x.detach().clone() if torch.is_tensor(x) else x


@functools.lru_cache(maxsize=None)
def _unsharded(name, D, no_attn):
    """(A): the full batch in one call of the unsharded product functions, forward and backward"""
    N, GL, _ = _mods()
    c = sc.CASES[name]
    li, lw, ln = _leaves(name, D, no_attn)
    w = sc.AUX_WEIGHTS[no_attn]
    labels = _labels(name).to(DEV)
    with _Spy(GL, "local_similarity") as spy:
        out = GL.local_loss(li.bfloat16() if c["bf16"] else li, lw, c["cap_lens"], *sc.TEMPS, "sum", ln, *w)
    seg = GL.attention_supervision_loss(out[5], labels)
    (_tensor_sum(out[:5]) + seg).backward()
    (sim, flat, amean), = spy.calls["local_similarity"]
    return dict(sim=_det(sim), flat=_det(flat), amean=_det(amean), parts=[_det(x) for x in out[:5]], seg=_det(seg),
                maps=[_det(m) for m in out[5]], gi=li.grad, gw=lw.grad, gn=None if ln is None else ln.grad)


def _run_rank(name, D, no_attn, dctx, r, li, lw, ln, channels_last=False):
    """rank r of `dctx.world_size` through GLoRIA.calc_loss; with grad enabled also its backward into the leaves"""
    N, GL, _ = _mods()
    c = sc.CASES[name]
    b_loc = c["B"] // dctx.world_size
    sl = slice(r * b_loc, (r + 1) * b_loc)
    dctx.rank, dctx.full_leaf = r, lw
    g = _bare_gloria(dctx, ln, sc.AUX_WEIGHTS[no_attn], 1.0)
    img = li[sl].bfloat16() if c["bf16"] else li[sl]
    if channels_last:
        img = img.contiguous(memory_format=torch.channels_last)
        assert not img.is_contiguous()
    sents = _Sents()
    sents.cap_lens = c["cap_lens"][sl]
    labels = _labels(name)[sl].to(DEV)
    parts = []
    inner = g._calc_local_loss_sharded
    g._calc_local_loss_sharded = lambda *a: (parts.append(inner(*a)), parts[-1])[1]
    with _Spy(GL, "local_similarity", "attention_supervision_loss") as spy:
        loss, maps = g.calc_loss(img, None, lw[sl], None, sents, labels)
    if torch.is_grad_enabled():
        loss.backward()
    (sim, flat, amean), = spy.calls["local_similarity"]
    (seg,) = spy.calls["attention_supervision_loss"]
    assert maps.flat is flat and maps.first == r * b_loc and len(maps) == b_loc
    return dict(sim=_det(sim), flat=_det(flat), amean=_det(amean), parts=[_det(x) for x in parts[0][:5]],
                seg=_det(seg) / dctx.world_size, maps=[_det(m) for m in maps], loss=_det(loss))


@functools.lru_cache(maxsize=None)
def _collected(name, D, world, no_attn):
    """first pass, under no_grad: every rank's block of similarity rows (what all_gather_nograd delivers later)"""
    c = sc.CASES[name]
    dctx = _StubDist(world, c["cap_lens"])
    li, lw, ln = _leaves(name, D, no_attn)
    with torch.no_grad():
        for r in range(world):
            _run_rank(name, D, no_attn, dctx, r, li, lw, ln)
    dctx.collecting = False
    return dctx


@functools.lru_cache(maxsize=None)
def _sharded(name, D, world, no_attn):
    """second pass: every rank's forward and backward; the leaves end with the sum of the ranks' gradients"""
    dctx = _collected(name, D, world, no_attn)
    li, lw, ln = _leaves(name, D, no_attn)
    ranks = [_run_rank(name, D, no_attn, dctx, r, li, lw, ln) for r in range(world)]
    return dict(ranks=ranks, gi=li.grad, gw=lw.grad, gn=None if ln is None else ln.grad)


@functools.lru_cache(maxsize=None)
def _oracle(name, D, no_attn):
    """(B): fp64 on the CPU, on the same (bf16-representable where the case is bf16) inputs"""
    _, _, orc = _mods()
    c = sc.CASES[name]
    img, words, na = sc.inputs(name, D, no_attn)
    ri, rw = img.double().requires_grad_(True), words.double().requires_grad_(True)
    rn = None if na is None else na.double().requires_grad_(True)
    out = orc.local_loss(ri, rw, c["cap_lens"], *sc.TEMPS, "sum", rn, *sc.AUX_WEIGHTS[no_attn], return_sim=True)
    seg = orc.attention_supervision_loss(out[5], _labels(name), 1.0)
    (_tensor_sum(out[:5]) + seg).backward()
    return dict(sim=out[6].detach(), parts=[float(x) for x in out[:5]], seg=float(seg),
                maps=[m.detach() for m in out[5]], gi=ri.grad, gw=rw.grad, gn=None if rn is None else rn.grad)


def _map_segment(c, r, world):
    """[start, end) of rank r's diagonal maps inside the flat buffer (the no-attention column is stripped)"""
    b_loc = c["B"] // world
    off = np.concatenate([[0], np.cumsum(np.asarray(c["cap_lens"], dtype=np.int64) * c["H"] * c["W"])])
    return int(off[r * b_loc]), int(off[(r + 1) * b_loc])


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


# ------------------------------------------------------------------ exact checks against (A)

@pytest.mark.parametrize("name,D,world,no_attn", LOCAL, ids=LOCAL_IDS)
def test_rank_forward_is_bitwise_the_unsharded_block(name, D, world, no_attn):
    """sim rows, the diagonal map segment (and zeros everywhere else in the flat buffer), the word-mean attention rows
    and both contrastive losses of every rank, bit for bit against the unsharded call"""
    c = sc.CASES[name]
    full, sh = _unsharded(name, D, no_attn), _sharded(name, D, world, no_attn)
    b_loc = c["B"] // world
    s_eff = c["H"] * c["W"] + (1 if no_attn else 0)
    for r, rk in enumerate(sh["ranks"]):
        sl = slice(r * b_loc, (r + 1) * b_loc)
        assert torch.equal(rk["sim"], full["sim"][sl]), f"rank {r}: sim rows"
        a, e = _map_segment(c, r, world)
        assert rk["flat"].shape == full["flat"].shape
        assert torch.equal(rk["flat"][a:e], full["flat"][a:e]), f"rank {r}: diagonal maps"
        assert float(rk["flat"][a:e].min()) > 0.0                               # ... and they were written at all
        assert not rk["flat"][:a].any() and not rk["flat"][e:].any(), f"rank {r}: maps of other ranks' images"
        assert torch.equal(rk["amean"][:, :, :s_eff], full["amean"][sl][:, :, :s_eff]), f"rank {r}: amean rows"
        assert torch.equal(rk["parts"][0], full["parts"][0]) and torch.equal(rk["parts"][1], full["parts"][1]), \
            f"rank {r}: l0 / l1 {rk['parts'][:2]} vs {full['parts'][:2]}"
        for k, m in enumerate(rk["maps"]):
            assert torch.equal(m, full["maps"][r * b_loc + k])


@pytest.mark.parametrize("name,D,world,no_attn", LOCAL, ids=LOCAL_IDS)
def test_regulariser_kernels_on_block_rows_are_bitwise(name, D, world, no_attn):
    """K6 called directly with img_offset = r * b_loc on the rank's amean rows: `out` rows and `damean` rows against
    the rows of the full call"""
    N, GL, _ = _mods()
    L = N.lib()
    c = sc.CASES[name]
    amean = _unsharded(name, D, no_attn)["amean"].contiguous()
    B, n_sent, s_pad = amean.shape
    shift = 1 if no_attn else 0
    s_eff = c["H"] * c["W"] + shift
    coef = torch.tensor([0.7, -0.3, 1.1 if no_attn else 0.0], device=DEV)

    def run(a, off):
        a = a.contiguous()
        out = torch.full((a.shape[0], 4), 3.0, device=DEV)
        dam = torch.full_like(a, 3.0)
        assert L.glr_attn_reg_fwd(N.ptr(a), a.shape[0], n_sent, s_pad, s_eff, shift, off, N.ptr(out), N.stream()) == 0
        assert L.glr_attn_reg_bwd(N.ptr(a), a.shape[0], n_sent, s_pad, s_eff, shift, off, N.ptr(coef), N.ptr(dam),
                                  N.stream()) == 0
        return out, dam

    # without the extra column the no-attention score is log(1 - 1) (never used: its weight is None): not compared
    cols = [0, 1, 2, 3] if no_attn else [0, 1, 3]
    out_full, dam_full = run(amean, 0)
    assert torch.isfinite(out_full[:, cols]).all() and torch.isfinite(dam_full).all()
    b_loc = B // world
    for r in range(world):
        sl = slice(r * b_loc, (r + 1) * b_loc)
        out, dam = run(amean[sl], r * b_loc)
        assert torch.equal(out[:, cols], out_full[sl][:, cols]), f"rank {r}: glr_attn_reg_fwd"
        assert torch.equal(dam, dam_full[sl]), f"rank {r}: glr_attn_reg_bwd"
    if world > 1:       # the offset matters: rank 1's rows read with rank 0's diagonal give another divergence term
        out, _ = run(amean[b_loc:2 * b_loc], 0)
        assert not torch.equal(out[:, 1], out_full[b_loc:2 * b_loc, 1])


@pytest.mark.parametrize("name,D,world,no_attn", LOCAL, ids=LOCAL_IDS)
def test_supervision_kernel_on_block_rows_is_bitwise(name, D, world, no_attn):
    """K4 called directly with first = r * b_loc: loss_b and the dmap segment against the full call; nothing outside
    the rank's segment is written"""
    N, GL, _ = _mods()
    c = sc.CASES[name]
    flat = _unsharded(name, D, no_attn)["flat"].contiguous()
    labels = _labels(name).to(DEV).to(torch.uint8).contiguous()
    cl = np.asarray(c["cap_lens"], dtype=np.int64)
    off = np.zeros(len(cl) + 1, dtype=np.int64)
    np.cumsum(cl * c["H"] * c["W"], out=off[1:])
    off_d, cl_d = torch.from_numpy(off[:-1].copy()).to(DEV), torch.from_numpy(cl.astype(np.int32)).to(DEV)

    def run(first, count):
        lab = labels[first:first + count].contiguous()
        loss_b = torch.full((count,), -7.0, device=DEV)
        dmap = torch.zeros_like(flat)
        assert N.lib().glr_attn_sup_fwd(N.ptr(flat), N.ptr(off_d), N.ptr(cl_d), first, N.ptr(lab), count, lab.shape[1],
                                        lab.shape[2], c["H"], c["W"], N.ptr(loss_b), N.ptr(dmap), N.stream()) == 0
        return loss_b, dmap

    loss_full, dmap_full = run(0, c["B"])
    assert torch.isfinite(loss_full).all() and dmap_full.abs().sum() > 0
    b_loc = c["B"] // world
    for r in range(world):
        loss_b, dmap = run(r * b_loc, b_loc)
        a, e = _map_segment(c, r, world)
        assert torch.equal(loss_b, loss_full[r * b_loc:(r + 1) * b_loc]), f"rank {r}: loss_b"
        assert torch.equal(dmap[a:e], dmap_full[a:e]), f"rank {r}: dmap"
        assert not dmap[:a].any() and not dmap[e:].any(), f"rank {r}: dmap outside the rank's maps"


@pytest.mark.parametrize("name,D,world,no_attn", LOCAL, ids=LOCAL_IDS)
def test_dual_ce_backward_block_rows_of_the_local_matrix_are_bitwise(name, D, world, no_attn):
    N, GL, _ = _mods()
    sim = _unsharded(name, D, no_attn)["sim"].contiguous()
    B = sim.shape[0]
    full = _dual_ce_bwd(N, sim, 0, B)
    for r in range(world):
        b_loc = B // world
        assert torch.equal(_dual_ce_bwd(N, sim, r * b_loc, b_loc), full[r * b_loc:(r + 1) * b_loc]), f"rank {r}"


def _dual_ce_bwd(N, sim, row0, n_rows, g=(1.3, 0.7)):
    L = N.lib()
    B = sim.shape[0]
    lse = torch.empty(2, B, device=DEV)
    losses = torch.empty(2, device=DEV)
    assert L.glr_dual_ce_fwd(N.ptr(sim), B, N.ptr(lse[0]), N.ptr(lse[1]), N.ptr(losses), N.stream()) == 0
    gt = torch.tensor(g, device=DEV)
    dsim = torch.full((n_rows, B), 5.0, device=DEV)
    assert L.glr_dual_ce_bwd(N.ptr(sim), B, N.ptr(lse[0]), N.ptr(lse[1]), N.ptr(gt), row0, n_rows, N.ptr(dsim),
                             N.stream()) == 0
    return dsim


# ------------------------------------------------------------------ banded checks against (B)

@pytest.mark.parametrize("name,D,world,no_attn", LOCAL, ids=LOCAL_IDS)
def test_ranks_against_the_fp64_oracle(name, D, world, no_attn):
    """Every rank's sim rows, maps and losses, the summed regulariser / supervision shares and the gradients of the
    summed loss (image, words, no-attention vector; summed over the ranks) against the oracle, in the bands the
    project uses for the same quantities unsharded.  bf16: the gradient band is applied per image and per sentence
    too, so one wrong diagonal is not diluted by the rest of the tensor.  Observed on an MI355X, bf16 cases: max |sim -
    oracle| 0.005 .. 0.008, gradients 0.003 .. 0.008 relative Frobenius per tensor, worst single image / sentence
    0.0134; fp32 cases: max |sim - oracle| below 1e-5."""
    c = sc.CASES[name]
    sh, ref = _sharded(name, D, world, no_attn), _oracle(name, D, no_attn)
    f32 = not c["bf16"]
    b_loc = c["B"] // world
    tag = f"[{name} D={D} P={world} no_attn={no_attn}]"
    for r, rk in enumerate(sh["ranks"]):
        sl = slice(r * b_loc, (r + 1) * b_loc)
        got, want = rk["sim"].double().cpu().numpy(), ref["sim"][sl].numpy()
        print(f"{tag} rank {r}: max |sim - oracle| = {np.abs(got - want).max():.3e}")
        if f32:
            np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4)
        else:
            assert np.abs(got - want).max() < BF16_SIM_ATOL
        for k, m in enumerate(rk["maps"]):
            np.testing.assert_allclose(m.double().cpu().numpy(), ref["maps"][r * b_loc + k].numpy(),
                                       rtol=1e-4 if f32 else BF16_MAP_RTOL, atol=1e-6 if f32 else 2e-5,
                                       err_msg=f"rank {r}: map of image {r * b_loc + k}")
        np.testing.assert_allclose([float(rk["parts"][0]), float(rk["parts"][1])], ref["parts"][:2],
                                   rtol=1e-4 if f32 else 2e-2, atol=1e-5 if f32 else 2e-3)
    for k in (2, 3, 4):                                  # no-attention, divergence, entropy: the ranks' shares add up
        if torch.is_tensor(sh["ranks"][0]["parts"][k]):
            share = sum(float(rk["parts"][k]) for rk in sh["ranks"])
            print(f"{tag} regulariser {k}: {share:.6f} vs {ref['parts'][k]:.6f}")
            np.testing.assert_allclose(share, ref["parts"][k], rtol=1e-4 if f32 else 2e-2, atol=1e-5 if f32 else 2e-3)
    seg = sum(float(rk["seg"]) for rk in sh["ranks"])
    print(f"{tag} supervision: {seg:.6f} vs {ref['seg']:.6f}")
    np.testing.assert_allclose(seg, ref["seg"], rtol=1e-4 if f32 else 2e-2)
    pairs = [("img", sh["gi"], ref["gi"]), ("words", sh["gw"], ref["gw"])]
    if no_attn:
        pairs.append(("no_attn", sh["gn"], ref["gn"]))
    for label, a, b in pairs:
        assert a.dtype == torch.float32
        if f32:
            np.testing.assert_allclose(a.double().cpu().numpy(), b.numpy(), rtol=2e-3, atol=1e-5, err_msg=label)
            continue
        slices = [(label, a, b)]
        if label != "no_attn":
            slices += [(f"{label}[{i}]", a[i], b[i]) for i in range(c["B"])]
        worst = max((_rel(x, y), n) for n, x, y in slices)
        print(f"{tag} grad {label}: relative Frobenius error {_rel(a, b):.4f}, worst slice {worst[1]} {worst[0]:.4f}")
        for n, x, y in slices:
            assert _rel(x, y) < 0.05, (n, _rel(x, y))


BF16_FULL = [t for t in LOCAL if t[0] == "full_bf16"]


@pytest.mark.parametrize("name,D,world,no_attn", BF16_FULL, ids=[i for t, i in zip(LOCAL, LOCAL_IDS) if t in BF16_FULL])
def test_bf16_sharded_gradients_are_as_close_to_fp64_as_the_unsharded_ones(name, D, world, no_attn):
    """E = relative Frobenius error against the fp64 oracle; E_sharded <= 1.5 E_unsharded per tensor and per image
    slice.  Margin: the precedent of test_encoder_on_real_rows_is_as_close_to_fp32_as_the_padded_path - identical
    arithmetic up to summation order (a rank's word / no-attention gradients are fp32 partial sums over its images).

    Observed on an MI355X (E_sharded / E_unsharded, ratio):
      D = 256   img      0.007578 / 0.007578  1.0000      D = 128   img      0.006258 / 0.006258  1.0000
                words    0.007078 / 0.007102  0.9966                words    0.005752 / 0.005686  1.0117
                no_attn  0.003353 / 0.003353  1.0000                no_attn  0.004458 / 0.004458  1.0000
      img[b], b = 0 .. 14, the same in both runs to all six printed digits (ratio 1.0000 for every image):
      D = 256   .007986 .013161 .005692 .006037 .006939 .006777 .007315 .006106 .006262 .010138 .005885 .006384
                .006046 .007373 .011508
      D = 128   .006749 .006634 .013439 .003827 .006865 .006193 .006661 .006516 .006688 .008593 .004475 .005547
                .004243 .005785 .006165
    An image's gradient comes from one rank only and is rounded to bf16 once in either run; only the word gradient,
    the sum of three fp32 partial GEMMs instead of one, moves at all (by about 1 %)."""
    c = sc.CASES[name]
    sh, full, ref = _sharded(name, D, world, no_attn), _unsharded(name, D, no_attn), _oracle(name, D, no_attn)
    rows = [("img", sh["gi"], full["gi"], ref["gi"]), ("words", sh["gw"], full["gw"], ref["gw"]),
            ("no_attn", sh["gn"], full["gn"], ref["gn"])]
    rows += [(f"img[{b}]", sh["gi"][b], full["gi"][b], ref["gi"][b]) for b in range(c["B"])]
    table = [(n, _rel(s, r), _rel(u, r)) for n, s, u, r in rows]
    print(f"\n[{name} D={D} P={world}] E_sharded  E_unsharded  ratio")
    for n, es, eu in table:
        print(f"  {n:8s} {es:.6f}  {eu:.6f}  {es / eu:.4f}")
    for n, es, eu in table:
        assert es <= 1.5 * eu, (n, es, eu)


# ------------------------------------------------------------------ channels-last features

def test_channels_last_features_give_bitwise_the_contiguous_rank():
    """Rank 1 of full_bf16 (D = 256) with the bf16 image tensor in channels_last - the layout the image encoder hands
    over: the layout = 1 branch of glr_pack_regions_tiled and the strided d_img view LocalSimFn.backward returns for
    every channels-last input of the operand dtype.  vt is bit-identical, and the d_img route differs only by an exact bf16 -> fp32 -> bf16 round trip, so sim, maps and all
    three gradients equal the contiguous run bit for bit."""
    name, D, world, no_attn = "full_bf16", 256, 3, True
    dctx = _collected(name, D, world, no_attn)
    res = []
    for cl in (False, True):
        li, lw, ln = _leaves(name, D, no_attn)
        rk = _run_rank(name, D, no_attn, dctx, 1, li, lw, ln, channels_last=cl)
        res.append((rk, li.grad, lw.grad, ln.grad))
    (a, ai, aw, an), (b, bi, bw, bn) = res
    assert float(ai[5:10].abs().max()) > 0 and float(ai[:5].abs().max()) == 0 and float(ai[10:].abs().max()) == 0
    assert torch.equal(a["sim"], b["sim"]), "sim"
    assert torch.equal(a["flat"], b["flat"]), "maps"
    assert torch.equal(a["amean"], b["amean"]), "amean"
    assert torch.equal(a["loss"], b["loss"]), "loss"
    for label, x, y in (("d_img", ai, bi), ("d_words", aw, bw), ("d_no_attn", an, bn)):
        assert torch.equal(x, y), (label, float((x - y).abs().max()), int((x != y).sum()))


# ------------------------------------------------------------------ global path

def test_global_loss_block_rows_against_the_fp64_oracle():
    """GLoRIA._calc_global_loss per rank (K3 on block rows of a 15 x 15 matrix at D = 100, K2 with row0 = r * 5):
    losses and summed gradients against fp64 oracle.global_loss, in the bands of
    test_global_similarity_rectangular_vs_oracle"""
    _, _, orc = _mods()
    B, D, world = 15, 100, 3
    img, txt = torch.from_numpy(gi.normal(7401, B, D)), torch.from_numpy(gi.normal(7402, B, D))
    li, lt = img.to(DEV).requires_grad_(True), txt.to(DEV).requires_grad_(True)
    dctx = _StubDist(world)
    dctx.full_leaf = lt
    g = _bare_gloria(dctx, None, (None, None, None), None)
    b_loc = B // world
    with torch.no_grad():
        for r in range(world):
            dctx.rank = r
            g._calc_global_loss(li[r * b_loc:(r + 1) * b_loc], lt[r * b_loc:(r + 1) * b_loc])
    dctx.collecting = False
    losses = []
    for r in range(world):
        dctx.rank = r
        g0, g1 = g._calc_global_loss(li[r * b_loc:(r + 1) * b_loc], lt[r * b_loc:(r + 1) * b_loc])
        (g0 + g1).backward()
        losses.append((float(g0), float(g1)))
    ri, rt = img.double().requires_grad_(True), txt.double().requires_grad_(True)
    r0, r1 = orc.global_loss(ri, rt, temp3=sc.TEMPS[2])
    (r0 + r1).backward()
    sim = torch.cat(dctx.rows, 0).double().cpu().numpy()
    want = orc.global_similarity_matrix(img.double(), txt.double(), temp3=sc.TEMPS[2]).numpy()
    np.testing.assert_allclose(sim, want, rtol=1e-5, atol=1e-5)
    for r in range(world):
        assert losses[r] == losses[0]                                        # the same matrix on every rank
        np.testing.assert_allclose(losses[r], [float(r0), float(r1)], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(li.grad.double().cpu().numpy(), ri.grad.numpy(), rtol=1e-4, atol=1e-6)
    scale = np.abs(rt.grad.numpy()).max()
    np.testing.assert_allclose(lt.grad.double().cpu().numpy() / scale, rt.grad.numpy() / scale, atol=1e-5)


# ------------------------------------------------------------------ K2 alone

@pytest.mark.parametrize("B,row0,n_rows", [(15, 5, 5), (300, 37, 100)])
def test_dual_ce_odd_and_beyond_one_loop_trip(B, row0, n_rows):
    """K2 at an odd B and at B = 300 (the second trip of the kernels' `j += 256` loops) with sim ~ 8 N(0, 1): losses
    and the full gradient against fp64 cross entropy of sim and sim^T (bands of test_dual_ce_matches_torch), block rows
    against rows of the full backward, and the argument checks of glr_dual_ce_bwd"""
    N, GL, _ = _mods()
    sim = torch.from_numpy(gi.normal(7500 + B, B, B, std=8.0))
    a = sim.to(DEV).requires_grad_(True)
    l0, l1 = GL.dual_cross_entropy(a)
    (1.3 * l0 + 0.7 * l1).backward()
    b = sim.double().requires_grad_(True)
    lab = torch.arange(B)
    r0 = torch.nn.functional.cross_entropy(b, lab)
    r1 = torch.nn.functional.cross_entropy(b.t(), lab)
    (1.3 * r0 + 0.7 * r1).backward()
    np.testing.assert_allclose([float(l0), float(l1)], [float(r0), float(r1)], rtol=1e-5)
    np.testing.assert_allclose(a.grad.double().cpu().numpy(), b.grad.numpy(), rtol=1e-4, atol=1e-7)
    s = sim.to(DEV).contiguous()
    full = _dual_ce_bwd(N, s, 0, B)
    assert torch.equal(full, a.grad)
    assert torch.equal(_dual_ce_bwd(N, s, row0, n_rows), full[row0:row0 + n_rows])
    # rows outside the matrix are refused before anything is written
    L = N.lib()
    lse, gt = torch.zeros(2, B, device=DEV), torch.ones(2, device=DEV)
    for bad0, bad_n in ((B - n_rows + 1, n_rows), (-1, n_rows), (B, 1)):
        canary = torch.full((n_rows, B), 42.0, device=DEV)
        rc = L.glr_dual_ce_bwd(N.ptr(s), B, N.ptr(lse[0]), N.ptr(lse[1]), N.ptr(gt), bad0, bad_n, N.ptr(canary), N.stream())
        assert rc != 0, (bad0, bad_n)
        torch.cuda.synchronize()
        assert bool((canary == 42.0).all())


# ------------------------------------------------------------------ argument check of the K1 forward

@pytest.mark.parametrize("pair_only", [0, 1])
def test_k1_forward_refuses_a_negative_image_offset(pair_only):
    """glr_local_attn_fwd returns GLR_EINVAL for img_offset < 0 before any launch (in pair-only mode the kernel would
    index sent_slot0 in front of the array): sim keeps its canary"""
    N, GL, _ = _mods()
    B, D, L_ = 2, 64, 6
    cap_lens = [6, 6]
    img = torch.from_numpy(gi.normal(7601, B, D, 3, 3)).to(DEV)
    words = torch.from_numpy(gi.normal(7602, B, D, L_)).to(DEV)
    o = GL._Opts(*sc.TEMPS, "sum", 1e-8, False, -1, 0)
    p = GL._pack_operands(img, words, None, cap_lens, o.word_start)
    plan = p.plan
    sim = torch.full((B, plan.n_sent), 42.0, device=DEV)

    def fwd(offset):
        return N.lib().glr_local_attn_fwd(*GL._k1_args(p, B, D, o), N.ptr(sim), plan.n_sent, None, None, None, None, 0,
                                          pair_only, offset, None, None, p.code, N.stream())
    for offset in (-1, -B):
        assert fwd(offset) == -1                       # GLR_EINVAL
        torch.cuda.synchronize()
        assert bool((sim == 42.0).all())
    assert fwd(0) == 0                                 # the same arguments at offset 0 are a valid call
    torch.cuda.synchronize()
    want = sim.diagonal() if pair_only else sim
    assert bool((want != 42.0).all()) and bool(torch.isfinite(sim).all())
