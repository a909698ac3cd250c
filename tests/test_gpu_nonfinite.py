"""Steps with non-finite gradients on the GPU: the guarded norm / guard / Adam kernels (include/glr.h glr_*_g,
glr_step_guard), ShadowAdam's skip (bitwise equal to never having taken the step), the trainer's policy (skip, raise,
the consecutive limit, dropping the encoder graphs), the stock fp32 path and checkpoints."""

import ctypes
import json

import numpy as np
import pytest
import torch

from gloria import _native as N
from gloria import nonfinite as NF

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INF = float("inf")


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def beq(a, b):
    return torch.equal(bits(a), bits(b))


def bias_table(b1, b2, cap=64):
    host = np.zeros(2 * cap, dtype=np.float32)
    N.check(N.lib().glr_adam_bias_table(b1, b2, cap, host.ctypes.data_as(ctypes.c_void_p)), "glr_adam_bias_table")
    return torch.from_numpy(host).to(DEV), cap


def chunk_table(numels, chunk):
    ent, off = [], 0
    for i, n in enumerate(numels):
        for c0 in range(0, n, chunk):
            ent.append((i, min(chunk, n - c0), c0, off + c0))
        off += (n + 7) // 8 * 8
    tab = np.zeros(len(ent), dtype=np.dtype([("param", "<i4"), ("count", "<i4"), ("poff", "<i8"), ("foff", "<i8")]))
    for k, e in enumerate(ent):
        tab[k] = e
    return torch.from_numpy(tab.view(np.uint8).copy()).to(DEV), ent, off


# ---------------------------------------------------------------- 1. kernels
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_flat_sumsq_guard_counts_and_locates(dtype):
    L, st = N.lib(), N.stream()
    n = 8 * 256 * 8 * 5 + 24
    nb = L.glr_sumsq_blocks(n)
    assert nb > 1
    g = torch.Generator(DEV).manual_seed(3)
    x = torch.randn(n, device=DEV, generator=g).to(dtype)
    bad = {50000: INF, 1000: -INF, 70001: float("nan")}
    for i, v in bad.items():
        x[i] = v
    pu = torch.zeros(nb, device=DEV)
    pg = torch.full((nb,), 7.0, device=DEV)
    nf = torch.full((2 * nb,), 99, dtype=torch.int64, device=DEV)
    N.check(L.glr_sumsq_partial(N.ptr(x), N.dtype_code(dtype), n, N.ptr(pu), st), "plain")
    N.check(L.glr_sumsq_partial_g(N.ptr(x), N.dtype_code(dtype), n, N.ptr(pg), N.ptr(nf), st), "guarded")
    ok = torch.isfinite(pu)
    assert beq(pg[ok], pu[ok]) and bool((~torch.isfinite(pg) == ~ok).all())
    per = ((n // 8 + nb - 1) // nb) * 8
    want = np.zeros(2 * nb, dtype=np.int64)
    want[1::2] = -1
    for b in range(nb):
        mine = sorted(i for i in bad if b * per <= i < min(b * per + per, n))
        if mine:
            want[2 * b], want[2 * b + 1] = len(mine), mine[0]
    assert np.array_equal(nf.cpu().numpy(), want)
    # the guard: clip_state as glr_clip_coef (bitwise), the step skipped, the first bad element named
    out_u = torch.zeros(2, device=DEV)
    out_g = torch.zeros(2, device=DEV)
    rec = torch.zeros(NF.RECORD_WORDS, dtype=torch.int64, device=DEV)
    rec[NF.APPLIED] = 4
    N.check(L.glr_clip_coef(N.ptr(pu), nb, 0.25, N.ptr(out_u), st), "clip")
    N.check(L.glr_step_guard(N.ptr(pg), N.ptr(nf), nb, 0.25, N.ptr(out_g), N.ptr(rec), 7, st), "guard")
    assert beq(out_g, out_u)
    r = rec.tolist()
    assert r[NF.APPLIED] == 4 and r[NF.SKIPPED] == 1 and r[NF.CONSECUTIVE] == 1 and r[NF.SKIP] == 1
    assert r[NF.LAST_CALL] == 7 and r[NF.LAST_COUNT] == 3 and r[NF.LAST_PARTIAL] == 1000 // per
    assert r[NF.LAST_OFFSET] == 1000 and r[NF.LONGEST] == 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pointer_table_sumsq_guard_counts_and_locates(dtype):
    from gloria.optim import CHUNK
    L, st = N.lib(), N.stream()
    numels = [100, 20000, 37, CHUNK + 8]
    table, ent, _ = chunk_table(numels, CHUNK)
    g = torch.Generator(DEV).manual_seed(4)
    grads = [torch.randn(k, device=DEV, generator=g).to(dtype) for k in numels]
    bad = {(1, 16390): INF, (1, 16385): -INF, (2, 36): float("nan"), (3, CHUNK): float("nan"), (3, 5): INF}
    for (p, i), v in bad.items():
        grads[p][i] = v
    ptrs = torch.tensor([t.data_ptr() for t in grads], dtype=torch.int64, device=DEV)
    nc = len(ent)
    pu, pg = torch.zeros(nc, device=DEV), torch.zeros(nc, device=DEV)
    nf = torch.full((2 * nc,), 99, dtype=torch.int64, device=DEV)
    N.check(L.glr_sumsq_mt(N.ptr(table), nc, N.ptr(ptrs), N.dtype_code(dtype), N.ptr(pu), st), "plain")
    N.check(L.glr_sumsq_mt_g(N.ptr(table), nc, N.ptr(ptrs), N.dtype_code(dtype), N.ptr(pg), N.ptr(nf), st), "guarded")
    ok = torch.isfinite(pu)
    assert beq(pg[ok], pu[ok]) and bool((~torch.isfinite(pg) == ~ok).all())
    want = []
    for (p, count, poff, _) in ent:
        mine = sorted(i - poff for (q, i) in bad if q == p and poff <= i < poff + count)
        want += [len(mine), mine[0]] if mine else [0, -1]
    assert nf.tolist() == want
    out_g = torch.zeros(2, device=DEV)
    rec = torch.zeros(NF.RECORD_WORDS, dtype=torch.int64, device=DEV)
    N.check(L.glr_step_guard(N.ptr(pg), N.ptr(nf), nc, 0.25, N.ptr(out_g), N.ptr(rec), 3, st), "guard")
    r = rec.tolist()
    first = next(k for k in range(nc) if want[2 * k])
    assert r[NF.SKIP] == 1 and r[NF.LAST_COUNT] == len(bad) and r[NF.LAST_PARTIAL] == first
    layout = [NF.group_layout(numels, chunk=CHUNK)]
    assert NF.locate(layout, r[NF.LAST_PARTIAL], r[NF.LAST_OFFSET]) == (0, 1, 16385)


@pytest.mark.parametrize("form", ["flat", "table"])
def test_finite_overflowing_norm_is_not_skipped(form):
    """all elements finite, the sum of squares overflows: NOT skipped; coefficient 0 and the step equals the plain one"""
    L, st = N.lib(), N.stream()
    n = 4096
    grad = torch.full((n,), 3e38, device=DEV)
    grad[::3] = -3e38
    g = torch.Generator(DEV).manual_seed(5)
    bufs = [torch.randn(n, device=DEV, generator=g) for _ in range(2)]       # two copies of (master, m, v, shadow)
    sets = []
    for _ in range(2):
        sets.append([bufs[0].clone(), bufs[1].clone() * 0.1, bufs[1].clone().abs() * 0.01,
                     torch.zeros(n, dtype=torch.bfloat16, device=DEV)])
    if form == "flat":
        nb = L.glr_sumsq_blocks(n)
        pu, pg = torch.zeros(nb, device=DEV), torch.zeros(nb, device=DEV)
        nf = torch.zeros(2 * nb, dtype=torch.int64, device=DEV)
        N.check(L.glr_sumsq_partial(N.ptr(grad), 0, n, N.ptr(pu), st), "plain")
        N.check(L.glr_sumsq_partial_g(N.ptr(grad), 0, n, N.ptr(pg), N.ptr(nf), st), "guarded")
    else:
        table, ent, _ = chunk_table([n], 1024)
        ptrs = torch.tensor([grad.data_ptr()], dtype=torch.int64, device=DEV)
        nb = len(ent)
        pu, pg = torch.zeros(nb, device=DEV), torch.zeros(nb, device=DEV)
        nf = torch.zeros(2 * nb, dtype=torch.int64, device=DEV)
        N.check(L.glr_sumsq_mt(N.ptr(table), nb, N.ptr(ptrs), 0, N.ptr(pu), st), "plain")
        N.check(L.glr_sumsq_mt_g(N.ptr(table), nb, N.ptr(ptrs), 0, N.ptr(pg), N.ptr(nf), st), "guarded")
    out_u, out_g = torch.zeros(2, device=DEV), torch.zeros(2, device=DEV)
    rec = torch.zeros(NF.RECORD_WORDS, dtype=torch.int64, device=DEV)
    N.check(L.glr_clip_coef(N.ptr(pu), nb, 0.25, N.ptr(out_u), st), "clip")
    N.check(L.glr_step_guard(N.ptr(pg), N.ptr(nf), nb, 0.25, N.ptr(out_g), N.ptr(rec), 1, st), "guard")
    assert beq(out_g, out_u) and float(out_g[0]) == INF and float(out_g[1]) == 0.0
    assert rec[NF.SKIP].item() == 0 and rec[NF.APPLIED].item() == 1 and rec[NF.SKIPPED].item() == 0
    bias, cap = bias_table(0.5, 0.999)
    hyper = (1e-2, 0.5, 0.999, 1e-8, 1e-3)
    (mu, au, vu, su), (mg, ag, vg, sg) = sets
    if form == "flat":
        N.check(L.glr_adam_step(N.ptr(mu), N.ptr(au), N.ptr(vu), N.ptr(grad), 0, N.ptr(su), n, *hyper, 1, N.ptr(out_u),
                                st), "adam")
        N.check(L.glr_adam_step_g(N.ptr(mg), N.ptr(ag), N.ptr(vg), N.ptr(grad), 0, N.ptr(sg), n, *hyper, N.ptr(bias), cap,
                                  N.ptr(rec), N.ptr(out_g), st), "adam_g")
    else:
        N.check(L.glr_adam_step_mt(N.ptr(table), nb, N.ptr(ptrs), 0, N.ptr(mu), N.ptr(au), N.ptr(vu), N.ptr(su), *hyper, 1,
                                   N.ptr(out_u), st), "adam_mt")
        N.check(L.glr_adam_step_mt_g(N.ptr(table), nb, N.ptr(ptrs), 0, N.ptr(mg), N.ptr(ag), N.ptr(vg), N.ptr(sg), *hyper,
                                     N.ptr(bias), cap, N.ptr(rec), N.ptr(out_g), st), "adam_mt_g")
    for a, b in zip(sets[0], sets[1]):
        assert beq(a, b)
    assert not beq(sets[1][0], bufs[0])                  # weight decay moved the masters


# ---------------------------------------------------------------- 2. ShadowAdam
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


def _shadow_adam(model, flat_grads):
    from gloria.optim import ShadowAdam, shadow_parameter_ids
    return ShadowAdam(list(model.parameters()), lr=1e-2, betas=(0.5, 0.999), weight_decay=1e-3, max_grad_norm=0.25,
                      shadow_ids=shadow_parameter_ids(model), flat_grads=flat_grads)


def _feed(opt, params, step, inject=None):
    """deterministic gradients of `step` (+ one injected value: (parameter index, index tuple, value))"""
    g = torch.Generator(DEV).manual_seed(100 + step)
    opt.zero_grad()
    for k, p in enumerate(params):
        grad = (torch.randn(p.shape, device=DEV, generator=g) * (0.3 if step % 2 else 3.0)).to(p.dtype)
        if inject is not None and inject[0] == k:
            grad[inject[1]] = inject[2]
        p.grad = torch.empty_strided(p.shape, p.stride(), dtype=p.dtype, device=DEV).copy_(grad)
    if opt.flat_grads:
        for grp in opt.groups:
            half = len(grp.params) // 2
            grp.gather(0, half)
            grp.gather(half, len(grp.params))


def _state(opt):
    out = []
    for grp in opt.groups:
        out += [grp.master, grp.exp_avg, grp.exp_avg_sq] + ([grp.shadow_buf] if grp.shadow_buf is not None else [])
    return [t.clone() for t in out]


@pytest.mark.parametrize("flat_grads", [True, False])
def test_skipped_steps_equal_never_taken(flat_grads):
    a, b = _toy(), _toy()
    pa, pb = list(a.parameters()), list(b.parameters())
    oa, ob = _shadow_adam(a, flat_grads), _shadow_adam(b, flat_grads)
    names = [n for n, _ in a.named_parameters()]
    i_fc1, i_ln = names.index("fc1.weight"), names.index("ln.weight")
    assert pa[i_fc1].dtype == torch.bfloat16 and pa[i_ln].dtype == torch.float32
    bad = {3: (i_fc1, (5, 7), INF), 5: (i_ln, (11,), float("nan"))}
    located = {}
    for step in range(1, 7):
        _feed(oa, pa, step, bad.get(step))
        oa.step()
        if step in bad:
            r = oa.record.tolist()
            assert r[NF.SKIP] == 1 and r[NF.LAST_CALL] == step and r[NF.LAST_COUNT] == 1
            located[step] = oa.locate(r[NF.LAST_PARTIAL], r[NF.LAST_OFFSET])
            continue
        _feed(ob, pb, step)
        ob.step()
        assert beq(oa.clip_state, ob.clip_state), step
    for x, y in zip(_state(oa), _state(ob)):
        assert beq(x, y)
    assert oa.t == 4 and ob.t == 4 and oa.calls == 6
    r = oa.record.tolist()
    assert r[NF.SKIPPED] == 2 and r[NF.CONSECUTIVE] == 0 and r[NF.LONGEST] == 1
    p, e = located[3]
    assert p is pa[i_fc1] and NF.unravel(tuple(p.shape), p.stride(), e) == (5, 7)
    p, e = located[5]
    assert p is pa[i_ln] and e == 11
    assert all(float(s["step"]) == 4.0 for s in oa.state_dict()["state"].values())


@pytest.mark.parametrize("flat_grads", [True, False])
def test_guarded_steps_equal_plain_entry_points(flat_grads):
    """20 finite steps through the guarded kernels == the unchanged glr_sumsq_* / glr_clip_coef / glr_adam_step* fed the
    same gradients (bias corrections from the host table at t = 1 .. 20), bitwise"""
    a, b = _toy(), _toy()
    pa, pb = list(a.parameters()), list(b.parameters())
    oa, ob = _shadow_adam(a, flat_grads), _shadow_adam(b, flat_grads)
    L, st = N.lib(), N.stream()
    pg = ob.param_groups[0]
    for step in range(1, 21):
        _feed(oa, pa, step)
        oa.step()
        _feed(ob, pb, step)
        o = 0
        for g, nb in zip(ob.groups, ob._nblocks):
            if flat_grads:
                N.check(L.glr_sumsq_partial(N.ptr(g.grad), N.dtype_code(g.gdt), g.n, N.ptr(ob._partial[o:]), st), "s")
            else:
                g.stage_grad_pointers()
                N.check(L.glr_sumsq_mt(N.ptr(g.table), g.n_chunks, N.ptr(g.ptr_dev), N.dtype_code(g.gdt),
                                       N.ptr(ob._partial[o:]), st), "s")
            o += nb
        N.check(L.glr_clip_coef(N.ptr(ob._partial), o, ob.max_grad_norm, N.ptr(ob.clip_state), st), "c")
        hyper = (float(pg["lr"]), 0.5, 0.999, float(pg["eps"]), float(pg["weight_decay"]), step, N.ptr(ob.clip_state), st)
        for g in ob.groups:
            if flat_grads:
                N.check(L.glr_adam_step(N.ptr(g.master), N.ptr(g.exp_avg), N.ptr(g.exp_avg_sq), N.ptr(g.grad),
                                        N.dtype_code(g.gdt), N.ptr(g.shadow_buf), g.n, *hyper), "a")
            else:
                N.check(L.glr_adam_step_mt(N.ptr(g.table), g.n_chunks, N.ptr(g.ptr_dev), N.dtype_code(g.gdt),
                                           N.ptr(g.master), N.ptr(g.exp_avg), N.ptr(g.exp_avg_sq), N.ptr(g.shadow_buf),
                                           *hyper), "a")
        assert beq(oa.clip_state, ob.clip_state), step
        for x, y in zip(_state(oa), _state(ob)):
            assert beq(x, y), step
    assert oa.t == 20 and oa.record[NF.SKIPPED].item() == 0


# ---------------------------------------------------------------- 3-8. trainer
def _cfg(B, layers=2):
    from gloria.config import pretrain_config
    cfg = pretrain_config("imagenome", batch_size=B)
    cfg.set_path("model.text.bert_config", dict(num_hidden_layers=layers, hidden_dropout_prob=0.0,
                                                attention_probs_dropout_prob=0.0))
    return cfg


def _trainer(precision="bf16", graphs=False, flat=None, nonfinite=None, dist_ctx=None, log_path=None, seed=21, B=8,
             layers=2):
    from gloria import builder
    from gloria.trainer import Trainer
    cfg = _cfg(B, layers)
    torch.manual_seed(seed)
    model = builder.build_lightning_model(cfg, builder.build_data_module(cfg))
    tr = Trainer(cfg, device=DEV, precision=precision, flat_optimizer=flat, nonfinite=nonfinite, dist_ctx=dist_ctx,
                 log_path=log_path, graph_image_encoder=graphs, graph_text_encoder=graphs)
    tr.setup(model)
    model.train()
    return tr, model


class _Inject:
    """gradient hook: puts `value` at `index` of the parameter's gradient on the listed trainer steps"""

    def __init__(self, tr, param, index, value, steps):
        self.tr, self.index, self.value, self.steps = tr, index, value, set(steps)
        param.register_hook(self)

    def __call__(self, g):
        if self.tr.global_step + 1 not in self.steps:
            return g
        g = g.clone()
        g[self.index] = self.value
        return g


def _flat_state(tr):
    return _state(tr.optimizer) + [p.detach().clone() for p in tr.params]


CONV = "gloria.img_encoder.model.layer1.0.conv2.weight"
TEXT_LN = "gloria.text_encoder.model.encoder.layer.0.attention.output.LayerNorm.weight"


@pytest.mark.parametrize("name,index,value", [(CONV, (3, 5, 1, 2), INF), (TEXT_LN, (17,), float("nan"))])
def test_trainer_skips_and_reports_bf16_eager(monkeypatch, tmp_path, name, index, value):
    from gloria.datasets.synthetic import make_batch
    monkeypatch.setattr(NF, "POLL_EVERY", 1)
    log = tmp_path / "log.jsonl"
    tr, model = _trainer(log_path=str(log))
    assert tr.flat and model.gloria._img_graph is None
    p = dict(model.named_parameters())[name]
    _Inject(tr, p, index, value, steps=[2])
    batch = make_batch(8, seed=5)
    tr.training_step(model, batch, 0)
    before = _flat_state(tr)
    with pytest.warns(RuntimeWarning, match="non-finite"):
        tr.training_step(model, batch, 1)                   # the bad step: skipped
        after = _flat_state(tr)
        tr.training_step(model, batch, 2)                   # its poll (POLL_EVERY = 1)
    for x, y in zip(before, after):
        assert beq(x, y)
    assert tr.skipped_steps == 1 and tr.optimizer.t == 2
    recs = [json.loads(line)["nonfinite"] for line in open(log) if "nonfinite" in line]
    assert len(recs) == 1 and recs[0]["parameter"] == name and recs[0]["step"] == 2
    assert tuple(recs[0]["element"]) == index and recs[0]["count"] == 1
    # raise mode: NonFiniteGradientError names the parameter within POLL_EVERY + 1 steps
    tr, model = _trainer(nonfinite="raise")
    _Inject(tr, dict(model.named_parameters())[name], index, value, steps=[1])
    with pytest.raises(NF.NonFiniteGradientError) as e:
        for i in range(3):
            tr.training_step(model, batch, i)
    assert e.value.parameter == name and e.value.step == 1 and tr.global_step <= 1 + 1


def test_graphs_dropped_after_a_skipped_step(monkeypatch):
    from gloria.datasets.synthetic import make_batch
    monkeypatch.setattr(NF, "POLL_EVERY", 1)
    tr, model = _trainer(graphs=None, layers=12)          # the text graph needs more layers than last_n_layers
    batch = make_batch(8, seed=6)
    tr.training_step(model, batch, 0)
    gl = model.gloria
    assert gl._img_graph is not None and gl.text_encoder._graph is not None, "both graphs must be captured"
    used = {"img": 0, "txt": 0}

    def counting(fn, key):
        def call(*a, **k):
            used[key] += 1
            return fn(*a, **k)
        return call

    object.__setattr__(gl, "_img_graph", counting(gl._img_graph, "img"))
    object.__setattr__(gl.text_encoder, "_graph", counting(gl.text_encoder._graph, "txt"))
    inner = model.training_step

    def bad_loss(b, i):
        out = inner(b, i)
        if tr.global_step + 1 == 3:
            out["loss"] = out["loss"] * INF
        return out

    monkeypatch.setattr(model, "training_step", bad_loss)
    tr.training_step(model, batch, 1)
    assert used["img"] == 1 and used["txt"] == 1, used          # the graphs are in use
    before = _flat_state(tr)
    tr.training_step(model, batch, 2)                           # loss * inf: skipped
    assert tr.optimizer.record[NF.SKIP].item() == 1 and used["img"] == 2 and used["txt"] == 2
    for x, y in zip(before, _flat_state(tr)):
        assert beq(x, y)
    with pytest.warns(RuntimeWarning, match="graphs are dropped"):
        tr.training_step(model, batch, 3)                       # replays, then its poll drops both graphs
    assert gl._img_graph is None and gl.text_encoder._graph is None
    losses = [float(tr.training_step(model, batch, i)) for i in range(4, 6)]
    assert all(np.isfinite(losses)) and tr.skipped_steps == 1
    assert used["img"] == 3 and used["txt"] == 3               # nothing replayed after the drop


def test_single_rank_rccl_flat_gradients_skip(monkeypatch):
    import socket
    import torch.distributed as dist
    from gloria import dist as gdist
    from gloria.datasets.synthetic import make_batch
    monkeypatch.setattr(NF, "POLL_EVERY", 1)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    for k, v in dict(GLR_FORCE_DIST="1", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                     MASTER_PORT=str(port)).items():
        monkeypatch.setenv(k, v)
    try:
        dctx = gdist.init_from_env("nccl")
        tr, model = _trainer(dist_ctx=dctx)
        assert tr.optimizer.flat_grads and tr.reducer is not None
        _Inject(tr, dict(model.named_parameters())[CONV], (0, 1, 2, 0), INF, steps=[2])
        batch = make_batch(8, seed=3)
        tr.training_step(model, batch, 0)
        before = _flat_state(tr)
        tr.training_step(model, batch, 1)
        for x, y in zip(before, _flat_state(tr)):
            assert beq(x, y)
        with pytest.warns(RuntimeWarning, match=CONV.replace(".", r"\.")):
            loss = float(tr.training_step(model, batch, 2))
        assert np.isfinite(loss) and tr.skipped_steps == 1 and tr.optimizer.t == 2
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_fp32_stock_path_skips(monkeypatch):
    from gloria.datasets.synthetic import make_batch
    monkeypatch.setattr(NF, "POLL_EVERY", 1)
    tr, model = _trainer(precision=32)
    assert not tr.flat and tr.optimizer.defaults.get("fused")
    p = dict(model.named_parameters())[CONV]
    _Inject(tr, p, (2, 0, 0, 1), float("nan"), steps=[2])
    batch = make_batch(8, seed=4)
    tr.training_step(model, batch, 0)
    w = [q.detach().clone() for q in tr.params]
    held = [q for q in tr.params if q in tr.optimizer.state]
    assert any(q is p for q in held)
    steps = [float(tr.optimizer.state[q]["step"]) for q in held]
    moments = [tr.optimizer.state[q]["exp_avg"].clone() for q in held]
    tr.training_step(model, batch, 1)
    for q, x in zip(tr.params, w):
        assert beq(q.detach(), x)
    for q, s0, m0 in zip(held, steps, moments):
        assert float(tr.optimizer.state[q]["step"]) == s0 == 1.0 and beq(tr.optimizer.state[q]["exp_avg"], m0)
    with pytest.warns(RuntimeWarning, match="non-finite"):
        tr.training_step(model, batch, 2)
    assert tr.skipped_steps == 1 and float(tr.optimizer.state[p]["step"]) == 2.0
    assert not beq(p.detach(), next(x for q, x in zip(tr.params, w) if q is p))


def test_checkpoint_round_trips_counters(tmp_path, monkeypatch):
    from gloria.datasets.synthetic import make_batch
    monkeypatch.setattr(NF, "POLL_EVERY", 1)
    tr, model = _trainer()
    _Inject(tr, dict(model.named_parameters())[CONV], (0, 0, 0, 0), INF, steps=[2])
    batch = make_batch(8, seed=8)
    with pytest.warns(RuntimeWarning):
        for i in range(3):
            tr.training_step(model, batch, i)
    ck = tmp_path / "skip.ckpt"
    with _quiet():
        tr.save_checkpoint(model, str(ck))
    saved = torch.load(ck, map_location="cpu", weights_only=True)
    assert saved["nonfinite"]["skipped"] == 1 and saved["nonfinite"]["applied"] == 2 and saved["nonfinite"]["calls"] == 3
    assert {float(s["step"]) for s in saved["optimizer_states"][0]["state"].values()} == {2.0}
    tr2, m2 = _trainer(seed=99)
    tr2.resume(m2, str(ck))
    assert tr2.optimizer.t == 2 and tr2.skipped_steps == 1 and tr2.optimizer.calls == 3
    assert tr2.optimizer.record[NF.LONGEST].item() == 1
    for (n1, p1), (_, p2) in zip(model.named_parameters(), m2.named_parameters()):
        a, b = tr.optimizer.master_of(p1), tr2.optimizer.master_of(p2)
        if a is None:
            continue
        assert beq(a, b) and beq(p1.detach(), p2.detach()), n1
        assert beq(tr.optimizer.state[p1]["exp_avg"], tr2.optimizer.state[p2]["exp_avg"]), n1
        assert beq(tr.optimizer.state[p1]["exp_avg_sq"], tr2.optimizer.state[p2]["exp_avg_sq"]), n1
    tr3, m3 = _trainer(flat=False, seed=98)
    tr3.resume(m3, str(ck))
    assert not tr3.flat
    assert {float(tr3.optimizer.state[p]["step"]) for p in tr3.params if p in tr3.optimizer.state} == {2.0}
    assert tr3.skipped_steps == 1


class _quiet:
    def __enter__(self):
        import warnings
        self.c = warnings.catch_warnings()
        self.c.__enter__()
        warnings.simplefilter("ignore")

    def __exit__(self, *a):
        return self.c.__exit__(*a)


def test_consecutive_limit_raises(monkeypatch):
    from gloria.datasets.synthetic import make_batch
    monkeypatch.setattr(NF, "POLL_EVERY", 1)
    monkeypatch.setattr(NF, "MAX_CONSECUTIVE", 3)
    tr, model = _trainer()
    _Inject(tr, dict(model.named_parameters())[CONV], (0, 0, 1, 1), INF, steps=range(1, 10))
    batch = make_batch(8, seed=9)
    with _quiet():
        with pytest.raises(NF.NonFiniteGradientError) as e:
            for i in range(8):
                tr.training_step(model, batch, i)
    assert e.value.consecutive == 3 and e.value.step == 3 and tr.global_step == 4
    assert tr.optimizer.t == 0 and tr.skipped_steps == 4
