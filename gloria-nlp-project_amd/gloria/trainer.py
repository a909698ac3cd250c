"""Minimal training driver standing in for the Lightning Trainer the reference configures in
run.py:172-207 (precision 16 -> bf16 autocast here, gradient_clip_val 0.25, Adam(0.5, 0.999),
ReduceLROnPlateau, ModelCheckpoint-style save/resume with the reference's checkpoint layout).
One process per GPU; with a DistContext the loss is the global-batch loss and parameter gradients
are SUM-all-reduced before clipping (so the clip uses the global norm).

Gradient accumulation (Lightning's `accumulate_grad_batches`, 1.1.4 semantics): a window is k consecutive training
batches, each a full forward and backward of its own; the optimizer sees (1/k) x the sum of their gradients, and the
non-finite test, the global-norm clip and the optimizer step run once per window, after its last micro-batch.  The last
batch of an epoch closes its window early (the scale stays 1/k).  `global_step`, `fit(max_steps=...)`, the non-finite
poller and `ShadowAdam.calls` count OPTIMIZER STEPS.  k = 1 (the default) is the unaccumulated step, launch for
launch."""

import json
import os
import time

import torch

from . import nonfinite as NF


class Trainer:
    def __init__(self, cfg, device="cuda", precision=None, dist_ctx=None, log_path=None, miopen_benchmark=False,
                 sync_bn=False, flat_optimizer=None, graph_image_encoder=None, graph_text_encoder=None, nonfinite=None,
                 accumulate_grad_batches=None):
        self.cfg = cfg
        # micro-batches per optimizer step: the argument overrides cfg.lightning.trainer.accumulate_grad_batches
        k = accumulate_grad_batches if accumulate_grad_batches is not None else cfg.lightning.trainer.accumulate_grad_batches
        if k is None:
            k = 1
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise ValueError(f"accumulate_grad_batches must be an integer >= 1, got {k!r}")
        self.accumulate = k
        self._micro = 0                   # micro-batches already in the open window (0: no window is open)
        self.device = torch.device(device)
        prec = precision if precision is not None else cfg.lightning.trainer.precision
        self.autocast_dtype = torch.bfloat16 if str(prec) in ("16", "bf16") else None
        self.clip = cfg.lightning.trainer.gradient_clip_val
        self.max_epochs = cfg.lightning.trainer.max_epochs or 1
        self.dist = dist_ctx
        self.log_path = log_path
        self.global_step = 0
        self.optimizer = self.scheduler = None
        # MIOpen "benchmark" (find) mode picks the fastest solver per conv shape (-8 % step time at B = 256); its
        # per-process search is kept short by gloria.miopen_env (naive reference solvers off)
        self.miopen_benchmark = miopen_benchmark
        # data-parallel parity mode: BatchNorm statistics over the GLOBAL batch (torch SyncBatchNorm: one small
        # per-channel all-reduce per layer) - the reference oracle is single-device full-batch BN (SURVEY.md
        # section 7); the default keeps per-rank statistics (speed mode)
        # sync_bn="fused" (opt-in): the same statistics on the project's own BatchNorm kernels - one all-gather of
        # 2C+1 doubles per site and direction between their two passes (gloria/models/fused_bn.py: GlobalBatchNorm2d).
        # With the kernels switched off (GLR_FUSED_BN=0) it is sync_bn=True.
        if isinstance(sync_bn, str) and sync_bn != "fused":
            raise ValueError(f"sync_bn must be False, True or 'fused', got {sync_bn!r}")
        if isinstance(sync_bn, str):
            from .models import fused_bn
            if not fused_bn.ENABLED:
                print("Trainer: sync_bn='fused' needs the fused BatchNorm kernels (GLR_FUSED_BN=0): using torch SyncBatchNorm")
                sync_bn = True
        self.sync_bn_fused = sync_bn == "fused"
        self.sync_bn = bool(sync_bn)
        # hipGraph capture of both encoders' forward + backward at the first training step (GLoRIA.enable_image_graph: the
        # whole image encoder; BertEncoder.enable_graph: the 12 BERT layers): small per-rank batches are bound by the HOST
        # time of ~1100 launches.  Measured with the graph-safe runtime flag of gloria/hipgraph.py, data-parallel path on
        # one GPU (single-rank RCCL), ms per step: 32 pairs 25.3 eager -> 17.9 image graph -> 16.0 both; 64: 24.8; 128: 42.3;
        # at 256 pairs the GPU is the limit and the replays cost 1.4 ms (78.6 vs 77.3 eager).  Default (None): captured
        # when the per-rank batch is <= GRAPH_MAX_BATCH; GLR_GRAPH_IMG / GLR_GRAPH_TXT = 0 / 1 override.  The image graph
        # is off with SyncBatchNorm (a collective inside the capture), the text graph needs the flat bf16 optimizer.
        self.graph_image_encoder = self._tristate(graph_image_encoder, "GLR_GRAPH_IMG")
        self.graph_text_encoder = self._tristate(graph_text_encoder, "GLR_GRAPH_TXT")
        if self.sync_bn:
            self.graph_image_encoder = False
        self._graph_tried = False
        # bucketed all-reduce overlapped with backward (hooks) or one gather + all-reduce per group after it
        # (GradReducer.from_flat); GLR_REDUCER_OVERLAP=0/1 overrides the default
        # Default: NO overlap.  Measured on the single-rank RCCL rehearsal (one GPU, image-encoder graph on) the
        # hook-driven reducer costs ~5 ms per step at every per-rank batch - 20.3 vs 16.1 ms at 32 pairs, 29.3 vs 24.6 at
        # 64, 47.9 vs 42.2 at 128 (~360 Python hook calls and 5 bucket launches from autograd's device thread, and the
        # accumulate-grad nodes it keeps alive across steps) - against the ~1.4 ms a 268-MB bf16 all-reduce takes on
        # 8 GPUs when nothing hides it.
        env = os.environ.get("GLR_REDUCER_OVERLAP")
        self.reducer_overlap = (env != "0") if env is not None else False
        # bf16 runs on the GPU keep fp32 master weights + bf16 shadows in flat buffers and do clip + Adam in three
        # launches (gloria/optim.py); GLR_FLAT_OPTIMIZER=0 or flat_optimizer=False keeps torch's fused Adam + autocast casts
        if flat_optimizer is None:
            flat_optimizer = os.environ.get("GLR_FLAT_OPTIMIZER", "1") != "0"
        self.flat_optimizer = bool(flat_optimizer) and self.device.type == "cuda" and self.autocast_dtype is not None \
            and cfg.train.optimizer.name == "Adam"
        # steps whose gradients hold an inf / NaN element are skipped (native AMP's GradScaler behaviour, which the
        # reference trains under); 'skip' reports them and goes on, 'raise' ends the run (gloria/nonfinite.py).
        # GLR_NONFINITE=skip / raise
        self.nonfinite = NF.resolve_mode(nonfinite)
        self.monitor = None
        self._record = None

    GRAPH_MAX_BATCH = 128

    @staticmethod
    def _tristate(arg, env):
        if arg is not None:
            return bool(arg)
        v = os.environ.get(env)
        return None if v is None else v != "0"

    # ------------------------------------------------------------------ setup
    def setup(self, model):
        model.to(self.device)
        if self.device.type == "cuda":
            torch.backends.cudnn.benchmark = bool(self.miopen_benchmark)
            model.gloria.img_encoder.to(memory_format=torch.channels_last)
        model.gloria.dist = self.dist
        if self.sync_bn_fused:
            # every active data-parallel context, the single-rank rehearsal (GLR_FORCE_DIST=1) included
            if self.dist is not None and self.dist.active:
                from .models.fused_bn import convert_global_batchnorm
                model.gloria.img_encoder = convert_global_batchnorm(model.gloria.img_encoder, self.dist)
        elif self.sync_bn and self.dist is not None and self.dist.world_size > 1:
            model.gloria.img_encoder = torch.nn.SyncBatchNorm.convert_sync_batchnorm(model.gloria.img_encoder,
                                                                                      self.dist.group)
        # how build_optimizer is to build the optimizer for THIS run, written explicitly in both cases: the cfg also
        # travels inside checkpoints (hyper_parameters), and a stale `flat_bf16: True` from a bf16 run must not hand an
        # fp32 / GLR_FLAT_OPTIMIZER=0 run bf16 parameters.
        # data-parallel ranks gather every bucket's gradients into a flat buffer (all-reduced slice by slice during
        # backward); a single process reads the gradients where autograd leaves them (pointer table)
        self.cfg.set_path("train.optimizer.flat_bf16", bool(self.flat_optimizer))
        self.cfg.set_path("train.optimizer.flat_clip", self.clip if self.flat_optimizer else None)
        self.cfg.set_path("train.optimizer.flat_grads",
                          bool(self.flat_optimizer and self.dist is not None and self.dist.active))
        # accumulation windows: fp32 flat accumulators in every group, filled by glr_accum_mt (gloria/optim.py)
        self.cfg.set_path("train.optimizer.flat_accumulate", self.accumulate if self.flat_optimizer else 1)
        opt = model.configure_optimizers()
        self.optimizer, self.scheduler = opt["optimizer"], opt["lr_scheduler"]
        self.params = [p for g in self.optimizer.param_groups for p in g["params"]]
        from .optim import ShadowAdam
        self.flat = isinstance(self.optimizer, ShadowAdam)
        self.reducer = None
        if self.dist is not None and self.dist.active:
            from .dist import GradReducer
            if self.flat:       # the optimizer's flat gradient buffers are the all-reduce buckets
                self.reducer = GradReducer.from_flat(self.optimizer.groups, self.dist, overlap=self.reducer_overlap)
            else:
                self.reducer = GradReducer(self.params, self.dist)      # grads become views of flat buckets
        self._setup_nonfinite(model)
        return model

    # ------------------------------------------------------------------ non-finite gradients (gloria/nonfinite.py)
    def _setup_nonfinite(self, model):
        # the record of applied / skipped steps: the flat optimizer's guard writes its own on the device; the stock path
        # keeps the same layout up to date with a few tensor ops per step (_stock_guard)
        if self.flat:
            self._record = self.optimizer.record
        else:
            self._record = torch.zeros(NF.RECORD_WORDS, dtype=torch.int64, device=self.device)
            self._found_inf = torch.zeros((), dtype=torch.float32, device=self.device)   # GradScaler's shapes
            self._unit = torch.ones((), dtype=torch.float32, device=self.device)
        self._pinned = None
        self._names = {id(p): n for n, p in model.named_parameters()}
        self._poller = NF.Poller(self._snapshot)
        self.monitor = NF.Monitor(self.nonfinite, describe=self._describe,
                                  drop_graphs=getattr(model.gloria, "disable_graphs", None), log=self._log)

    def _snapshot(self):
        if self._record.is_cuda:
            if self._pinned is None:
                self._pinned = torch.zeros(NF.RECORD_WORDS, dtype=torch.int64).pin_memory()
            self._pinned.copy_(self._record, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            return _Snapshot(ev, self._pinned)
        return _Snapshot(None, self._record.clone())

    def _describe(self, partial, offset):
        if not self.flat:
            return None, None
        p, e = self.optimizer.locate(partial, offset)
        if p is None:
            return None, None
        return self._names.get(id(p)), NF.unravel(tuple(p.shape), p.stride(), e)

    def _stock_guard(self):
        """stock optimizer path: GradScaler's element-wise test (unit scale: the gradients stay bitwise as they are) before
        clipping; fused Adam reads the flag (`found_inf`), skips the update and rolls its step counts back on the
        device.  Other optimizers (and a CPU device) are skipped from the host.  Returns False when step() must not run."""
        grads = [p.grad for p in self.params if p.grad is not None]
        if not grads:
            return True
        found = self._found_inf.zero_()
        if self.device.type == "cuda":
            torch._amp_foreach_non_finite_check_and_unscale_(grads, found, self._unit)
        else:
            found.fill_(0.0 if all(bool(torch.isfinite(g).all()) for g in grads) else 1.0)
        b = found.to(torch.int64)
        r = self._record
        r[NF.APPLIED:NF.APPLIED + 1].add_(1 - b)
        r[NF.SKIPPED:NF.SKIPPED + 1].add_(b)
        r[NF.CONSECUTIVE:NF.CONSECUTIVE + 1].add_(1).mul_(b)
        r[NF.SKIP:NF.SKIP + 1].copy_(b)
        r[NF.LAST_CALL:NF.LAST_CALL + 1].mul_(1 - b).add_(b * (self.global_step + 1))
        r[NF.LAST_COUNT:NF.LAST_OFFSET + 1].mul_(1 - b).sub_(b)      # count and location unknown here: -1
        torch.maximum(r[NF.LONGEST:NF.LONGEST + 1], r[NF.CONSECUTIVE:NF.CONSECUTIVE + 1], out=r[NF.LONGEST:NF.LONGEST + 1])
        if self.device.type == "cuda" and self.optimizer.defaults.get("fused"):
            self.optimizer.found_inf = found
            return True
        return not bool(found)

    def _poll_nonfinite(self, now=False):
        """every POLL_EVERY steps: act on the record copied POLL_EVERY steps ago; now=True (the existing sync points):
        act on the current record"""
        if self.monitor is None:
            return
        if now:
            self._poller.drop_pending()
            rec = self._record.tolist()
        else:
            rec = self._poller.at_step(self.global_step)
        self.monitor.act(rec, self.global_step)

    @property
    def skipped_steps(self):
        """optimizer steps skipped for non-finite gradients so far (reads the device record: a sync)"""
        return 0 if self._record is None else int(self._record[NF.SKIPPED])

    def to_device(self, batch):
        out = {}
        for k, v in batch.items():
            if torch.is_tensor(v):
                host = v.numpy() if (k in ("caption_ids", "attention_mask") and v.device.type == "cpu") \
                    else getattr(v, "_glr_host", None)
                v = v.to(self.device, non_blocking=True)
                if k == "imgs" and self.device.type == "cuda":
                    v = v.contiguous(memory_format=torch.channels_last)
                if host is not None:
                    v._glr_host = host           # word-piece slotting and the row plan run on the host: no D2H sync per step
            out[k] = v
        return out

    # ------------------------------------------------------------------ one optimisation step
    def training_step(self, model, batch, batch_idx=0, last_in_epoch=False):
        """one micro-batch: forward, backward and - when it closes its accumulation window (every batch with
        accumulate_grad_batches = 1; else the window's k-th batch, or the epoch's last one) - the optimizer step.
        Returns the micro-batch's own, undivided loss."""
        batch = self.to_device(batch)
        if not self._graph_tried and self.device.type == "cuda" and self.autocast_dtype is not None:
            self._graph_tried = True          # once: the batch shape is static in training (drop_last loaders)
            auto = int(batch["imgs"].shape[0]) <= self.GRAPH_MAX_BATCH
            if auto if self.graph_image_encoder is None else self.graph_image_encoder:
                model.gloria.enable_image_graph(batch["imgs"], self.autocast_dtype)
            if (auto if self.graph_text_encoder is None else self.graph_text_encoder) and self.flat_optimizer:
                model.gloria.enable_text_graph(batch["caption_ids"], batch["attention_mask"], batch["token_type_ids"],
                                               self.autocast_dtype)
        ctx = torch.autocast(self.device.type, dtype=self.autocast_dtype) if self.autocast_dtype else _Null()
        with ctx:
            out = model.training_step(batch, batch_idx)
        loss = out["loss"]
        k = self.accumulate
        if k == 1:
            if self.reducer is not None:
                self.reducer.zero_grad()
                loss.backward()               # bucket all-reduces start as soon as a bucket is complete
                self.reducer.finish()
            else:
                self.optimizer.zero_grad(set_to_none=True)
                loss.backward()
        else:
            first = self._micro == 0
            last = self._micro + 1 == k or bool(last_in_epoch)
            self._micro = 0 if last else self._micro + 1
            # flat optimizer: backward at the full loss (the micro-batch's gradients are bitwise those of an
            # unaccumulated step) and 1/k applied in fp32 on the way into the accumulator; stock: the loss is divided
            # and autograd adds in place
            part = loss if self.flat else loss / k
            if self.reducer is not None:
                self.reducer.begin(first, last, scale=1.0 / k)
                part.backward()
                self.reducer.finish()         # the all-reduce happens in the window's last cycle only
            else:
                if first or self.flat:
                    self.optimizer.zero_grad(set_to_none=True)
                part.backward()
                if self.flat:
                    self.optimizer.accumulate(1.0 / k, first)
            if not last:
                return self._global_loss(model, loss)
        run = True if self.flat else self._stock_guard()       # the flat optimizer guards inside its step
        if self.clip and not self.flat:       # the flat optimizer clips inside its step (post-reduce global norm)
            torch.nn.utils.clip_grad_norm_(self.params, self.clip)
        if run:
            self.optimizer.step()
        self.global_step += 1
        self._poll_nonfinite()
        return self._global_loss(model, loss)

    def _global_loss(self, model, loss):
        """what a single process would report: under data parallelism a rank's own loss holds only its share of
        the segmentation / regulariser terms (GLoRIA.global_batch_loss adds the other ranks' shares)"""
        if self.dist is not None and self.dist.active and hasattr(model.gloria, "global_batch_loss"):
            return model.gloria.global_batch_loss().detach()
        return loss.detach()

    @torch.no_grad()
    def evaluate(self, model, loader, split="val"):
        self._poll_nonfinite(now=True)
        model.eval()
        tot, n = 0.0, 0
        for i, batch in enumerate(loader):
            batch = self.to_device(batch)
            ctx = torch.autocast(self.device.type, dtype=self.autocast_dtype) if self.autocast_dtype else _Null()
            with ctx:
                out = (model.validation_step if split == "val" else model.test_step)(batch, i)
            tot += float(self._global_loss(model, out["loss"]))      # identical on every rank
            n += 1
        model.train()
        return tot / max(n, 1)

    # ------------------------------------------------------------------ fit loop
    def fit(self, model, dm, max_steps=None, ckpt_dir=None):
        self.setup(model)
        model.train()
        history = []
        for epoch in range(self.max_epochs):
            model.current_epoch = epoch
            t0 = time.time()
            for i, (batch, last) in enumerate(_mark_last(dm.train_dataloader())):
                loss = self.training_step(model, batch, i, last_in_epoch=last)
                history.append(float(loss))
                self._log({"step": self.global_step, "epoch": epoch, "train_loss": history[-1]})
                if max_steps is not None and self.global_step >= max_steps:
                    break
            val = self.evaluate(model, dm.val_dataloader())
            self._log({"epoch": epoch, "val_loss": val, "epoch_s": time.time() - t0})
            sch = self.scheduler["scheduler"] if self.scheduler else None
            if sch is not None:
                sch.step(val) if isinstance(sch, torch.optim.lr_scheduler.ReduceLROnPlateau) else sch.step()
            if ckpt_dir and (self.dist is None or self.dist.rank == 0):
                self.save_checkpoint(model, os.path.join(ckpt_dir, "last.ckpt"))
            if max_steps is not None and self.global_step >= max_steps:
                break
        self._poll_nonfinite(now=True)
        return history

    def _log(self, rec):
        if self.log_path and (self.dist is None or self.dist.rank == 0):
            with open(self.log_path, "a") as f:
                f.write(json.dumps(rec) + "\n")

    # ------------------------------------------------------------------ checkpoints (reference layout + resume state)
    def save_checkpoint(self, model, path):
        """Checkpoints are written at epoch ends, where no accumulation window is open (the epoch's last batch closes
        it): gradient accumulators are not saved, and a resumed run starts a new window."""
        self._poll_nonfinite(now=True)
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        ckpt = model.checkpoint()
        if self.flat:        # the reference layout holds fp32 weights: write the masters, not the bf16 shadows
            for name, p in model.named_parameters():
                m = self.optimizer.master_of(p)
                if m is not None:
                    ckpt["state_dict"][name] = m.detach().clone()
        ckpt["optimizer_states"] = [self.optimizer.state_dict()]
        ckpt["global_step"] = self.global_step
        ckpt["epoch"] = model.current_epoch
        if self._record is not None:         # optimizer `step` holds the applied steps; the skip counters travel here
            r = self._record.tolist()
            ckpt["nonfinite"] = {"applied": r[NF.APPLIED], "skipped": r[NF.SKIPPED], "consecutive": r[NF.CONSECUTIVE],
                                 "longest": r[NF.LONGEST], "calls": self.optimizer.calls if self.flat else self.global_step}
        torch.save(ckpt, path)

    def resume(self, model, path):
        from .builder import clean_state_dict
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        sd = clean_state_dict(ckpt["state_dict"])
        model.load_state_dict(sd)
        if getattr(self, "flat", False):
            self.optimizer.load_masters((p, sd[name]) for name, p in model.named_parameters() if name in sd)
        if self.optimizer is not None and "optimizer_states" in ckpt:
            self.optimizer.load_state_dict(ckpt["optimizer_states"][0])
        self.global_step = ckpt.get("global_step", 0)
        model.current_epoch = ckpt.get("epoch", 0)
        nf = ckpt.get("nonfinite")
        if nf is not None and self._record is not None:
            r = self._record
            for k, slot in (("skipped", NF.SKIPPED), ("consecutive", NF.CONSECUTIVE), ("longest", NF.LONGEST)):
                r[slot] = int(nf[k])
            if self.flat:
                self.optimizer.calls = max(self.optimizer.calls, int(nf["calls"]))
            else:
                r[NF.APPLIED] = int(nf["applied"])
            self.monitor.seen_skipped = int(nf["skipped"])


def _mark_last(loader):
    """(batch, is the last one) over a loader, by a one-batch look-ahead (no len(): iterable datasets have none)"""
    it = iter(loader)
    try:
        cur = next(it)
    except StopIteration:
        return
    for nxt in it:
        yield cur, False
        cur = nxt
    yield cur, True


class _Snapshot:
    """a record copy in flight: wait() blocks on its event (never queried: gloria/nonfinite.py)"""

    def __init__(self, event, buf):
        self.event, self.buf = event, buf

    def wait(self):
        if self.event is not None:
            self.event.synchronize()
        return self.buf.tolist()


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
