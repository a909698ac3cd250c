"""BertEncoder with the reference's interface (/root/reference/gloria/models/text_model.py:6-144):
forward(ids, attn_mask, token_type) -> (word_embeddings [B, D, L], sent_embeddings [B, D], sents).

What changes underneath:
  * the BERT stack is gloria.models.bert.BertModel (HF-compatible parameter names);
  * `aggregate_tokens` (ref :32-90: a Python double loop with one `.item()` device sync per token)
    becomes a segment-sum: word-piece -> word slot indices are computed on the host from the caption
    ids with vectorised numpy (one small copy per step, no per-token sync) and the pieces are summed
    into their word slot on the GPU.  Because merging pieces is a sum, the 4-layer sum (ref :112)
    is taken first and merged once.
  * `sents` is a SentenceBatch: a list of B lists of L word strings like the reference returns, built
    lazily, that also carries the cap_lens the loss needs (ref gloria_model.py:107-109) so the hot
    path never touches Python strings.
"""

import ctypes
import os

import numpy as np
import torch
import torch.nn as nn

from .. import _native as N
from . import text_rows
from .bert import BertConfig, BertModel, encode_rows

PAD, UNK, CLS, SEP, MASK = 0, 100, 101, 102, 103


class Vocab:
    """id -> token properties needed by the aggregation (and, optionally, the strings)."""

    def __init__(self, tokens):
        self.tokens = list(tokens)
        self.is_cont = np.array([t.startswith("##") for t in self.tokens], dtype=bool)
        self.is_bracket = np.array([t.startswith("[") for t in self.tokens], dtype=bool)
        self.sep_id = self.tokens.index("[SEP]")

    def __len__(self):
        return len(self.tokens)

    @classmethod
    def synthetic(cls, size=28996, seed=99, cont_frac=0.2):
        """Offline stand-in for the Bio_ClinicalBERT word-piece vocabulary:
        ids 0/100/101/102/103 = PAD/UNK/CLS/SEP/MASK, `cont_frac` of the rest are '##' pieces."""
        rng = np.random.default_rng(seed)
        cont = rng.random(size) < cont_frac
        toks = [("##p%d" % i) if cont[i] else ("w%d" % i) for i in range(size)]
        for i, t in ((PAD, "[PAD]"), (UNK, "[UNK]"), (CLS, "[CLS]"), (SEP, "[SEP]"), (MASK, "[MASK]")):
            toks[i] = t
        return cls(toks)

    @classmethod
    def from_file(cls, path):
        with open(path, encoding="utf-8") as f:
            return cls([line.rstrip("\n") for line in f])

    @classmethod
    def from_dict(cls, idxtoword):
        return cls([idxtoword[i] for i in range(len(idxtoword))])


class SentenceBatch(list):
    """list of B word lists (materialised on first element access) + host cap_lens."""

    def __init__(self, ids, dst, starts, n_words, vocab, L):
        super().__init__()
        self._ids, self._dst, self._n_words, self._vocab, self._L = ids, dst, n_words, vocab, L
        first = np.full((ids.shape[0], L), -1, dtype=np.int64)      # first token id of every word slot
        b, t = np.nonzero((dst >= 0) & starts)                       # exactly one opening token per word
        first[b, dst[b, t]] = ids[b, t]
        has = first >= 0
        brk = np.zeros_like(has)
        brk[has] = vocab.is_bracket[first[has]]
        # cap_len = 1 + #words not starting with "[" ; padding slots are "[PAD]" (ref gloria_model.py:107-109)
        self.cap_lens = (1 + (has & ~brk).sum(1)).astype(np.int64).tolist()
        self._built = False

    def _build(self):
        if self._built:
            return
        toks = self._vocab.tokens
        out = []
        for b in range(self._ids.shape[0]):
            words = [""] * int(self._n_words[b])
            for t in range(self._ids.shape[1]):
                k = self._dst[b, t]
                if k >= 0:
                    s = toks[int(self._ids[b, t])]
                    words[k] += s[2:] if s.startswith("##") else s
            out.append(words + ["[PAD]"] * (self._L - len(words)))
        list.extend(self, out)
        self._built = True

    def __iter__(self):
        self._build()
        return list.__iter__(self)

    def __getitem__(self, i):
        self._build()
        return list.__getitem__(self, i)

    def __len__(self):
        return self._ids.shape[0]


def wordpiece_slots(ids: np.ndarray, vocab: Vocab):
    """Vectorised restatement of the scan of text_model.py:48-76.
    ids [B, L] -> dst [B, L] (word slot of every token, -1 = dropped), starts [B, L], n_words [B].
    A token that is not a '##' piece opens a new word; '[SEP]' is its own word and ends the scan;
    without a '[SEP]' the last open word is never flushed (dropped), exactly like the reference."""
    B, L = ids.shape
    starts = ~vocab.is_cont[ids]
    starts[:, 0] = True
    widx = np.cumsum(starts, axis=1) - 1
    is_sep = ids == vocab.sep_id
    has_sep = is_sep.any(1)
    sep_pos = np.where(has_sep, is_sep.argmax(1), L)
    t = np.arange(L)[None, :]
    keep = t <= sep_pos[:, None]
    last = widx[:, -1]
    keep &= has_sep[:, None] | (widx < last[:, None])
    dst = np.where(keep, widx, -1)
    n_words = np.where(has_sep, widx[np.arange(B), np.minimum(sep_pos, L - 1)] + 1, last)
    return dst, starts, n_words


def _segsum(rows, direction):
    """(entry point, its name, the row-plan argument it takes after dst) of K5 on padded (rows=None) or packed hidden states"""
    name = "glr_wordpiece_segsum_%s%s" % ("" if rows is None else "rows_", direction)
    return getattr(N.lib(), name), name, () if rows is None else (N.ptr(rows.row_start),)


class WordpieceSegSumFn(torch.autograd.Function):
    """K5: (token -> word-slot index [B, L], PackedRows or None, mean over the layers?, hidden states of the last layers)
    -> word_emb [B, D, L], sent_emb [B, D].  rows=None: padded hidden states [B, L, D].  With a PackedRows they are [T, D]
    (models/text_rows.py): token t of sentence b is row row_start[b] + t.  dst stays [B, L], so word_emb / sent_emb are
    bitwise what the padded K5 gives; the backward writes the T packed rows."""

    @staticmethod
    def forward(ctx, dst, rows, mean_layers, *layers):
        hs = [h.detach().contiguous() for h in layers]
        if hs[0].dtype not in (torch.float32, torch.bfloat16):
            hs = [h.float() for h in hs]
        if rows is None:
            B, L, D = hs[0].shape
        else:
            B, L, D = rows.B, rows.L, hs[0].shape[-1]
            if tuple(hs[0].shape) != (rows.T, D) or tuple(dst.shape) != (B, L):
                raise RuntimeError("WordpieceSegSumFn: hidden states and dst do not match the row plan")
        dev = hs[0].device
        word = torch.empty(B, D, L, dtype=torch.float32, device=dev)
        sent = torch.empty(B, D, dtype=torch.float32, device=dev)
        ptrs = (ctypes.c_void_p * len(hs))(*[h.data_ptr() for h in hs])
        fn, name, plan = _segsum(rows, "fwd")
        N.check(fn(ptrs, len(hs), N.dtype_code(hs[0].dtype), N.ptr(dst), *plan, N.ptr(word), N.ptr(sent), B, L, D,
                   1 if mean_layers else 0, N.stream()), name)
        ctx.save_for_backward(dst)
        ctx.meta = (rows, hs[0].shape, B, L, D, len(hs), mean_layers, [h.dtype for h in layers])
        return word, sent

    @staticmethod
    def backward(ctx, d_word, d_sent):
        (dst,) = ctx.saved_tensors
        rows, shape, B, L, D, nl, mean_layers, dts = ctx.meta
        dw = None if d_word is None else d_word.float().contiguous()
        ds = None if d_sent is None else d_sent.float().contiguous()
        out_dt = torch.bfloat16 if dts[0] == torch.bfloat16 else torch.float32
        dh = torch.empty(shape, dtype=out_dt, device=dst.device)
        fn, name, plan = _segsum(rows, "bwd")
        N.check(fn(N.ptr(dw), N.ptr(ds), N.ptr(dst), *plan, N.ptr(dh), N.dtype_code(out_dt), B, L, D, nl,
                   1 if mean_layers else 0, N.stream()), name)
        return (None, None, None) + tuple(dh.to(dt) for dt in dts)


def _sum_word_pieces(embeddings, dst):
    """embeddings [B, L, D] -> [B, L, D]: token t of sentence b added into word slot dst[b, t] (torch ops: CPU tensors)"""
    B, L = dst.shape
    flat = dst + (np.arange(B) * L)[:, None]
    src = np.nonzero(dst.reshape(-1) >= 0)[0]
    idx = torch.from_numpy(np.stack([src, flat.reshape(-1)[src]])).to(embeddings.device, non_blocking=True)
    x = embeddings.reshape(B * L, -1)
    return torch.zeros_like(x).index_add_(0, idx[1], x.index_select(0, idx[0])).view(B, L, -1)


def host_ids(ids):
    """caption ids as a host array WITHOUT a device sync when the trainer kept the host copy (Trainer.to_device
    attaches it as `_glr_host`); a plain `.cpu()` here would drain the stream every step (the image encoder is
    already queued) and expose the launch latency of everything behind it."""
    host = getattr(ids, "_glr_host", None)
    if host is not None:
        return host
    return ids.detach().cpu().numpy() if torch.is_tensor(ids) else np.asarray(ids)


class BertEncoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.bert_type = cfg.model.text.bert_type
        self.last_n_layers = cfg.model.text.last_n_layers
        self.aggregate_method = cfg.model.text.aggregate_method
        self.norm = cfg.model.text.norm
        self.embedding_dim = cfg.model.text.embedding_dim
        self.freeze_bert = cfg.model.text.freeze_bert
        self.agg_tokens = cfg.model.text.agg_tokens

        # no network: a local directory with config/weights/vocab may be given as bert_type,
        # otherwise BERT-base geometry with random init and the synthetic vocabulary.
        bcfg = BertConfig(hidden_size=self.embedding_dim) if self.embedding_dim != 768 else BertConfig()
        if cfg.model.text.bert_config is not None:
            bcfg = BertConfig(**cfg.model.text.bert_config)
        self.model = BertModel(bcfg)
        vocab_file = os.path.join(str(self.bert_type), "vocab.txt")
        if os.path.exists(vocab_file):
            self.vocab = Vocab.from_file(vocab_file)
            weights = os.path.join(str(self.bert_type), "model.safetensors")
            if os.path.exists(weights):
                from safetensors.torch import load_file
                sd = {k.replace("bert.", "", 1) if k.startswith("bert.") else k: v for k, v in load_file(weights).items()}
                self.model.load_state_dict(sd, strict=False)
        else:
            self.vocab = Vocab.synthetic(bcfg.vocab_size)
        self.idxtoword = None          # built on demand (reference attribute, text_model.py:23)

        # set by enable_graph(); out of the module tree (the graphed callable wraps self.model.encoder)
        object.__setattr__(self, "_graph", None)
        self._graph_key = None
        self._graph_rng = None

        self.emb_global, self.emb_local = None, None
        if self.freeze_bert is True:
            print("Freezing BERT model")
            for param in self.model.parameters():
                param.requires_grad = False

    def enable_graph(self, ids, attn_mask, token_type, autocast_dtype=None, warmup=3):
        """Capture the encoder layers' forward AND backward (12 layers: ~600 of the step's launches, static shapes) into
        two hipGraphs (torch.cuda.make_graphed_callables on bert.BertStackPath).  Small per-rank batches are bound by the
        HOST time of exactly these launches.  Dropout keys of the fused kernels come from a device cell rewritten before
        every replay (models/rng.py), so a replay draws fresh masks from torch's generator like the eager launches."""
        from .. import hipgraph
        from .bert import BertStackPath
        from .rng import GraphRng, capturing
        n_layers = len(self.model.encoder.layer)
        if (not ids.is_cuda or attn_mask is None or self.freeze_bert is True or self.last_n_layers <= 1
                or self.last_n_layers > n_layers or not hipgraph.usable("text encoder")):
            return False
        path = BertStackPath(self.model.encoder, self.last_n_layers)
        path.train(self.training)
        ctx = torch.autocast("cuda", dtype=autocast_dtype, cache_enabled=False) if autocast_dtype is not None \
            else torch.autocast("cuda", enabled=False)
        rng = GraphRng(ids.device)
        with ctx:
            with torch.no_grad():
                x = self.model.embeddings(ids, token_type)
            x = x.detach().clone().requires_grad_(True)
            mask4 = (attn_mask != 0)[:, None, None, :].clone()
            with capturing(rng):
                graphed = torch.cuda.make_graphed_callables(path, (x, mask4), num_warmup_iters=warmup)
            if not hipgraph.verify_capture("text encoder", path, graphed, (x, mask4), before_replay=rng.refresh):
                return False
        object.__setattr__(self, "_graph", graphed)
        self._graph_key = (tuple(ids.shape), autocast_dtype)
        self._graph_rng = rng
        return True

    def _graph_fits(self, ids, attn_mask):
        """whether this call goes through the captured graphs"""
        return (getattr(self, "_graph", None) is not None and self.training and torch.is_grad_enabled() and attn_mask is not None
                and self._graph_key == (tuple(ids.shape), torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else None))

    def _packed_rows(self, ids, attn_mask):
        """(PackedRows, word-piece slots) when this call may run the layers on its real token rows only, else (None, None):
        the K5 configuration on the GPU under bf16 autocast with every fused kernel on, host copies of ids and mask (no
        device sync), no captured graph for this call, and a mask plan_rows accepts (models/text_rows.py)."""
        from . import fused_attn, fused_linear, fused_ln
        none = (None, None)
        if not (text_rows.ENABLED and self.agg_tokens and self.last_n_layers > 1 and self.aggregate_method in ("sum", "mean")
                and torch.is_tensor(ids) and ids.is_cuda and torch.is_tensor(attn_mask)
                and fused_attn.ENABLED and fused_ln.ENABLED and fused_linear.ENABLED
                and torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16
                and not self._graph_fits(ids, attn_mask)):
            return none
        ids_h, mask_h = getattr(ids, "_glr_host", None), getattr(attn_mask, "_glr_host", None)
        if ids_h is None or mask_h is None or ids.dim() != 2 or tuple(np.shape(ids_h)) != tuple(ids.shape) \
                or tuple(np.shape(mask_h)) != tuple(ids.shape):
            return none
        c = self.model.config
        if not (fused_attn.heads_ok(c.hidden_size, c.num_attention_heads)
                and fused_ln.ln_ok(c.hidden_size, self.model.encoder.layer[0].output.LayerNorm)):
            return none
        slots = wordpiece_slots(np.asarray(ids_h), self.vocab)
        plan = text_rows.plan_rows(mask_h, slots[0], fused_attn._max_tokens())
        if plan is None:
            return none
        return text_rows.PackedRows(plan[0], plan[1], ids.shape[0], ids.shape[1], ids.device), slots

    def aggregate_tokens(self, embeddings, caption_ids):
        """embeddings [B, L, D] (already reduced over layers) -> word slots [B, L, D], sents."""
        ids = host_ids(caption_ids)
        dst, starts, n_words = wordpiece_slots(ids, self.vocab)
        return _sum_word_pieces(embeddings, dst), SentenceBatch(ids, dst, starts, n_words, self.vocab, ids.shape[1])

    def _hidden_states(self, ids, attn_mask, token_type):
        """step 1, the route -> (hidden states of the last `last_n_layers` layers or None when only the last is read,
        BertModel's outputs or None, PackedRows or None, the word-piece slots the row plan was made from or None)"""
        rows, slots = self._packed_rows(ids, attn_mask)
        if rows is not None:                    # the layers on the real token rows only; K5 reads the packed rows
            x = self.model.embeddings(ids, token_type)
            return encode_rows(self.model.encoder, x, rows, self.last_n_layers), None, rows, slots
        if self.last_n_layers > 1 and self._graph_fits(ids, attn_mask):         # the captured graphs
            x = self.model.embeddings(ids, token_type)
            self._graph_rng.refresh()
            return self._graph(x, (attn_mask != 0)[:, None, None, :]), None, None, None
        outputs = self.model(ids, attn_mask, token_type)                        # padded, eager (and every CPU call)
        return (outputs[2][-self.last_n_layers:] if self.last_n_layers > 1 else None), outputs, None, None

    def _aggregate(self, ids, layers, outputs, rows, slots):
        """step 2 -> (word_embeddings [B, L, D], sent_embeddings [B, D], sents)"""
        if layers is not None and self.aggregate_method not in ("sum", "mean"):
            print(self.aggregate_method)
            raise Exception("Aggregation method not implemented")
        host = host_ids(ids)
        if layers is not None and self.agg_tokens:
            dst, starts, n_words = wordpiece_slots(host, self.vocab) if slots is None else slots
            sents = SentenceBatch(host, dst, starts, n_words, self.vocab, host.shape[1])
        else:
            dst, sents = None, [[self.vocab.tokens[int(w)] for w in sent] for sent in host]
        if layers is None:
            return outputs[0], outputs[1], sents
        if dst is not None and layers[0].is_cuda:
            # K5 (every GPU call, any D / layer count): segment-sum fused with the layer reduction and the L-mean,
            # [B, D, L] written directly.  The torch branch below only ever sees CPU tensors (host-logic tests and the
            # CPU baseline of bench.py).
            dst_d = N.upload(dst.astype(np.int32), layers[0].device)
            word, sent = WordpieceSegSumFn.apply(dst_d, rows, self.aggregate_method == "mean", *layers)
            return word.permute(0, 2, 1), sent, sents                   # [B, L, D] view; permuted back in forward
        word = torch.stack(layers).sum(0) if self.aggregate_method == "sum" else torch.stack(layers).mean(0)
        if dst is not None:
            word = _sum_word_pieces(word, dst)
        return word, word.mean(dim=1), sents                            # over ALL L slots (ref :110)

    def forward(self, ids, attn_mask, token_type):
        layers, outputs, rows, slots = self._hidden_states(ids, attn_mask, token_type)
        word_embeddings, sent_embeddings, sents = self._aggregate(ids, layers, outputs, rows, slots)

        batch_dim, num_words, feat_dim = word_embeddings.shape
        if self.emb_local is not None:
            word_embeddings = self.emb_local(word_embeddings.reshape(batch_dim * num_words, feat_dim))
            word_embeddings = word_embeddings.view(batch_dim, num_words, self.embedding_dim)
        word_embeddings = word_embeddings.permute(0, 2, 1)
        if self.emb_global is not None:
            sent_embeddings = self.emb_global(sent_embeddings)
        if self.norm is True:
            word_embeddings = word_embeddings / torch.norm(word_embeddings, 2, dim=1, keepdim=True).expand_as(
                word_embeddings)
            sent_embeddings = sent_embeddings / torch.norm(sent_embeddings, 2, dim=1, keepdim=True).expand_as(
                sent_embeddings)
        return word_embeddings, sent_embeddings, sents
