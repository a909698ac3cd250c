"""Steps with non-finite gradients: skipped on the device, reported and acted on here.

The reference trains under native AMP (precision 16, its run.py:172-207), whose GradScaler checks every
gradient element and skips `optimizer.step()` when one is inf or NaN.  The flat optimizer does the same on the device
(include/glr.h glr_step_guard): a small int64 record counts applied and skipped steps and notes the first bad element of
the last skipped one.  This module decodes that record and decides what to do about it.  Nothing here touches the GPU,
so the CPU suite covers every decision.

Polling is deterministic: at every step k that is a multiple of POLL_EVERY the trainer copies the record to pinned host
memory, and at step k + POLL_EVERY it waits for that copy (long complete by then) and acts on it; the existing sync
points (evaluate, save_checkpoint, the end of fit) read the record directly.  No decision ever depends on whether a copy
has completed yet (no event.query()): every data-parallel rank holds the same record and must raise or drop its graphs
at the same step, or the next collective hangs.
"""

import bisect
import json
import os
import warnings

POLL_EVERY = 16           # steps between two looks at the device record
MAX_CONSECUTIVE = 50      # this many skipped steps in a row end the run (NonFiniteGradientError) in either mode

MODES = ("skip", "raise")

# record slots (include/glr.h GLR_GUARD_*)
APPLIED, SKIPPED, CONSECUTIVE, SKIP, LAST_CALL, LAST_COUNT, LAST_PARTIAL, LAST_OFFSET, LONGEST = range(9)
RECORD_WORDS = 16


class NonFiniteGradientError(RuntimeError):
    """a step's gradients held inf / NaN elements (the step itself was skipped: the weights are clean)"""

    def __init__(self, step, parameter, element, count, consecutive=1):
        self.step, self.parameter, self.element, self.count, self.consecutive = step, parameter, element, count, consecutive
        super().__init__(f"non-finite gradient at step {step}: {count} element(s), first in {parameter} at {element} "
                         f"({consecutive} consecutive skipped step(s))")


def resolve_mode(arg=None):
    """Trainer(nonfinite=...) or the environment's GLR_NONFINITE: 'skip' (default) or 'raise'"""
    v = arg if arg is not None else os.environ.get("GLR_NONFINITE", "skip")
    v = str(v).strip().lower()
    if v not in MODES:
        raise ValueError(f"nonfinite mode must be one of {MODES}, got {v!r}")
    return v


def new_record():
    return [0] * RECORD_WORDS


# ---------------------------------------------------------------- where a partial sum came from
def group_layout(numels, nblocks=None, chunk=None):
    """one dtype group of the flat optimizer, parameters in the group's order (gloria/optim.py): element counts, flat
    offsets (each parameter padded to 8) and either the number of glr_sumsq_partial blocks over the flat gradient buffer
    (`nblocks`) or the chunk table of the pointer-table kernels ({param, count, offset in the parameter}, `chunk`
    elements per entry: one partial per chunk)"""
    offsets, off = [], 0
    for n in numels:
        offsets.append(off)
        off += (n + 7) // 8 * 8
    g = {"numel": list(numels), "offsets": offsets, "n": off}
    if chunk is not None:
        g["chunks"] = [(i, min(chunk, n - c0), c0) for i, n in enumerate(numels) for c0 in range(0, n, chunk)]
        g["n_partials"] = len(g["chunks"])
    else:
        g["chunks"] = None
        g["n_partials"] = int(nblocks)
    return g


def locate(layout, partial_index, offset):
    """(group, parameter position in the group, element) of the non-finite element a guard record names: `offset` is an
    element of the flat gradient buffer (flat layout) or of the chunk (pointer-table layout).  The element is the index
    in the parameter's MEMORY order (channels-last weights stay as they lie).  (group, None, None) for padding."""
    base = 0
    for gi, g in enumerate(layout):
        if partial_index < base + g["n_partials"]:
            if g["chunks"] is not None:
                i, count, poff = g["chunks"][partial_index - base]
                if not 0 <= offset < count:
                    raise ValueError(f"offset {offset} outside chunk {partial_index} of {count} elements")
                return gi, i, poff + offset
            i = bisect.bisect_right(g["offsets"], offset) - 1
            if i < 0 or offset >= g["n"]:
                raise ValueError(f"offset {offset} outside the group's flat buffer of {g['n']} elements")
            e = offset - g["offsets"][i]
            return (gi, i, e) if e < g["numel"][i] else (gi, None, None)
        base += g["n_partials"]
    raise ValueError(f"partial index {partial_index} beyond the {base} partials of the layout")


def unravel(shape, stride, element):
    """memory-order element of a dense tensor -> its index tuple"""
    dims = sorted(range(len(shape)), key=lambda d: -stride[d])
    idx = [0] * len(shape)
    for d in dims:
        if stride[d]:
            idx[d], element = divmod(element, stride[d])
    return tuple(idx)


# ---------------------------------------------------------------- polling and policy
class Poller:
    """snapshot(): starts an asynchronous copy of the record, returns a handle whose wait() returns it (blocking).
    at_step(k) acts only at multiples of POLL_EVERY and returns the snapshot taken POLL_EVERY steps earlier (None for
    the first)."""

    def __init__(self, snapshot):
        self.snapshot = snapshot
        self.pending = None

    def at_step(self, step):
        if step % POLL_EVERY:
            return None
        rec = self.pending.wait() if self.pending is not None else None
        self.pending = self.snapshot()
        return rec

    def drop_pending(self):
        self.pending = None


class Monitor:
    """acts on record snapshots: new skips are logged (one JSON record and one warning per poll), raise in 'raise' mode
    or after MAX_CONSECUTIVE skips in a row, and drop the captured encoder graphs otherwise.

    describe(partial, offset) -> (parameter name, element index) or (None, None); drop_graphs() -> True when graphs
    were active and have been dropped; log(dict) writes a JSON log record."""

    def __init__(self, mode, describe=None, drop_graphs=None, log=None):
        self.mode = resolve_mode(mode)
        self.describe = describe or (lambda partial, offset: (None, None))
        self.drop_graphs = drop_graphs or (lambda: False)
        self.log = log or (lambda rec: None)
        self.seen_skipped = 0            # skipped steps already reported
        self.events = []                 # every decision taken: (kind, step, JSON record) - compared across ranks

    def act(self, rec, step):
        """rec: a record snapshot (sequence of ints), step: the trainer step at which it is acted on"""
        if rec is None:
            return None
        rec = [int(v) for v in rec]
        new = rec[SKIPPED] - self.seen_skipped
        if new <= 0:
            return None
        self.seen_skipped = rec[SKIPPED]
        name, element = self.describe(rec[LAST_PARTIAL], rec[LAST_OFFSET]) if rec[LAST_PARTIAL] >= 0 else (None, None)
        info = {"nonfinite": {"poll_step": step, "skipped": new, "skipped_total": rec[SKIPPED],
                              "applied_total": rec[APPLIED], "consecutive": rec[CONSECUTIVE],
                              "step": rec[LAST_CALL], "parameter": name,
                              "element": list(element) if isinstance(element, tuple) else element,
                              "count": rec[LAST_COUNT]}}
        self.log(info)
        if self.mode == "raise" or rec[LONGEST] >= MAX_CONSECUTIVE:
            self.events.append(("raise", step, json.dumps(info, sort_keys=True)))
            raise NonFiniteGradientError(rec[LAST_CALL], name, element, rec[LAST_COUNT], max(rec[LONGEST], 1))
        msg = (f"skipped {new} optimizer step(s) with non-finite gradients (last at step {rec[LAST_CALL]}: "
               f"{rec[LAST_COUNT]} element(s), first in {name} at {element})")
        dropped = bool(self.drop_graphs())
        if dropped:
            msg += "; the captured encoder graphs are dropped, training continues eagerly"
        warnings.warn(msg, RuntimeWarning, stacklevel=3)
        self.events.append(("drop" if dropped else "skip", step, json.dumps(info, sort_keys=True)))
        return info
