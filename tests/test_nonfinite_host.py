"""CPU checks of the non-finite gradient guard's host side (gloria/nonfinite.py): policy decisions from synthetic device
records, deterministic polling across simulated ranks, locate() on both partial-sum layouts, and the host-built Adam
bias-correction table (glr_adam_bias_table, no GPU)."""

import ctypes
import json
import warnings

import numpy as np
import pytest

from gloria import nonfinite as NF


def rec(applied=0, skipped=0, consecutive=0, call=0, count=0, partial=-1, offset=-1, longest=None):
    r = NF.new_record()
    r[NF.APPLIED], r[NF.SKIPPED], r[NF.CONSECUTIVE] = applied, skipped, consecutive
    r[NF.SKIP] = int(consecutive > 0)
    r[NF.LAST_CALL], r[NF.LAST_COUNT], r[NF.LAST_PARTIAL], r[NF.LAST_OFFSET] = call, count, partial, offset
    r[NF.LONGEST] = consecutive if longest is None else longest
    return r


def monitor(mode, graphs=False):
    logs, dropped = [], []

    def drop():
        dropped.append(True)
        return graphs

    m = NF.Monitor(mode, describe=lambda p, o: (f"param{p}", (o,)), drop_graphs=drop, log=logs.append)
    return m, logs, dropped


def test_mode_from_argument_and_environment(monkeypatch):
    monkeypatch.delenv("GLR_NONFINITE", raising=False)
    assert NF.resolve_mode() == "skip"
    monkeypatch.setenv("GLR_NONFINITE", "raise")
    assert NF.resolve_mode() == "raise"
    assert NF.resolve_mode("skip") == "skip"                  # the argument wins over the environment
    monkeypatch.setenv("GLR_NONFINITE", "ignore")
    with pytest.raises(ValueError):
        NF.resolve_mode()
    with pytest.raises(ValueError):
        NF.resolve_mode("warn")


def test_trainer_rejects_unknown_mode(monkeypatch):
    from gloria.config import pretrain_config
    from gloria.trainer import Trainer
    cfg = pretrain_config("imagenome", batch_size=4)
    assert Trainer(cfg, device="cpu", nonfinite="raise").nonfinite == "raise"
    monkeypatch.setenv("GLR_NONFINITE", "bogus")
    with pytest.raises(ValueError):
        Trainer(cfg, device="cpu")


def test_skip_mode_logs_warns_and_drops_graphs():
    m, logs, dropped = monitor("skip", graphs=True)
    assert m.act(rec(applied=7), 8) is None and not logs           # nothing skipped: nothing happens
    with pytest.warns(RuntimeWarning, match="dropped"):
        info = m.act(rec(applied=7, skipped=2, consecutive=0, call=5, count=3, partial=4, offset=17), 16)
    assert dropped and len(logs) == 1 and logs[0] is info
    got = json.loads(json.dumps(info))["nonfinite"]                 # a JSON log record
    assert got["skipped"] == 2 and got["skipped_total"] == 2 and got["step"] == 5 and got["count"] == 3
    assert got["parameter"] == "param4" and got["element"] == [17] and got["poll_step"] == 16
    assert m.act(rec(applied=15, skipped=2, call=5), 24) is None    # already reported
    with pytest.warns(RuntimeWarning) as w:
        m.act(rec(applied=15, skipped=3, consecutive=1, call=25, count=1, partial=0, offset=0), 32)
    assert len(w) == 1 and logs[-1]["nonfinite"]["skipped"] == 1


def test_raise_mode_and_consecutive_limit(monkeypatch):
    m, logs, _ = monitor("raise")
    with pytest.raises(NF.NonFiniteGradientError) as e:
        m.act(rec(applied=3, skipped=1, consecutive=1, call=4, count=2, partial=1, offset=9), 5)
    assert e.value.parameter == "param1" and e.value.element == (9,) and e.value.step == 4 and e.value.count == 2
    assert logs                                                     # logged before it raises
    monkeypatch.setattr(NF, "MAX_CONSECUTIVE", 3)
    m, _, _ = monitor("skip")
    with pytest.warns(RuntimeWarning):
        m.act(rec(skipped=2, consecutive=2, call=2, count=1, partial=0, offset=0), 2)
    with pytest.raises(NF.NonFiniteGradientError) as e:
        m.act(rec(skipped=3, consecutive=3, call=3, count=1, partial=0, offset=0), 3)
    assert e.value.consecutive == 3
    # a run of 3 that ended between two polls still raises (LONGEST keeps it)
    m, _, _ = monitor("skip")
    with pytest.raises(NF.NonFiniteGradientError):
        m.act(rec(applied=9, skipped=3, consecutive=0, call=7, count=1, partial=0, offset=0, longest=3), 16)


class _FakeRank:
    """a rank whose record copies complete after a rank-specific delay (in 'host ticks'); wait() blocks until then"""

    def __init__(self, history, delay):
        self.history, self.delay, self.clock, self.step = history, delay, 0, 0
        self.waited = []

    def snapshot(self):
        r = list(self.history[self.step])
        ready_at = self.clock + self.delay
        rank = self

        class H:
            def wait(self):
                rank.waited.append(max(0, ready_at - rank.clock))
                rank.clock = max(rank.clock, ready_at)
                return r

        return H()


def test_ranks_with_different_copy_timings_decide_identically(monkeypatch):
    monkeypatch.setattr(NF, "POLL_EVERY", 4)
    # the device record after each step: skips at steps 6, 7 and 13 (identical on every rank: reduced gradients)
    hist, r = {}, rec()
    for step in range(0, 25):
        r = list(r)
        if step in (6, 7, 13):
            r[NF.SKIPPED] += 1
            r[NF.CONSECUTIVE] += 1
            r[NF.LAST_CALL], r[NF.LAST_COUNT], r[NF.LAST_PARTIAL], r[NF.LAST_OFFSET] = step, 1, 0, step
            r[NF.LONGEST] = max(r[NF.LONGEST], r[NF.CONSECUTIVE])
        elif step:
            r[NF.APPLIED] += 1
            r[NF.CONSECUTIVE] = 0
        hist[step] = r
    events = []
    for delay in (0, 3, 50):
        fr = _FakeRank(hist, delay)
        poller = NF.Poller(fr.snapshot)
        m, _, _ = monitor("skip", graphs=True)
        for step in range(1, 25):
            fr.step = step
            fr.clock += 1
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                m.act(poller.at_step(step), step)
        events.append(m.events)
    assert events[0] == events[1] == events[2]
    assert [e[1] for e in events[0]] == [12, 20]       # skips of steps 6, 7 act at 12 (copied at 8), 13 at 20 (from 16)


def test_poller_acts_only_on_multiples(monkeypatch):
    monkeypatch.setattr(NF, "POLL_EVERY", 2)
    taken = []

    class H:
        def __init__(self, k):
            self.k = k

        def wait(self):
            return self.k

    p = NF.Poller(lambda: taken.append(len(taken)) or H(len(taken) - 1))
    assert [p.at_step(s) for s in range(1, 8)] == [None, None, None, 0, None, 1, None]
    p.drop_pending()
    assert p.at_step(8) is None


def _ref_chunks(numels, chunk):
    return [(i, min(chunk, n - c0), c0) for i, n in enumerate(numels) for c0 in range(0, n, chunk)]


def test_locate_pointer_table_layout():
    from gloria.optim import CHUNK
    # registration order a, b, c, d, e; the optimizer's groups hold them in REVERSE registration order
    numels = {"a": 13, "b": 2 * CHUNK + 5, "c": 8, "d": CHUNK, "e": 3}
    shadow = {"b", "d"}
    order = [n for n in reversed(list(numels))]
    groups = [[n for n in order if n in shadow], [n for n in order if n not in shadow]]
    layout = [NF.group_layout([numels[n] for n in g], chunk=CHUNK) for g in groups]
    assert [g["n_partials"] for g in layout] == [1 + 3, 1 + 1 + 1]
    assert layout[0]["chunks"] == _ref_chunks([numels[n] for n in groups[0]], CHUNK)
    assert groups[0] == ["d", "b"] and groups[1] == ["e", "c", "a"]
    assert NF.locate(layout, 0, 5) == (0, 0, 5)                       # d
    assert NF.locate(layout, 1, 0) == (0, 1, 0)                       # b, first chunk
    assert NF.locate(layout, 2, CHUNK - 1) == (0, 1, 2 * CHUNK - 1)   # b, the chunk boundary
    assert NF.locate(layout, 3, 4) == (0, 1, 2 * CHUNK + 4)           # b, its short last chunk
    assert NF.locate(layout, 4, 2) == (1, 0, 2)                       # second group: e
    assert NF.locate(layout, 6, 12) == (1, 2, 12)                     # a
    with pytest.raises(ValueError):
        NF.locate(layout, 3, 5)                                       # beyond the chunk's 5 elements
    with pytest.raises(ValueError):
        NF.locate(layout, 7, 0)


def test_locate_flat_gradient_layout():
    from gloria import _native as N
    numels = [13, 40000, 3, 8]
    L = N.lib()
    g0 = NF.group_layout(numels, nblocks=L.glr_sumsq_blocks(sum((n + 7) // 8 * 8 for n in numels)))
    g1 = NF.group_layout([5], nblocks=1)
    assert g0["offsets"] == [0, 16, 40016, 40024] and g0["n"] == 40032
    layout = [g0, g1]
    nb = g0["n_partials"]
    assert NF.locate(layout, 0, 12) == (0, 0, 12)
    assert NF.locate(layout, 0, 13) == (0, None, None)                # padding after the first parameter
    assert NF.locate(layout, nb - 1, 16 + 39999) == (0, 1, 39999)
    assert NF.locate(layout, nb - 1, 40016) == (0, 2, 0)
    assert NF.locate(layout, nb, 4) == (1, 0, 4)
    with pytest.raises(ValueError):
        NF.locate(layout, 0, 40032)


def test_unravel_memory_order():
    assert NF.unravel((2, 3, 4), (12, 4, 1), 17) == (1, 1, 1)
    # channels-last [O, C, H, W] = [2, 3, 2, 2]: strides (12, 1, 6, 3)
    assert NF.unravel((2, 3, 2, 2), (12, 1, 6, 3), 12 + 6 + 3 + 2) == (1, 2, 1, 1)
    assert NF.unravel((5,), (1,), 4) == (4,)


def test_adam_bias_table_runs_without_gpu():
    from gloria import _native as N
    cap = 200
    out = np.zeros(2 * cap, dtype=np.float32)
    assert N.lib().glr_adam_bias_table(0.5, 0.999, cap, out.ctypes.data_as(ctypes.c_void_p)) == 0
    t = np.arange(1, cap + 1)
    want = np.float32(1) - np.ldexp(np.float32(1), -t).astype(np.float32)      # 1 - 2^-t, rounded to fp32
    assert np.array_equal(out[0::2], want)
    assert out[0] == 0.5 and out[2] == 0.75 and out[4] == 0.875
    b2 = out[1::2]
    assert np.all(np.diff(b2) >= 0) and np.all((b2 > 0) & (b2 <= 1))
    assert abs(float(b2[0]) - (1 - 0.999) ** 0.5) < 1e-6
    assert N.lib().glr_adam_bias_table(0.5, 0.999, 0, out.ctypes.data_as(ctypes.c_void_p)) != 0
