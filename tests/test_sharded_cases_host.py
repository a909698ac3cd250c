"""Host check of tests/sharded_cases.py: every case's tile plan, built on the CPU by glr_plan_build, still has the work
items the GPU tests of the block-row loss path (tests/test_gpu_sharded_loss.py) rely on.  Those tests put the diagonal
sentences of the ranks with a non-zero image offset into every kind of K1 work item; if the planner ever packs these
captions differently, this test fails instead of the GPU tests silently losing a kernel."""

import numpy as np
import pytest

import sharded_cases as sc


def _plan(case):
    from gloria import _native as N
    return N.TilePlan(case["cap_lens"], "cpu", capacity=case["capacity"], allow_pairs=case["allow_pairs"])


@pytest.mark.parametrize("name", list(sc.CASES))
def test_plan_counts(name):
    c = sc.CASES[name]
    from gloria import _native as N
    assert N.lib().glr_tile_capacity(N.GLR_BF16 if c["bf16"] else N.GLR_F32) == c["capacity"]
    s_eff = c["H"] * c["W"] + 1                       # every case runs (also) with the no-attention vector
    s_pad = N.lib().glr_region_pad(s_eff)
    assert (s_pad == N.MAX_SPAD and s_eff < s_pad) == c["allow_pairs"]      # the rule of gloria_loss._pack_operands
    p = _plan(c)
    assert (p.n_tiles, p.n_single, p.n_pair, p.n_long_pair) == (c["n_tiles"], c["n_single"], c["n_pair"], c["n_long_pair"])
    h = p.host
    nsub = h[h[12]:h[12] + p.n_tiles]
    single = h[h[13]:h[13] + p.n_single]
    assert [int(nsub[t]) for t in single] == c["single_nsub"]
    assert len(c["cap_lens"]) == c["B"] and max(c["cap_lens"]) <= c["L"]
    assert all(c["B"] % w == 0 for w in c["worlds"])


@pytest.mark.parametrize("name", list(sc.CASES))
def test_diagonals_of_the_later_ranks_lie_in_every_listed_item_kind(name):
    c = sc.CASES[name]
    host = _plan(c).host
    assert sc.sentence_kinds(host) == c["kinds"]
    union = set()
    for world in c["worlds"]:
        union |= sc.diagonal_kinds(host, c["B"], world)
    assert union == c["diag_kinds"]
    if name == "full_bf16":
        # each later rank on its own meets more than one kind: rank 1 ordinary pairs + the unpaired tile, rank 2 the
        # four-tile sentence, both long pairs and an ordinary pair
        kinds = sc.sentence_kinds(host)
        assert {kinds[i] for i in range(5, 10)} == {sc.SINGLE, sc.PAIR}
        assert {kinds[i] for i in range(10, 15)} == {sc.SINGLE, sc.LONG_PAIR, sc.PAIR}
        assert kinds[10] == sc.SINGLE and c["cap_lens"][10] == 200          # 4 tiles, worked in sweeps
        assert kinds[7] == kinds[8] == sc.SINGLE                              # share the ordinary tile without a partner


def test_inputs_are_bf16_representable_where_the_case_says_so():
    for name, c in sc.CASES.items():
        img, words, na = sc.inputs(name, c["D"][0])
        assert img.shape == (c["B"], c["D"][0], c["H"], c["W"]) and words.shape == (c["B"], c["D"][0], c["L"])
        exact = all(bool((t.bfloat16().float() == t).all()) for t in (img, words, na))
        assert exact == c["bf16"]
        assert abs(float(img.std()) - 0.5) < 0.02
    assert sc.inputs("f32", 64, no_attn=False)[2] is None
