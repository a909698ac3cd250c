"""Case table of the block-row (data-parallel) loss tests: shapes, caption lengths, the tile plan every case is meant
to produce, and the seeded inputs.  Shared by tests/test_sharded_cases_host.py (checks the plans on the CPU, so a change
of the planner cannot silently take a kernel out of the GPU tests) and tests/test_gpu_sharded_loss.py.

Caption lengths are deliberately NOT sorted: the long sentences are diagonals of the later ranks (rank r owns images
and diagonal sentences [r * B / P, (r + 1) * B / P)).

Work-item kinds of a K1 plan (include/glr.h): SINGLE = an item of the single-tile kernel (one ordinary tile that found
no partner, or one sentence of more than two tiles / any multi-tile sentence without pairing, worked in sweeps);
LONG_PAIR = the two tiles of one 65..128-word sentence; PAIR = two consecutive ordinary tiles."""

import numpy as np
import torch

import golden_inputs as gi

SINGLE, LONG_PAIR, PAIR = 1, 2, 3

CASES = {
    # 19 x 19 regions + the no-attention vector = 362 regions, S_pad 384: the only shape that pairs tiles.  At D = 256
    # the ordinary pairs run the per-tile kernel (glr_local_attn_t1.hip), at D = 128 every pair runs the pair kernel.
    "full_bf16": dict(
        B=15, H=19, W=19, L=200, D=(256, 128), worlds=(3,), bf16=True, no_attn=(True,), capacity=64, allow_pairs=True,
        cap_lens=[9, 5, 2, 1, 3, 64, 40, 33, 23, 17, 200, 100, 70, 64, 12],
        n_tiles=13, n_single=2, n_pair=4, n_long_pair=2, single_nsub=[4, 0],
        kinds={0: PAIR, 1: PAIR, 2: PAIR, 3: PAIR, 4: PAIR, 5: PAIR, 6: PAIR, 7: SINGLE, 8: SINGLE, 9: PAIR,
               10: SINGLE, 11: LONG_PAIR, 12: LONG_PAIR, 13: PAIR, 14: PAIR},
        diag_kinds={SINGLE, LONG_PAIR, PAIR}, seed=7100),
    # 14 x 14 regions + the no-attention vector = 197 regions, S_pad 256: the non-FULL single-tile kernel, no pairing
    "nonfull_bf16": dict(
        B=6, H=14, W=14, L=130, D=(128,), worlds=(2, 3), bf16=True, no_attn=(True,), capacity=64, allow_pairs=False,
        cap_lens=[5, 130, 64, 65, 1, 77],
        n_tiles=9, n_single=5, n_pair=0, n_long_pair=0, single_nsub=[3, 2, 2, 0, 0],
        kinds={i: SINGLE for i in range(6)}, diag_kinds={SINGLE}, seed=7200),
    # fp32 operands: 32-word tiles, never paired; 25 / 26 regions (S_pad 64)
    "f32": dict(
        B=6, H=5, W=5, L=40, D=(64,), worlds=(2, 3), bf16=False, no_attn=(True, False), capacity=32, allow_pairs=False,
        cap_lens=[3, 33, 1, 40, 12, 32],
        n_tiles=6, n_single=4, n_pair=0, n_long_pair=0, single_nsub=[2, 2, 0, 0],
        kinds={i: SINGLE for i in range(6)}, diag_kinds={SINGLE}, seed=7300),
}

# regulariser weights (no-attention, divergence, entropy): the reference's training flags; the no-attention score
# needs the extra column
AUX_WEIGHTS = {True: (1.0, 0.1, 1.0), False: (None, 0.1, 1.0)}
TEMPS = (4.0, 5.0, 10.0)


def sentence_kinds(host):
    """sentence -> work-item kind, from the int32 plan buffer of glr_plan_build (TilePlan.host; layout: include/glr.h):
    the header counts and the arrays tile_first, order, tile_nsub, single_tile, pair_tile."""
    h = np.asarray(host)
    n_sent, n_tiles, _, n_order, n_single, n_pair, n_long_pair = (int(v) for v in h[:7])
    off = [int(v) for v in h[8:16]]
    tile_first = h[off[2]:off[2] + n_tiles + 1]
    order = h[off[3]:off[3] + n_order]
    tile_nsub = h[off[4]:off[4] + n_tiles]
    single_tile = h[off[5]:off[5] + n_single]
    pair_tile = h[off[6]:off[6] + n_pair]
    kinds = {}

    def claim(tiles, kind):
        for t in tiles:
            for s in order[tile_first[t]:tile_first[t + 1]]:
                assert kinds.setdefault(int(s), kind) == kind, (int(s), kind, kinds)

    for t in single_tile:
        claim(range(int(t), int(t) + max(int(tile_nsub[t]), 1)), SINGLE)
    for k, t in enumerate(pair_tile):
        claim((int(t), int(t) + 1), LONG_PAIR if k < n_long_pair else PAIR)
    assert sorted(kinds) == list(range(n_sent)), kinds          # every sentence belongs to exactly one kind of item
    return kinds


def diagonal_kinds(host, B, world):
    """kinds of the items that hold the diagonal sentences of the ranks with a non-zero image offset"""
    kinds = sentence_kinds(host)
    return {kinds[i] for i in range(B // world, B)}


def inputs(name, D, no_attn=True):
    """fp32 CPU tensors (img [B, D, H, W], words [B, D, L], no-attention vector [D] or None), N(0, 0.5^2); in the bf16
    cases every value is bf16-representable, so casting a leaf to bf16 is exact"""
    c = CASES[name]
    seed = c["seed"] + D
    img = torch.from_numpy(gi.normal(seed, c["B"], D, c["H"], c["W"]))
    words = torch.from_numpy(gi.normal(seed + 1, c["B"], D, c["L"]))
    na = torch.from_numpy(gi.normal(seed + 2, D)) if no_attn else None
    if c["bf16"]:
        img, words = img.bfloat16().float(), words.bfloat16().float()
        na = None if na is None else na.bfloat16().float()
    return img, words, na
