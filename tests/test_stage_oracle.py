"""The stage criterion of tests/stagelib.py, proved on the reference alone (CPU).

ViT-S, B = 2, T = 2, 70 x 98 (4 frames of 5 x 7 patches), synthetic recipe weights rounded to fp16.
For every stage (encoder taps, reassemble, the four motion modules, the four fusion blocks, the head) the
reference ``r`` and the bars 4 x O16(all) are computed once and shared.

* The unmutated other placement, O16(matmul), passes the criterion on every stage (measured: worst slice
  E 0.08 .. 0.29 of the bar, max|y - r| 0.05 .. 0.25 of its bar; O16(all) itself sits at 0.25).
* Every localized mutant of O16(all) fails it: last column / row / pixel / token of the last frame, first
  token of the first frame, a frame replaced by its neighbour, the PE table shifted by one frame inside
  temporal_module, batch 1's frames taken from batch 0, ``sel`` off by one.  Measured worst slice E of the
  output mutants: 0.44 .. 0.52 for a zeroed last column, 0.09 .. 0.73 for a copied last row, 0.07 .. 0.35 for
  a last pixel from the frame before, 1.0 .. 1.4 for the tokens, 0.3 .. 1.7 for whole frames, against bars of
  7.5e-4 .. 4.8e-3: the weakest mutant (last pixel of the depth) is 45x its bar.
"""
import functools
import os

import pytest
import torch

import stagelib as L
from helpers import recipe_state_dict

B, T = 2, 2


@functools.lru_cache(maxsize=None)
def clip():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    g = torch.Generator().manual_seed(21)
    x = torch.randn(B, T, 3, 70, 98, generator=g)
    return L.Clip(L.round_weights(recipe_state_dict("vits")), "vits", x)


@functools.lru_cache(maxsize=None)
def stage(name):
    """(r, bars, O16(all)) of a stage: computed once, shared, never modified."""
    c = clip()
    r, bars = c.bars(name)
    return r, bars, c.outputs(name, "all")


@pytest.mark.parametrize("name", L.STAGES)
def test_other_placement_passes(name):
    r, bars, _ = stage(name)
    y = clip().outputs(name, "matmul")
    for k in r:
        rE, rmax = L.check_fp16(f"{name}/{k} O16(matmul)", y[k], r[k], bars[k])
        assert rE <= 1.0 and rmax <= 1.0


def test_reference_passes_and_o16_sits_at_a_quarter():
    r, bars, o = stage("head")
    assert L.passes_fp16(r["depth"], r["depth"], bars["depth"])
    rE, _, rmax, lines = L.evaluate(o["depth"], r["depth"], bars["depth"].E, bars["depth"].max)
    assert not lines and abs(rE - 1 / L.FACTOR) < 1e-12 and abs(rmax - 1 / L.FACTOR) < 1e-12


def _last_column_zero(y):
    y[-1, ..., -1] = 0


def _last_row_copied(y):
    y[-1, :, -1] = y[-1, :, -2]


def _last_pixel_from_frame_before(y):
    y[-1, :, -1, -1] = y[-2, :, -1, -1]


def _last_token_copied(y):
    y[-1, -1] = y[-1, -2]


def _last_token_zero(y):
    y[-1, -1] = 0


def _first_token_zero(y):
    y[0, 0] = 0


def _frame_from_neighbour(y):
    y[1] = y[2]


def _batch1_from_batch0(y):
    y[T:2 * T] = y[:T]


MAP_MUTANTS = [_last_column_zero, _last_row_copied, _last_pixel_from_frame_before, _frame_from_neighbour,
               _batch1_from_batch0]
TOKEN_MUTANTS = [_last_token_copied, _last_token_zero, _first_token_zero, _frame_from_neighbour, _batch1_from_batch0]
CASES = ([("reassemble", f"layer{i}", m) for i in (1, 2, 3, 4) for m in MAP_MUTANTS]
         + [(s, s, m) for s in ("mm0", "mm1", "mm2", "mm3", "fus4", "fus3", "fus2", "fus1") for m in MAP_MUTANTS]
         + [("head", "depth", m) for m in MAP_MUTANTS]
         + [("encode", f"tap{i}", m) for i in range(4) for m in TOKEN_MUTANTS])


@pytest.mark.parametrize("name,key,mutant", CASES, ids=[f"{k}-{m.__name__[1:]}" for _, k, m in CASES])
def test_output_mutant_fails(name, key, mutant):
    r, bars, o = stage(name)
    y = o[key].clone()
    mutant(y)
    assert not torch.equal(y, o[key])
    with pytest.raises(L.StageFailure, match=f"stage {name}/{key}") as ei:
        L.check_fp16(f"{name}/{key}", y, r[key], bars[key])
    print(ei.value)
    assert "slice [frame" in str(ei.value) and "bar" in str(ei.value)


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_pe_shifted_by_one_frame_fails(k):
    """temporal_module with every attention block's PE table shifted by one frame (row t holds row t + 1)."""
    c = clip()
    r, bars, _ = stage(f"mm{k}")
    sd = dict(c.sd32)
    n = 0
    for key, v in c.sd32.items():
        if key.startswith(f"head.motion_modules.{k}.") and key.endswith("pos_encoder.pe"):
            sd[key] = torch.roll(v, -1, 1)
            n += 1
    assert n == 2
    y = c.outputs(f"mm{k}", "all", sd=sd)
    with pytest.raises(L.StageFailure, match=f"stage mm{k}"):
        L.check_fp16(f"mm{k}", y[f"mm{k}"], r[f"mm{k}"], bars[f"mm{k}"])


@pytest.mark.parametrize("skip", [False, True])
def test_sel_off_by_one_fails(skip):
    """Streaming head: depth asked for frames ``sel`` of a 4-frame clip; path_3 cut one frame too late."""
    c = clip4()
    sel = [0, 2]
    r, bars = c.bars("head", sel=sel, skip_tmp_block=skip)
    ok = c.outputs("head", "matmul", sel=sel, skip_tmp_block=skip)["depth"]
    L.check_fp16("head(sel)", ok, r["depth"], bars["depth"])
    l1, l2, l3, l4 = (l.float() for l in c.layers)
    bad = L.run(lambda: L.O.head_from_layers(c.sd32, l1[sel], l2[sel], l3, l4, c.ph, c.pw, c.T, skip,
                                             sel=[s + 1 for s in sel]), "all")
    with pytest.raises(L.StageFailure, match="stage head"):
        L.check_fp16("head(sel)", bad, r["depth"], bars["depth"])


@functools.lru_cache(maxsize=None)
def clip4():
    """The same four frames as one clip of T = 4 (streaming is B = 1)."""
    c = clip()
    return L.Clip(c.sd32, "vits", c.x.view(1, B * T, 3, 70, 98), need_head=False)


def test_slices_cover_every_element():
    """Ring classes partition a map (also a 2 x 3 one without interior), token parts a token matrix, channel
    blocks the channels (a last partial block included): a unit error anywhere moves exactly two slices."""
    for h, w in ((2, 3), (1, 1), (5, 7)):
        m = L.ring_masks(h, w)
        assert bool((m["corner"].int() + m["edge"].int() + m["interior"].int() == 1).all())
    r = torch.ones(2, 70, 2, 3)
    names = [n for n, _ in L.slice_errors(r, r)]
    assert len(names) == 2 * 2 + 2 * 2 and not any("interior" in n for n in names)
    for idx in ((1, 69, 1, 2), (0, 0, 0, 1)):
        y = r.clone()
        y[idx] += 1
        assert sum(e > 0 for _, e in L.slice_errors(y, r)) == 2
    r = torch.ones(3, 5, 130)
    y = r.clone()
    y[2, 4, 129] = float("nan")
    bad = [n for n, e in L.slice_errors(y, r) if e == float("inf")]
    assert bad == ["frame 2 / last token", "frame 2 / channels 128..129"]
    assert L.max_abs(y, r) == float("inf")


def test_round_weights_and_proxy_restore():
    sd = L.round_weights(recipe_state_dict("vits"))
    w = sd["pretrained.blocks.0.attn.qkv.weight"]
    assert torch.equal(w, w.half().float())
    for k in ("head.scratch.output_conv2.0.weight", "pretrained.pos_embed", "pretrained.blocks.0.attn.qkv.bias"):
        assert torch.equal(sd[k], recipe_state_dict("vits")[k].float())
    import torch.nn.functional as F
    with pytest.raises(ZeroDivisionError):
        with L.fp16_storage("all"):
            assert L.O.F is not F
            y = L.O.F.linear(torch.full((1, 1), 1 / 3), torch.ones(1, 1))
            assert float(y) == float(torch.tensor(1 / 3).half()) and L.O.F.softmax is F.softmax
            1 / 0
    assert L.O.F is F
