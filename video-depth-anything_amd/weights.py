"""Weights for the Video-Depth-Anything module tree: reference checkpoints or a synthetic recipe.

No checkpoint can be downloaded here (``get_weights.sh`` needs the network), so tests, goldens
and the benchmark use a deterministic synthetic recipe keyed by the reference ``state_dict`` key
names.  The same function fills the reference model (in
``tests/golden/make_golden.py``, container only) and this package's model, so both sides see
bit-identical fp32 weights without sharing code or files.

Recipe, per key (generator seeded with crc32(key)):
  * ``*.pos_encoder.pe``           sinusoidal table (motion_module.py:189-203; a buffer, not random)
  * ``*.mask_token``               zeros (unused by the forward)
  * ``*norm*.weight``              1 + 0.1 N(0,1)      (LayerNorm / GroupNorm affine)
  * ``*.gamma``                    U(0.2, 0.6)         (LayerScale)
  * 1-D ``*.bias`` / cls / pos     0.02 N(0,1)
  * conv / linear weights          N(0,1) / sqrt(fan_in)
  * ``head.scratch.output_conv2.2`` weight |N(0,1)|/sqrt(32), bias 0.05: keeps the depth strictly
    positive so the final ReLUs (dpt.py:122, video_depth.py:64) do not zero most of the map.
  * BatchNorm (use_bn=True): running_mean 0.1 N(0,1), running_var U(0.5, 1.5), num_batches_tracked 0.
"""
from __future__ import annotations

import math
import zlib
from typing import Dict, Iterable, Tuple

import torch


def _pe_table(C: int, max_len: int) -> torch.Tensor:
    pos = torch.arange(max_len).unsqueeze(1)
    div = torch.exp(torch.arange(0, C, 2) * (-math.log(10000.0) / C))
    pe = torch.zeros(1, max_len, C)
    pe[0, :, 0::2] = torch.sin(pos * div)
    pe[0, :, 1::2] = torch.cos(pos * div)
    return pe


def synthetic_tensor(key: str, shape: Tuple[int, ...]) -> torch.Tensor:
    g = torch.Generator().manual_seed(zlib.crc32(key.encode()) & 0x7FFFFFFF)
    shape = tuple(int(s) for s in shape)
    if key.endswith("pos_encoder.pe"):
        return _pe_table(shape[-1], shape[-2])
    if key.endswith("mask_token"):
        return torch.zeros(shape)
    if key == "head.scratch.output_conv2.2.weight":
        return torch.randn(shape, generator=g).abs() / math.sqrt(32.0)
    if key == "head.scratch.output_conv2.2.bias":
        return torch.full(shape, 0.05)
    leaf = key.rsplit(".", 1)[-1]
    if leaf == "num_batches_tracked":  # BatchNorm bookkeeping (use_bn=True trees)
        return torch.zeros(shape, dtype=torch.long)
    if leaf == "running_var":
        return 0.5 + torch.rand(shape, generator=g)
    if leaf == "running_mean":
        return 0.1 * torch.randn(shape, generator=g)
    if leaf == "gamma":
        return 0.2 + 0.4 * torch.rand(shape, generator=g)
    if leaf == "weight" and len(shape) == 1:  # norm affine
        return 1.0 + 0.1 * torch.randn(shape, generator=g)
    if leaf in ("bias", "cls_token", "pos_embed") or len(shape) == 1:
        return 0.02 * torch.randn(shape, generator=g)
    # conv / linear weight
    if key in ("head.resize_layers.0.weight", "head.resize_layers.1.weight"):
        fan_in = shape[0]  # ConvTranspose2d weight [in, out, k, k]: each output sums `in` taps
    else:
        fan_in = int(math.prod(shape[1:]))
    return torch.randn(shape, generator=g) / math.sqrt(fan_in)


def synthetic_state_dict(key_shapes: Iterable[Tuple[str, Tuple[int, ...]]]) -> Dict[str, torch.Tensor]:
    return {k: synthetic_tensor(k, s) for k, s in key_shapes}


# Phase groups of the sub-pixel conv (include/vda.h vda_subpixel_conv): per s, a list of (phases, window) with
# the window's source pixels relative to the phase's corner (i + [a == s - 1], j + [b == s - 1]).
_CORNER = ((-1, -1), (0, -1), (0, 0), (-1, 0))
SUBPIXEL_GROUPS = {
    2: [(((0, 0), (0, 1), (1, 0), (1, 1)), _CORNER)],
    4: [(((0, 0), (0, 3), (3, 0), (3, 3)), _CORNER),
        (((1, 0), (1, 3), (2, 0), (2, 3)), _CORNER[1:3]),
        (((0, 1), (0, 2), (3, 1), (3, 2)), _CORNER[2:4]),
        (((1, 1), (1, 2), (2, 1), (2, 2)), _CORNER[2:3])],
}


def subpixel_blocks(wt: torch.Tensor, wr: torch.Tensor, s: int) -> Dict[tuple, torch.Tensor]:
    """ConvTranspose2d(k = s) weights ``wt`` [Cin, Cmid, s, s] composed with 3x3 conv weights ``wr``
    [Cout, Cmid, 3, 3] in float64: {(a, b, di, dj): Wc [Cout, Cin]} over the non-zero blocks, with
    R[s i + a, s j + b] = sum Wc[a, b, di, dj] p[i + di, j + dj] (vda.h vda_subpixel_conv)."""
    wt, wr = wt.detach().double().cpu(), wr.detach().double().cpu()
    out: Dict[tuple, torch.Tensor] = {}
    for a in range(s):
        for b in range(s):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    di, a2 = divmod(a + dy, s)
                    dj, b2 = divmod(b + dx, s)
                    blk = wr[:, :, dy + 1, dx + 1] @ wt[:, :, a2, b2].t()
                    key = (a, b, di, dj)
                    out[key] = out[key] + blk if key in out else blk
    return out


def subpixel_bias9(bt: torch.Tensor, wr: torch.Tensor) -> torch.Tensor:
    """The ConvT bias ``bt`` [Cmid] through the taps of ``wr`` that the zero padding leaves at each of the 9
    classes (top / middle / bottom output row x left / middle / right column): float64 [9, Cout]."""
    bt, wr = bt.detach().double().cpu(), wr.detach().double().cpu()
    taps = ((0, 1), (-1, 0, 1), (-1, 0))  # dy (dx) in bounds at the first / a middle / the last row (column)
    rows = []
    for rc in range(3):
        for cc in range(3):
            rows.append(sum(wr[:, :, dy + 1, dx + 1] @ bt for dy in taps[rc] for dx in taps[cc]))
    return torch.stack(rows, 0)


def compose_subpixel(wt: torch.Tensor, bt: torch.Tensor, wr: torch.Tensor, s: int):
    """Kernel-ready operands of ``ops.subpixel_conv`` for ConvTranspose2d(wt, bt, k = s) then conv3x3(wr, pad 1):
    products in float64 from the unrounded weights, rounded once -> (w fp16, flat: the phase groups of
    SUBPIXEL_GROUPS[s], each [4 Cout, window pixels * Cin]; bias9 fp32 [9, Cout])."""
    blocks = subpixel_blocks(wt, wr, s)
    used = set()
    parts = []
    for phases, window in SUBPIXEL_GROUPS[s]:
        rows = []
        for a, b in phases:
            ea, eb = int(a == s - 1), int(b == s - 1)
            keys = [(a, b, r + ea, c + eb) for r, c in window]
            used.update(keys)
            rows.append(torch.cat([blocks[k] for k in keys], 1))  # [Cout, len(window) * Cin]
        parts.append(torch.cat(rows, 0).reshape(-1))
    assert used == set(blocks), "every non-zero block of the composition belongs to exactly one phase window"
    return torch.cat(parts).half().contiguous(), subpixel_bias9(bt, wr).float().contiguous()


def compose_pointwise_conv3(w0: torch.Tensor, b0: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor):
    """A biased 1x1 conv (w0 [Cmid, Cin, 1, 1], b0) followed - through any resize whose weights sum to 1 - by a
    zero-padded 3x3 conv (w1 [Cout, Cmid, 3, 3], b1) as ONE 3x3 conv on the 1x1 conv's input: float64 products of
    the unrounded weights, rounded once -> (w fp16 [Cout, 3, 3, Cin] NHWC, bias9 fp32 [9, Cout] =
    b1 + the 1x1 bias through the taps in bounds at each class, vda.h vda_epilogue.bias9)."""
    w0d = w0.detach().double().cpu().reshape(w0.shape[0], -1)
    w1d = w1.detach().double().cpu()
    wc = torch.einsum("omyx,mi->oyxi", w1d, w0d)
    b9 = subpixel_bias9(b0, w1) + b1.detach().double().cpu()[None, :]
    return wc.half().contiguous(), b9.float().contiguous()


def load_checkpoint(path: str) -> Dict[str, torch.Tensor]:
    """Load a reference checkpoint (video_depth_anything_{vits,vitl}.pth) without unpickling code."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(sd, dict) and "model" in sd and isinstance(sd["model"], dict):
        sd = sd["model"]
    return sd
