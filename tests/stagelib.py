"""Stage-by-stage parity against the oracle, slice by slice (shared by test_stage_oracle.py and
test_gpu_stages.py; no tests here).

The whole-clip bar (rel-L1 <= 1e-3 on the final depth) cannot see a fault confined to one frame, one
border or one token: it is averaged away.  Here each stage of the clip forward (encoder taps, reassemble,
temporal module, fusion block, head) is fed the oracle's input of that stage rounded to fp16, so errors do
not compound, and its output is held to the reference on every *slice*: each (frame, ring class) of a map,
each (frame, first / last / other tokens) of a token matrix and each (frame, 64-channel block) of either.

* Reference ``r``: the oracle's own stage function (oracle/vda_oracle.py) on ``round_weights`` weights
  (every weight matrix rounded to fp16, as the kernels hold them; biases, norm affines, position tables and
  the output_conv2 weights stay fp32, as the kernels hold those) and the fp16-rounded stage input, in
  float64 where the function allows it (``head_from_layers`` casts to float inside: fp32 there).
* fp16-storage oracle ``O16``: the same function with the output of every listed ``F.*`` op rounded through
  fp16 (``fp16_storage``: a proxy stands in for ``vda_oracle.F`` for the duration of a call; the oracle is
  not edited).  Placement ``all`` rounds linear, conv2d, conv_transpose2d, layer_norm, group_norm, gelu,
  relu, interpolate and batch_norm; ``matmul`` only the first three.  Its distance from ``r`` is the
  reference's own estimate of what fp16 storage costs in that stage.  It runs in fp32 (1e-7 against the
  5e-4 it estimates).
* One rounding was added to ``O16(all)`` after the first GPU run, for the encoder stage only: the kernels
  keep the encoder's residual stream ``t`` in fp16 (documented: DESIGN.md, the proj / fc2 epilogues'
  packed-fp16 residual adds; test_forward_massive_residual_channels), so there ``O16(all)`` also rounds
  every tensor add (``_RoundedAdds``: the position-table add and the two residual adds per block).
  Without it O16 put ViT-L's last tap at E 5.6e-4, max 3.3e-3, the GPU at 1.5e-3 and 1.69e-2 (1.24x
  the max bar); with it O16 gives E 1.48e-3, max 1.66e-2, the GPU's figures.  The way fp16_bounds.py
  models the attention's P rounding.
* Statistics: ``E(y, s) = sum_s |y - r| / sum_s |r|`` per slice s, and ``max |y - r|`` per output.
* Criterion, fp16 path: every slice has ``E(y, s) <= 4 * max_s' E(O16(all), s')`` and
  ``max|y - r| <= 4 * max|O16(all) - r|``; both bars come from the reference alone.  fp32 mode: every slice
  has ``E <= 1e-5``.  Why 4: the kernels round in other places than O16 (fused epilogues keep fp32 where
  O16 rounds, the attention rounds P, the encoder's residual stream is fp16), two rounding placements of
  the reference itself differ by up to 1.22x in the max over slices, and the smallest localized fault
  measured is several hundred times the bar.
"""
import contextlib
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F
from torch.overrides import TorchFunctionMode

from helpers import vda_oracle

O = vda_oracle
MATMUL_OPS = ("linear", "conv2d", "conv_transpose2d")
ALL_OPS = MATMUL_OPS + ("layer_norm", "group_norm", "gelu", "relu", "interpolate", "batch_norm")
PLACEMENTS = {"matmul": MATMUL_OPS, "all": ALL_OPS}
FACTOR = 4.0     # fp16 path: y may be this many times O16(all)'s own distance from r
FP32_BAR = 1e-5  # fp32 mode: the project's fp32 parity bar, per slice
CBLOCK = 64


def r16(t: torch.Tensor) -> torch.Tensor:
    """t rounded to fp16, in t's dtype."""
    return t.to(torch.float16).to(t.dtype)


# ---------------------------------------------------------------------------------------------
# weights, O16
# ---------------------------------------------------------------------------------------------
def round_weights(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """fp32 state_dict whose values are the numbers the kernels multiply by: weight matrices rounded to
    fp16; 1-D parameters, cls / position tables, BatchNorm statistics and output_conv2 (fp32 in the depth
    tail) unchanged.  Loading it into the model makes the model's own fp16 packing of them exact."""
    out = {}
    for k, v in sd.items():
        v = v.detach().float().cpu()
        if k.endswith(".weight") and v.dim() >= 2 and ".output_conv2." not in k:
            v = r16(v)
        out[k] = v
    return out


def cast(sd: Dict[str, torch.Tensor], dtype) -> Dict[str, torch.Tensor]:
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


class _RoundedF:
    """torch.nn.functional with the outputs of the named ops rounded through fp16."""

    def __init__(self, names: Sequence[str]):
        self._names = frozenset(names)

    def __getattr__(self, name):
        f = getattr(F, name)
        if name not in self._names:
            return f

        def rounded(*a, **k):
            return r16(f(*a, **k))
        return rounded


class _RoundedAdds(TorchFunctionMode):
    """Every floating-point tensor ``+`` stores fp16.  In ``encoder_taps`` those are the position-table add
    and the two residual adds of each block, i.e. the residual stream ``t``."""
    ADDS = (torch.Tensor.add, torch.Tensor.__add__, torch.Tensor.__radd__, torch.add)

    def __torch_function__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        if func in self.ADDS and isinstance(out, torch.Tensor) and out.is_floating_point():
            out = r16(out)
        return out


@contextlib.contextmanager
def fp16_storage(placement: Optional[str], residual: bool = False):
    """Within the block the oracle's ``F.*`` ops of ``placement`` ('all' / 'matmul') store fp16; None: as is.
    ``residual``: tensor adds store fp16 too (the encoder's fp16 residual stream, see ``Clip.outputs``)."""
    if placement is None:
        yield
        return
    saved = O.F
    O.F = _RoundedF(PLACEMENTS[placement])
    try:
        with (_RoundedAdds() if residual else contextlib.nullcontext()):
            yield
    finally:
        O.F = saved


def run(fn, placement: Optional[str] = None, residual: bool = False):
    """fn() as the reference (placement None) or as O16(placement)."""
    with torch.no_grad(), fp16_storage(placement, residual):
        return fn()


# ---------------------------------------------------------------------------------------------
# layouts: oracle NCHW maps / [BT, np, C] tokens (CPU)  <->  model NHWC maps / [BT*np, C] rows (GPU)
# ---------------------------------------------------------------------------------------------
def map_to_nhwc(x: torch.Tensor, dtype=torch.float16, device="cuda") -> torch.Tensor:
    return x.permute(0, 2, 3, 1).to(dtype).contiguous().to(device)


def map_to_rows(x: torch.Tensor, dtype=torch.float16, device="cuda") -> torch.Tensor:
    return map_to_nhwc(x, dtype, device).view(-1, x.shape[1])


def map_from_nhwc(y: torch.Tensor) -> torch.Tensor:
    return y.detach().to("cpu", torch.float64).permute(0, 3, 1, 2)


def map_from_rows(y: torch.Tensor, BT: int, h: int, w: int) -> torch.Tensor:
    return map_from_nhwc(y.view(BT, h, w, -1))


def tokens_to_rows(t: torch.Tensor, dtype=torch.float16, device="cuda") -> torch.Tensor:
    return t.reshape(-1, t.shape[-1]).to(dtype).contiguous().to(device)


def tokens_from_rows(y: torch.Tensor, BT: int) -> torch.Tensor:
    return y.detach().to("cpu", torch.float64).view(BT, -1, y.shape[-1])


# ---------------------------------------------------------------------------------------------
# the oracle's stages, with the inputs of the inner ones exposed
# ---------------------------------------------------------------------------------------------
def project_taps(sd, feats: List[torch.Tensor], ph: int, pw: int) -> List[torch.Tensor]:
    """The oracle's projects.i 1x1 conv (the first op of ``reassemble``) on each tap, as tokens
    [BT, np, oc_i]: what the encoder stage returns where it projects the taps itself."""
    out = []
    for i, t in enumerate(feats):
        x = t.permute(0, 2, 1).reshape(t.shape[0], t.shape[-1], ph, pw)
        x = O.F.conv2d(x, sd[f"head.projects.{i}.weight"], sd[f"head.projects.{i}.bias"])
        out.append(x.flatten(2).transpose(1, 2))
    return out


FUSION_OF = {4: "head.scratch.refinenet4.", 3: "head.scratch.refinenet3.", 2: "head.scratch.refinenet2.",
             1: "head.scratch.refinenet1."}


def head_inputs(sd, l1, l2, l3, l4, T: int) -> dict:
    """The input of every inner stage of ``head_from_layers``, by the oracle's own stage functions in the
    order of dpt_temporal.py:71-99: ``mm{k}`` the map entering motion module k, ``fus{i}`` = (inputs,
    size) of refinenet i.  Every stage input is rounded to fp16 before the next stage runs on it, so each
    entry is exactly what a stage test feeds."""
    mm, s = "head.motion_modules.", "head.scratch."
    c = {}
    c["mm0"], c["mm1"] = r16(l3), r16(l4)
    t3 = r16(O.temporal_module(sd, mm + "0.", c["mm0"], T))
    t4 = r16(O.temporal_module(sd, mm + "1.", c["mm1"], T))
    r1, r2, r3, r4 = (r16(F.conv2d(r16(x), sd[f"{s}layer{i}_rn.weight"], padding=1))
                      for i, x in ((1, l1), (2, l2), (3, t3), (4, t4)))
    c["fus4"] = ([r4], tuple(r3.shape[2:]))
    c["mm2"] = r16(O._fusion(sd, FUSION_OF[4], *c["fus4"]))
    p4 = r16(O.temporal_module(sd, mm + "2.", c["mm2"], T))
    c["fus3"] = ([p4, r3], tuple(r2.shape[2:]))
    c["mm3"] = r16(O._fusion(sd, FUSION_OF[3], *c["fus3"]))
    p3 = r16(O.temporal_module(sd, mm + "3.", c["mm3"], T))
    c["fus2"] = ([p3, r2], tuple(r1.shape[2:]))
    p2 = r16(O._fusion(sd, FUSION_OF[2], *c["fus2"]))
    c["fus1"] = ([p2, r1], None)
    return c


# ---------------------------------------------------------------------------------------------
# slices and statistics
# ---------------------------------------------------------------------------------------------
def _ratio(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
    """num / den; 0 where both are 0, inf where only den is (or num is not finite)."""
    e = num / den
    e = torch.where((den == 0) & (num == 0), torch.zeros_like(e), e)
    return torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))


def ring_masks(h: int, w: int) -> Dict[str, torch.Tensor]:
    """corner: the (up to) four corner pixels; edge: the rest of the border; interior: everything else."""
    border = torch.zeros(h, w, dtype=torch.bool)
    border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
    corner = torch.zeros(h, w, dtype=torch.bool)
    for i in (0, h - 1):
        for j in (0, w - 1):
            corner[i, j] = True
    return {"corner": corner, "edge": border & ~corner, "interior": ~border}


def slice_errors(y: torch.Tensor, r: torch.Tensor) -> List[Tuple[str, float]]:
    """[(slice name, E(y, slice))] over every slice of the output: y, r of one shape, a map [N, C, H, W]
    or a token matrix [N, np, C].  Empty slices (no interior in a 2-row map) do not exist."""
    y, r = y.detach().to("cpu", torch.float64), r.detach().to("cpu", torch.float64)
    assert y.shape == r.shape, f"shapes {tuple(y.shape)} vs {tuple(r.shape)}"
    assert bool(torch.isfinite(r).all()), "reference is not finite"
    d = (y - r).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
    a = r.abs()
    out = []
    if y.dim() == 4:
        N, C, h, w = y.shape
        for name, m in ring_masks(h, w).items():
            if not bool(m.any()):
                continue
            e = _ratio((d * m).sum((1, 2, 3)), (a * m).sum((1, 2, 3)))
            out += [(f"frame {n} / ring {name}", float(e[n])) for n in range(N)]
        dc, ac = d.sum((2, 3)), a.sum((2, 3))
    elif y.dim() == 3:
        N, S, C = y.shape
        parts = [("first token", slice(0, 1)), ("last token", slice(S - 1, S))]
        if S > 2:
            parts.append(("other tokens", slice(1, S - 1)))
        for name, sl in parts:
            e = _ratio(d[:, sl].sum((1, 2)), a[:, sl].sum((1, 2)))
            out += [(f"frame {n} / {name}", float(e[n])) for n in range(N)]
        dc, ac = d.sum(1), a.sum(1)
    else:
        raise ValueError(f"a map [N, C, H, W] or tokens [N, np, C], got {tuple(y.shape)}")
    for c0 in range(0, C, CBLOCK):
        c1 = min(C, c0 + CBLOCK)
        e = _ratio(dc[:, c0:c1].sum(1), ac[:, c0:c1].sum(1))
        out += [(f"frame {n} / channels {c0}..{c1 - 1}", float(e[n])) for n in range(N)]
    return out


def max_abs(y: torch.Tensor, r: torch.Tensor) -> float:
    d = (y.detach().to("cpu", torch.float64) - r.detach().to("cpu", torch.float64)).abs()
    return float("inf") if not bool(torch.isfinite(d).all()) else float(d.max())


class Bars:
    """The two bars of one stage output, from the reference alone."""

    def __init__(self, o16: torch.Tensor, r: torch.Tensor):
        self.healthy_E = max(e for _, e in slice_errors(o16, r))
        self.healthy_max = max_abs(o16, r)
        self.E = FACTOR * self.healthy_E
        self.max = FACTOR * self.healthy_max
        assert 0 < self.E < float("inf") and 0 < self.max < float("inf"), "O16 gives no usable bar"


class StageFailure(AssertionError):
    pass


def evaluate(y, r, bar_E: float, bar_max: Optional[float]):
    """(worst E / bar, its slice, max|y - r| / bar or None, [failure lines])."""
    errs = slice_errors(y, r)
    name, worst = max(errs, key=lambda t: t[1])
    bad = [(n, e) for n, e in errs if not e <= bar_E]
    lines = [f"slice [{n}]: E = sum|y - r| / sum|r| = {e:.3e} > bar {bar_E:.3e} ({e / bar_E:.2f}x)" for n, e in bad[:8]]
    if len(bad) > 8:
        lines.append(f"... and {len(bad) - 8} more slices of {len(errs)}")
    rmax = None
    if bar_max is not None:
        m = max_abs(y, r)
        rmax = m / bar_max
        if not m <= bar_max:
            lines.append(f"whole output: max|y - r| = {m:.3e} > bar {bar_max:.3e} ({rmax:.2f}x)")
    return worst / bar_E, name, rmax, lines


RATIOS: Dict[str, Tuple[float, float]] = {}  # stage -> worst (E / bar, max / bar) seen in this process


def check_fp16(stage: str, y, r, bars: Bars) -> Tuple[float, float]:
    """The fp16 criterion on one stage output; raises StageFailure naming stage, slice, statistic, bar."""
    rE, name, rmax, lines = evaluate(y, r, bars.E, bars.max)
    print(f"{stage}: worst E / bar = {rE:.3f} at [{name}]; max|y - r| / bar = {rmax:.3f} "
          f"(bars {FACTOR:g} x O16(all): E {bars.E:.3e}, max {bars.max:.3e})")
    old = RATIOS.get(stage, (0.0, 0.0))
    RATIOS[stage] = (max(old[0], rE), max(old[1], rmax))
    if lines:
        raise StageFailure(f"stage {stage} (fp16, bars = {FACTOR:g} x O16(all)):\n  " + "\n  ".join(lines))
    return rE, rmax


def check_fp32(stage: str, y, r) -> float:
    """fp32 mode: E <= 1e-5 on every slice."""
    rE, name, _, lines = evaluate(y, r, FP32_BAR, None)
    print(f"{stage}: fp32 worst E / bar = {rE:.3f} at [{name}] (bar {FP32_BAR:g})")
    if lines:
        raise StageFailure(f"stage {stage} (fp32 mode, bar {FP32_BAR:g}):\n  " + "\n  ".join(lines))
    return rE


def passes_fp16(y, r, bars: Bars) -> bool:
    return not evaluate(y, r, bars.E, bars.max)[3]


# ---------------------------------------------------------------------------------------------
# one clip through the reference, stage by stage
# ---------------------------------------------------------------------------------------------
class Clip:
    """The reference chain of one clip x [B, T, 3, H, W] on ``round_weights`` weights ``sd``: the fp16-rounded
    input of every stage (float64, computed once, never modified), and ``outputs(stage, placement)``: that
    stage alone on its input as ``r`` (placement None: float64, the head fp32) or ``O16(placement)`` (fp32).

    Stages and their outputs: ``encode`` -> tap0..3 (tokens) and, with readout weights, cls0..3 ([BT, 1, C]);
    ``reassemble`` -> layer1..4; ``mm0..3`` -> the map out of that motion module; ``fus4..1`` -> the map out
    of that refinenet; ``head`` -> depth [n, 1, H, W] (``skip_tmp_block`` / ``sel`` as head_from_layers;
    ``sel12``: the frames layer_1/2 carry, ``sel`` itself by default)."""

    def __init__(self, sd, enc: str, x: torch.Tensor, need_head: bool = True):
        self.enc, self.sd32 = enc, sd
        self.sd64 = cast(sd, torch.float64)
        self.B, self.T, _, H, W = x.shape
        self.BT = self.B * self.T
        self.ph, self.pw = H // O.PATCH, W // O.PATCH
        self.readout = "head.readout_projects.0.0.weight" in sd
        self.x = r16(x.double().flatten(0, 1))
        feats, cls = run(lambda: O.encoder_taps(self.sd64, enc, self.x, return_cls=True))
        self.feats, self.cls = [r16(f) for f in feats], [r16(c) for c in cls]
        self.layers = [r16(l) for l in run(lambda: O.reassemble(self.sd64, self.feats, self.ph, self.pw, self.cls))]
        self.inner = run(lambda: head_inputs(self.sd64, *self.layers, self.T)) if need_head else None

    def sd(self, dtype):
        return self.sd64 if dtype == torch.float64 else self.sd32

    def outputs(self, stage: str, placement: Optional[str] = None, skip_tmp_block: bool = False, sel=None,
                sel12=None, sd=None) -> Dict[str, torch.Tensor]:
        dt = torch.float64 if placement is None and stage != "head" else torch.float32
        sd = self.sd(dt) if sd is None else cast(sd, dt)
        if stage == "encode":
            feats, cls = run(lambda: O.encoder_taps(sd, self.enc, self.x.to(dt), return_cls=True), placement,
                             placement == "all")
            out = {f"tap{i}": f for i, f in enumerate(feats)}
            if self.readout:
                out.update({f"cls{i}": c[:, None] for i, c in enumerate(cls)})
            return out
        if stage == "encode_projected":
            def fn():
                feats = O.encoder_taps(sd, self.enc, self.x.to(dt))
                return project_taps(sd, feats, self.ph, self.pw)
            return {f"tap{i}": f for i, f in enumerate(run(fn, placement, placement == "all"))}
        if stage == "reassemble":
            lay = run(lambda: O.reassemble(sd, [f.to(dt) for f in self.feats], self.ph, self.pw,
                                           [c.to(dt) for c in self.cls]), placement)
            return {f"layer{i + 1}": l for i, l in enumerate(lay)}
        if stage.startswith("mm"):
            k = int(stage[2:])
            return {stage: run(lambda: O.temporal_module(sd, f"head.motion_modules.{k}.", self.inner[stage].to(dt),
                                                         self.T), placement)}
        if stage.startswith("fus"):
            xs, size = self.inner[stage]
            return {stage: run(lambda: O._fusion(sd, FUSION_OF[int(stage[3:])], [t.to(dt) for t in xs], size=size),
                               placement)}
        if stage == "head":
            l1, l2, l3, l4 = (l.to(dt) for l in self.layers)
            if sel is not None:  # streaming: layer_1/2 carry only the frames whose depth is asked for (sel12:
                # where a negative context index names another frame there than in path_3, StreamEngine.predict)
                l1, l2 = l1[list(sel12 or sel)], l2[list(sel12 or sel)]
            return {"depth": run(lambda: O.head_from_layers(sd, l1, l2, l3, l4, self.ph, self.pw, self.T,
                                                            skip_tmp_block, sel=sel), placement)}
        raise KeyError(stage)

    def bars(self, stage: str, **kw) -> Tuple[Dict[str, torch.Tensor], Dict[str, Bars]]:
        """(r, bars) of every output of the stage: the reference and 4 x O16(all)'s distance from it."""
        r = self.outputs(stage, None, **kw)
        o = self.outputs(stage, "all", **kw)
        return r, {k: Bars(o[k], r[k]) for k in r}


STAGES = ("encode", "reassemble", "mm0", "mm1", "mm2", "mm3", "fus4", "fus3", "fus2", "fus1", "head")
