"""Operand placement: run a kernel with every operand surrounded by poison and every workspace exact and guarded.

The output-side tests (sentinel frames, per-element bounds) cannot see what a kernel READS.  A K tail masked on
one operand only, row M of a residual, a halo row before the first frame or a key row past the last head reads
whatever the allocator left next to a fresh tensor: finite, usually zero, and finite garbage times a zero-padded
partner is zero.  Here the neighbourhood is chosen.  `place` puts a tensor inside a buffer that this test owns,
at the weakest alignment the C ABI promises, with a fill value before it, after it and between the rows of a
strided view.  `run_placed` runs a call once per fill and holds it to five checks:

  (a) bit identity across fills   every output has the same bits under the zero, quiet-NaN and +Inf fills
                                  (NaN x 0 = NaN; +Inf survives the ReLU / fmaxf that turn a NaN into a number)
  (b) bound                       the zero-fill outputs meet the bound the op's own test uses (the `check` callable)
  (c) output frame                the sentinel frame around (and between the rows of) each output is intact
  (d) inputs unchanged            every input's whole buffer, surroundings included, is bitwise unchanged
  (e) workspace                   each workspace is exactly the size asked for inside a guard that stays intact,
                                  and the outputs do not depend on its contents before the call (0x00 / 0xFF bytes)

Every zone is at least max(64 KiB, 256 row pitches) long, so a masked over-read of a whole tile panel stays in
memory the test owns: a placed run cannot fault.  The module runs on the CPU (tests/test_placement.py drives it
with deliberately leaky torch "kernels") and on the GPU (tests/test_gpu_placement*.py).
"""
import torch

ZONE_MIN = 64 * 1024
ZONE_ROWS = 256
FILLS = ("zero", "nan", "inf")
SENT = -7776.0          # the output sentinel: exact in fp16 and fp32
WS_GUARD = 0x5A         # the byte around a workspace; differs from both prefill bytes
WS_PREFILLS = (0x00, 0xFF)
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def fill_value(dtype, fill):
    """The value a named fill has for an operand of `dtype`: zeros / quiet NaN / +Inf for floating point, the
    bytes 0x00 / 0xFF / 0xFF for integers.  A number is taken as it is."""
    if not isinstance(fill, str):
        return fill
    if dtype.is_floating_point:
        return {"zero": 0.0, "nan": float("nan"), "inf": float("inf")}[fill]
    return 0 if fill == "zero" else (0xFF if dtype == torch.uint8 else -1)


def bits(t):
    """t as a contiguous integer tensor of the same width: equality of bits, NaNs included."""
    return t.contiguous().view(_INT[t.element_size()])


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


class Placed:
    """A tensor inside an owned buffer.  buf: the whole buffer as uint8, its first byte on a 256-byte boundary;
    view: the operand (a typed, possibly row-strided view of buf)."""

    def __init__(self, t, *, align, fill, ld=None, device=None):
        device = t.device if device is None else torch.device(device)
        es = t.element_size()
        assert 0 <= align < 256 and align % es == 0, "align is a byte offset past a 256-byte boundary, in whole elements"
        if ld is None:
            strides = tuple(t.contiguous().stride())
            body = t.numel() * es
            # a row: the last dim of a matrix, W x C of an NHWC map; a vector has none
            pitch = (t.shape[-1] * (t.shape[-2] if t.dim() > 2 else 1) if t.dim() > 1 else 0) * es
        else:
            assert t.dim() == 2 and ld >= t.shape[1], "ld: the row pitch of a 2-D operand, in elements"
            strides = (ld, 1)
            body = t.shape[0] * ld * es
            pitch = ld * es
        zone = max(ZONE_MIN, ZONE_ROWS * pitch)
        zone = (zone + 255) // 256 * 256
        total = zone + align + body + zone
        total = (total + 255) // 256 * 256
        raw = torch.empty(total + 256, dtype=torch.uint8, device=device)
        off = (-raw.data_ptr()) % 256
        self.buf = raw[off:off + total]
        self.dtype, self.shape, self.strides, self.start = t.dtype, tuple(t.shape), strides, (zone + align) // es
        self.zone, self.body = zone, body
        self.typed(self.buf).fill_(fill_value(t.dtype, fill))
        self.view = self.view_in(self.buf)
        self.view.copy_(t)
        if not t.numel():  # an empty view has no address to check
            return
        assert self.view.data_ptr() % 256 == align
        assert self.view.data_ptr() - self.buf.data_ptr() >= zone
        assert self.buf.data_ptr() + total - (self.view.data_ptr() + body) >= zone

    def typed(self, buf):
        return buf.view(self.dtype)

    def view_in(self, buf):
        """The operand's geometry inside another uint8 buffer of the same length (a snapshot)."""
        t = self.typed(buf)
        return t.as_strided(self.shape, self.strides, t.storage_offset() + self.start)

    def outside_intact(self, value):
        """True when every byte of buf outside the view still holds `value` (the frame of an output, the guard of
        a workspace): the view's own elements are overwritten with it in a copy, which must then be uniform."""
        snap = self.buf.clone()
        self.view_in(snap).fill_(value)
        t = self.typed(snap)
        return same_bits(t, torch.full_like(t, value))


def place(t, *, align, fill, ld=None, device=None):
    """(buf, view): `view` has t's shape and values (row pitch `ld` elements for a 2-D operand) and starts exactly
    `align` bytes past a 256-byte boundary; everything else in `buf` (uint8, the zone before the view, the zone
    after it, the gaps between strided rows) holds `fill` (a name of FILLS or a value of t's dtype).  Each zone is at
    least max(64 KiB, 256 row pitches) bytes."""
    p = Placed(t, align=align, fill=fill, ld=ld, device=device)
    return p.buf, p.view


class In:
    """An input operand: a CPU tensor of the kernel's dtype, its byte alignment (16 for fp16 matrices and maps,
    else what include/vda.h states) and, for a row-strided 2-D operand, its row pitch in elements."""

    def __init__(self, t, align=16, ld=None):
        self.t, self.align, self.ld = t, align, ld


class Out:
    """An output: shape, dtype, alignment, row pitch.  init: the contents before the call (an in-place residual);
    else the output starts as the sentinel, so an element the kernel does not store fails the bound."""

    def __init__(self, shape, dtype=torch.float16, align=16, ld=None, init=None, sentinel=SENT):
        self.shape, self.dtype, self.align, self.ld, self.init, self.sentinel = tuple(shape), dtype, align, ld, init, sentinel


class PlacementError(AssertionError):
    pass


def _run(call, operands, outputs, workspaces, fills, prefill, device):
    """One run: fills maps operand name -> fill.  Returns (outputs as CPU clones, list of failures (c)-(e))."""
    ins = {k: Placed(o.t, align=o.align, fill=fills[k], ld=o.ld, device=device) for k, o in operands.items()}
    before = {k: p.buf.clone() for k, p in ins.items()}
    outs = {}
    for k, o in outputs.items():
        t = torch.full(o.shape, o.sentinel, dtype=o.dtype) if o.init is None else o.init
        outs[k] = Placed(t, align=o.align, fill=o.sentinel, ld=o.ld, device=device)
    wss = {}
    for k, nbytes in workspaces.items():
        wss[k] = Placed(torch.full((max(int(nbytes), 0),), prefill, dtype=torch.uint8), align=16, fill=WS_GUARD, device=device)
    call({k: p.view for k, p in ins.items()}, {k: p.view for k, p in outs.items()}, {k: p.view for k, p in wss.items()})
    if device.type == "cuda":
        torch.cuda.synchronize()
    bad = []
    for k, p in outs.items():
        if not p.outside_intact(outputs[k].sentinel):
            bad.append(f"(c) output frame: a store outside output '{k}'")
    for k, p in ins.items():
        if not torch.equal(p.buf, before[k]):
            inside = not same_bits(p.view, p.view_in(before[k]))
            bad.append(f"(d) inputs unchanged: input '{k}' was written ({'the operand itself' if inside else 'its surroundings'})")
    for k, p in wss.items():
        if not p.outside_intact(WS_GUARD):
            bad.append(f"(e) workspace guard: a store outside the {int(workspaces[k])} bytes of workspace '{k}'")
    return {k: p.view.detach().to("cpu").clone() for k, p in outs.items()}, bad


def _differs(a, b):
    return [k for k in a if not same_bits(a[k], b[k])]


def run_placed(call, operands, outputs, workspaces=None, *, check=None, what="", device="cpu", fills=FILLS, tally=None):
    """Run `call(inputs, outputs, workspaces)` (three dicts of views by name) once per fill with every operand of
    `operands` (name -> In) placed in that fill, every output of `outputs` (name -> Out) framed in the sentinel and
    every workspace of `workspaces` (name -> exact byte size) guarded, and assert (a) - (e) of the module docstring.
    With workspaces (of more than 0 bytes), the zero fill also runs with the workspaces prefilled with 0xFF bytes instead of 0x00.
    check(outs) -> worst |y - ref| / bound: asserts the op's own bound on the zero-fill outputs (CPU tensors).
    On a difference between fills the run is repeated with one operand poisoned at a time, only to name the culprit.
    Returns dict(runs=, worst=, outputs= the zero-fill outputs); tally: a [runs, worst] list to add them to."""
    device = torch.device(device)
    workspaces = workspaces or {}
    zero = {k: "zero" for k in operands}
    base, bad = _run(call, operands, outputs, workspaces, zero, WS_PREFILLS[0], device)
    runs = 1
    if bad:
        raise PlacementError(f"{what}: zero fill: " + "; ".join(bad))
    worst = 0.0
    if check is not None:
        try:
            worst = float(check(base) or 0.0)
        except AssertionError as e:
            raise PlacementError(f"{what}: (b) bound: the zero-fill output misses the op's bound: {e}") from e
    for fill in fills:
        if fill == "zero":
            continue
        outs, bad = _run(call, operands, outputs, workspaces, {k: fill for k in operands}, WS_PREFILLS[0], device)
        runs += 1
        diff = _differs(base, outs)
        if diff:
            culprits = []
            for name in operands:  # one operand poisoned at a time: only to name the culprit
                one, _ = _run(call, operands, outputs, workspaces, dict(zero, **{name: fill}), WS_PREFILLS[0], device)
                if _differs(base, one):
                    culprits.append(name)
            idx = _first_diff(base[diff[0]], outs[diff[0]])
            raise PlacementError(f"{what}: (a) bit identity across fills: output {diff} under the {fill} fill differs from the "
                                 f"zero fill (first at {idx}); it depends on the surroundings of: {culprits or 'a combination of operands'}")
        if bad:
            raise PlacementError(f"{what}: {fill} fill: " + "; ".join(bad))
    if any(int(n) > 0 for n in workspaces.values()):  # a 0-byte workspace has no contents to depend on
        outs, bad = _run(call, operands, outputs, workspaces, zero, WS_PREFILLS[1], device)
        runs += 1
        diff = _differs(base, outs)
        if diff:
            culprits = []
            for name in workspaces:
                def one_ws(i, o, w, name=name):
                    for k in w:
                        if k != name:
                            w[k].zero_()
                    call(i, o, w)
                one, _ = _run(one_ws, operands, outputs, workspaces, zero, WS_PREFILLS[1], device)
                if _differs(base, one):
                    culprits.append(name)
            raise PlacementError(f"{what}: (e) workspace prefill: output {diff} depends on what the workspace held before "
                                 f"the call (0x00 against 0xFF bytes): {culprits or list(workspaces)}")
        if bad:
            raise PlacementError(f"{what}: workspace prefilled with 0xFF: " + "; ".join(bad))
    if tally is not None:
        tally[0] += runs
        tally[1] = max(tally[1], worst)
    return dict(runs=runs, worst=worst, outputs=base)


def _first_diff(a, b):
    d = (bits(a) != bits(b)).nonzero()
    return tuple(int(i) for i in d[0]) if len(d) else None


def report(family, tally):
    print(f"placement {family}: {tally[0]} (route, shape, fill) runs so far, worst zero-fill |y - ref| / bound = {tally[1]:.3f}")
