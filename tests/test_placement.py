"""The placement harness (tests/placement.py) has teeth: plain torch "kernels" on the CPU, one faithful and the
others leaky in exactly the ways the GPU kernels could be, each reported by the check that is there for it.

The fake kernel is y = relu?(x w^T) + bias + res in float64 on float32 operands (M = 5, N = 12, K = 40: a K
tail against the 32-wide K step it pretends to have).  An over-read is an as_strided view past the operand, the
zero-padded partner a weight matrix padded with zero columns: garbage x 0, as a kernel that masks one operand
only produces it.  Each leaky variant also runs under the fills that CANNOT see it, which proves that the
three fills and the five checks are each needed.
"""
import pytest
import torch

import placement as pl
from placement import In, Out, PlacementError, place, run_placed

M, N, K, KSTEP = 5, 12, 40, 32
KP = (K + KSTEP - 1) // KSTEP * KSTEP


def rnd(*s, seed=0):
    return torch.randn(*s, generator=torch.Generator().manual_seed(seed))


X, W, BIAS, RES = rnd(M, K, seed=1), rnd(N, K, seed=2), rnd(N, seed=3), rnd(M, N, seed=4)
REF = X.double() @ W.double().t() + BIAS.double() + RES.double()
REF_RELU = torch.relu(X.double()) @ W.double().t() + BIAS.double() + RES.double()


def over(t, rows, cols):
    """t's first element onwards as [rows, cols] with t's row pitch: rows / columns past t are its surroundings."""
    return t.as_strided((rows, cols), (t.stride(0), 1), t.storage_offset())


def wpad():
    return torch.cat([W.double(), torch.zeros(N, KP - K, dtype=torch.float64)], 1)


def operands(ldx=None):
    return dict(x=In(X, ld=ldx), w=In(W), bias=In(BIAS), res=In(RES))


def outputs():
    return dict(y=Out((M, N), torch.float32, ld=N + 4))


def check(ref):
    def f(outs):
        err = float((outs["y"].double() - ref).abs().max())
        assert err <= 1e-5, f"max error {err}"
        return err / 1e-5
    return f


def faithful(i, o, ws):
    o["y"].copy_(i["x"].double() @ i["w"].double().t() + i["bias"].double() + i["res"].double())


def k_tail_on_x_only(i, o, ws):
    """The K loop runs to KP = 64; W's tail is zero-filled, X's is read from whatever follows the row."""
    o["y"].copy_(over(i["x"], M, KP).double() @ wpad().t() + i["bias"].double() + i["res"].double())


def k_tail_behind_relu(i, o, ws):
    """The same over-read, through a pre-ReLU that is an fmaxf: NaN becomes 0, +Inf stays."""
    xr = torch.fmax(over(i["x"], M, KP).double(), torch.zeros((), dtype=torch.float64))
    o["y"].copy_(xr @ wpad().t() + i["bias"].double() + i["res"].double())


def res_row_m(i, o, ws):
    """The epilogue adds res for a whole 8-row tile and masks the rows >= M by multiplication before it folds the
    tile into a per-column sum (a second output)."""
    acc = torch.zeros(8, N, dtype=torch.float64)
    acc[:M] = i["x"].double() @ i["w"].double().t() + i["bias"].double()
    v = acc + over(i["res"], 8, N).double()
    o["y"].copy_(v[:M])
    mask = (torch.arange(8) < M).double()[:, None]
    o["colsum"].copy_((v * mask).sum(0))


def res_row_m_faithful(i, o, ws):
    faithful(i, o, ws)
    o["colsum"].copy_(o["y"].double().sum(0))


def ws_assumed_zero(i, o, ws):
    """Split-K partial sums accumulated INTO the workspace."""
    acc = ws["split"].view(torch.float32).view(M, N)
    for k0 in range(0, K, 8):
        acc += (i["x"][:, k0:k0 + 8].double() @ i["w"][:, k0:k0 + 8].double().t()).float()
    o["y"].copy_(acc.double() + i["bias"].double() + i["res"].double())


def ws_written_first(i, o, ws):
    ws["split"].zero_()
    ws_assumed_zero(i, o, ws)


def ws_overrun(i, o, ws):
    w = ws["split"]
    w.as_strided((w.numel() + 4,), (1,), w.storage_offset()).zero_()
    ws_assumed_zero(i, o, ws)


def writes_input(i, o, ws):
    faithful(i, o, ws)
    i["x"][0, 0] = 0.0


def writes_before_input(i, o, ws):
    faithful(i, o, ws)
    b = i["bias"]
    b.as_strided((1,), (1,), b.storage_offset() - 1).zero_()


def writes_past_output(i, o, ws):
    faithful(i, o, ws)
    y = o["y"]
    y.as_strided((1,), (1,), y.storage_offset() + N).zero_()  # column N of row 0: the gap of the strided output


# ---- place ----
@pytest.mark.parametrize("dtype,align,ld", [(torch.float16, 16, None), (torch.float16, 16, 56), (torch.float32, 16, None),
                                            (torch.float32, 8, None), (torch.float32, 4, 44), (torch.uint8, 1, None)])
@pytest.mark.parametrize("fill", pl.FILLS)
def test_place_geometry(dtype, align, ld, fill):
    t = (rnd(7, 40) * 10).to(dtype)
    buf, v = place(t, align=align, fill=fill, ld=ld)
    assert buf.dtype == torch.uint8 and buf.data_ptr() % 256 == 0
    assert v.data_ptr() % 256 == align and tuple(v.shape) == (7, 40) and v.stride() == (ld or 40, 1)
    assert pl.same_bits(v, t)
    es, pitch = t.element_size(), (ld or 40) * t.element_size()
    zone = max(64 * 1024, 256 * pitch)
    lead = v.data_ptr() - buf.data_ptr()
    assert lead >= zone and buf.numel() - lead - 7 * pitch >= zone
    typed = buf.view(dtype)
    want = pl.fill_value(dtype, fill)
    mask = torch.ones(typed.numel(), dtype=torch.bool)
    mask.as_strided((7, 40), (ld or 40, 1), lead // es).fill_(False)
    around = typed[mask]
    assert around.numel() == typed.numel() - 7 * 40  # the zones and, with ld, 7 gaps of ld - 40 elements
    assert pl.same_bits(around, torch.full_like(around, want))
    if dtype == torch.uint8:
        assert int(around[0]) == (0 if fill == "zero" else 0xFF)
    elif fill == "nan":
        assert bool(torch.isnan(around).all())


def test_place_zone_scales_with_the_row_pitch():
    buf, v = place(torch.zeros(2, 1024, dtype=torch.float16), align=16, fill="nan")
    assert v.data_ptr() - buf.data_ptr() >= 256 * 2048 > 64 * 1024


# ---- run_placed: the faithful kernel passes everything ----
def test_faithful_passes_all_fills():
    tally = [0, 0.0]
    r = run_placed(faithful, operands(ldx=K + 24), outputs(), check=check(REF), what="faithful", tally=tally)
    assert r["runs"] == 3 and tally[0] == 3 and 0 <= r["worst"] <= 1
    r = run_placed(ws_written_first, operands(), outputs(), {"split": M * N * 4}, check=check(REF), what="faithful ws")
    assert r["runs"] == 4  # the three fills and the 0xFF workspace prefill
    assert float((r["outputs"]["y"].double() - REF).abs().max()) <= 1e-5  # the zero-fill outputs come back
    r = run_placed(lambda i, o, ws: faithful(i, o, ws), operands(), outputs(), {"none": 0}, check=check(REF), what="empty ws")
    assert r["runs"] == 3  # a 0-byte workspace has no contents: no prefill run, no inflated count
    outs = dict(outputs(), colsum=Out((N,), torch.float32))
    run_placed(res_row_m_faithful, operands(), outs, check=check(REF), what="faithful colsum")


# ---- run_placed: each leak is reported by the check that exists for it ----
def test_k_tail_on_x_only_needs_the_nan_fill():
    run_placed(k_tail_on_x_only, operands(), outputs(), check=check(REF), what="zero only", fills=("zero",))
    run_placed(k_tail_on_x_only, operands(), outputs(), check=check(REF), what="finite garbage", fills=("zero", 3.0))
    with pytest.raises(PlacementError, match=r"\(a\) bit identity.*nan fill.*\['x'\]"):
        run_placed(k_tail_on_x_only, operands(), outputs(), check=check(REF), what="k tail")


def test_k_tail_behind_relu_needs_the_inf_fill():
    run_placed(k_tail_behind_relu, operands(), outputs(), check=check(REF_RELU), what="no inf", fills=("zero", "nan"))
    with pytest.raises(PlacementError, match=r"\(a\) bit identity.*inf fill.*\['x'\]"):
        run_placed(k_tail_behind_relu, operands(), outputs(), check=check(REF_RELU), what="k tail relu")


def test_row_m_of_res():
    outs = dict(outputs(), colsum=Out((N,), torch.float32))
    run_placed(res_row_m, operands(), outs, check=check(REF), what="zero only", fills=("zero", -2.5))
    with pytest.raises(PlacementError, match=r"\(a\) bit identity.*\['colsum'\].*nan fill.*\['res'\]"):
        run_placed(res_row_m, operands(), outs, check=check(REF), what="res row M")


def test_columns_past_k_of_a_strided_x():
    """With a contiguous x only the last row's tail is poison; with a row pitch every row's is.  An unplaced x
    (the gap holding finite values) hides it altogether."""
    run_placed(k_tail_on_x_only, operands(ldx=K + 24), outputs(), check=check(REF), what="finite gap", fills=("zero", 1.0))
    with pytest.raises(PlacementError, match=r"\(a\) bit identity.*first at \(0, 0\).*\['x'\]"):
        run_placed(k_tail_on_x_only, operands(ldx=K + 24), outputs(), check=check(REF), what="strided x")


def test_workspace_assumed_zero():
    with pytest.raises(PlacementError, match=r"\(e\) workspace prefill.*\['split'\]"):
        run_placed(ws_assumed_zero, operands(), outputs(), {"split": M * N * 4}, check=check(REF), what="stale ws")


def test_workspace_overrun_by_4_bytes():
    with pytest.raises(PlacementError, match=r"\(e\) workspace guard.*240 bytes of workspace 'split'"):
        run_placed(ws_overrun, operands(), outputs(), {"split": M * N * 4}, check=check(REF), what="ws overrun")


def test_write_into_an_input():
    with pytest.raises(PlacementError, match=r"\(d\) inputs unchanged: input 'x' was written \(the operand itself\)"):
        run_placed(writes_input, operands(), outputs(), check=check(REF), what="input write")
    with pytest.raises(PlacementError, match=r"\(d\) inputs unchanged: input 'bias' was written \(its surroundings\)"):
        run_placed(writes_before_input, operands(), outputs(), check=check(REF), what="input surroundings write")


def test_store_outside_the_output():
    with pytest.raises(PlacementError, match=r"\(c\) output frame.*'y'"):
        run_placed(writes_past_output, operands(), outputs(), check=check(REF), what="output gap")


def test_bound_is_checked_on_the_zero_fill_run():
    with pytest.raises(PlacementError, match=r"\(b\) bound"):
        run_placed(faithful, operands(), outputs(), check=check(REF + 1e-3), what="wrong value")
    with pytest.raises(PlacementError, match=r"\(b\) bound"):  # an element never stored keeps the sentinel
        run_placed(lambda i, o, ws: o["y"][:M - 1].copy_(REF[:M - 1]), operands(), outputs(), check=check(REF), what="unstored row")
