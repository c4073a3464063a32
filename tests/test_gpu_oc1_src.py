"""output_conv1 with the channel mixing at the source resolution of its fused x2 resize (csrc/vda_oc1_src.hip), on
the GPU, driven through the tuning library: vda_debug_oc1_src(2) takes the new kernel wherever it serves, (0) the halo
conv with the fused resize (the parent route) for every shape, (1) is the product's automatic choice: the new kernel
for a bias9 call, the parent route (and the bits of resize + conv) for a plain bias.

Reference of the accuracy cases: the float64 chain ``conv2d 1x1 -> interpolate(scale 2, align_corners) -> conv2d 3x3``
(head_linear_ref.Case3).  Bar: stagelib's, ``FACTOR`` x the distance of the every-op-fp16-rounded chain from that
reference, per slice and for the largest element: the bar test_gpu_head_linear.py holds the parent route to.  Both
routes are held to it and printed side by side.  The new kernel stores z_t = W_t x as fp16 in LDS (one more
rounding per tap than the parent); the figures printed here are that choice's margin.

A case also asserts that the two routes do NOT return the same bits where the new kernel serves (it is the same
linear map in another order of operations), and the same bits where it does not serve: that is how the test knows
which kernel ran.
"""
import ctypes

import pytest
import torch

import stagelib as SL
import vda_amd
from head_linear_ref import MAPS3, Case3, class_map
from helpers import load_golden, recipe_state_dict, rel_l1
from tunelib import tune_lib
from vda_amd import _lib, ops, weights

pytestmark = pytest.mark.gpu

# MAPS3; tiles cross in both directions and a footprint straddles a tile edge; the one-row resize; an output of
# exactly 3 x 1 whole tiles
SHAPES = MAPS3 + [(1, 17, 9), (2, 1, 2), (1, 24, 8)]


SENT, GUARD = -7776.0, 1024  # the sentinel (exact in fp16) and its count before and after every output


def conv_up(route: int, x, w, up, bias=None, bias9=None):
    """vda_conv2d (3x3 / s1 / p1) of NHWC fp16 x through the resize to `up` (None: no resize), tuning library with
    vda_debug_oc1_src(route), into an output between sentinel guards that must be intact afterwards."""
    T = tune_lib()
    BT, H, W, Cin = x.shape
    Cout = w.shape[0]
    Ho, Wo = (H, W) if up is None else up
    n = BT * Ho * Wo * Cout
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.float16, device=x.device)
    y = buf[GUARD:GUARD + n].view(BT, Ho, Wo, Cout)
    e = _lib.Epilogue(rdiv=1, rmod=1)
    if bias is not None:
        e.bias = bias.data_ptr()
    if bias9 is not None:
        e.bias9 = bias9.data_ptr()
    uh, uw = (0, 0) if up is None else up
    assert T.lib.vda_debug_oc1_src(route) == 0
    try:
        rc = T.lib.vda_conv2d(x.data_ptr(), w.data_ptr(), y.data_ptr(), BT, H, W, Cin, Cout, 3, 1, 1, 0, uh, uw,
                              ctypes.byref(e), None, 0, torch.cuda.current_stream().cuda_stream)
    finally:
        assert T.lib.vda_debug_oc1_src(1) == 0
    assert rc == 0, T.lib.vda_last_error().decode()
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all()), "a store outside the output"
    return y


def _composed(c: Case3):
    wq, b9 = weights.compose_pointwise_conv3(c.w0, c.b0, c.w1, c.b1)
    return wq.cuda(), b9.cuda()


def _both(c: Case3, kind: str, x=None, wq=None, b9=None):
    """(new route, parent route) on the case: 'bias9' = the composed conv on x, 'bias' = out_conv as a GEMM, then
    output_conv1 with its plain bias."""
    x = c.x if x is None else x
    up = (2 * c.h, 2 * c.w)
    if kind == "bias9":
        if wq is None:
            wq, b9 = _composed(c)
        xin = SL.map_to_nhwc(x)
        return tuple(conv_up(r, xin, wq, up, bias9=b9) for r in (2, 0))
    y = ops.gemm(SL.map_to_rows(x), c.w0.reshape(256, 256).half().contiguous().cuda(), bias=c.b0.float().cuda())
    y = y.view(c.BT, c.h, c.w, 256)
    w1 = c.w1.permute(0, 2, 3, 1).half().contiguous().cuda()
    return tuple(conv_up(r, y, w1, up, bias=c.b1.float().cuda()) for r in (2, 0))


@pytest.mark.parametrize("kind", ["bias9", "bias"])
@pytest.mark.parametrize("BT,h,w", SHAPES)
def test_source_route_meets_the_bar_the_parent_route_meets(BT, h, w, kind):
    c = Case3(BT, h, w)
    r = c.ref()
    bars = SL.Bars(c.o16(), r)
    new, par = _both(c, kind)
    assert not torch.equal(new, par), "the two routes returned the same bits: the new kernel did not run"
    res = {n: SL.evaluate(SL.map_from_nhwc(y), r, bars.E, bars.max) for n, y in (("new", new), ("parent", par))}
    print(f"oc1_src {kind} {BT}x{h}x{w}: worst E / bar new {res['new'][0]:.3f} at [{res['new'][1]}], parent "
          f"{res['parent'][0]:.3f} at [{res['parent'][1]}]; max|y - r| / bar new {res['new'][2]:.3f}, parent "
          f"{res['parent'][2]:.3f} (bars {SL.FACTOR:g} x O16: E {bars.E:.3e}, max {bars.max:.3e})")
    assert not res["parent"][3], res["parent"][3]
    assert not res["new"][3], res["new"][3]


@pytest.mark.parametrize("BT,h,w", SHAPES)
def test_source_route_border_ring_and_frame_isolation(BT, h, w):
    """Weights zero: the output is the bias9 class map bit for bit.  A zero frame beside a large one: exactly its
    bias map."""
    c = Case3(BT, h, w)
    wq, b9 = _composed(c)
    assert len({tuple(r.tolist()) for r in b9[:, :4].cpu()}) == 9
    want = b9.cpu()[class_map(2 * h, 2 * w)].half()
    y = conv_up(2, SL.map_to_nhwc(c.x), torch.zeros_like(wq), (2 * h, 2 * w), bias9=b9)
    assert torch.equal(y.cpu(), want[None].expand(BT, -1, -1, -1))
    c2 = Case3(2, h, w)
    x = c2.x.clone()
    x[0] *= 64
    x[1] = 0
    new, par = _both(c2, "bias9", x=x, wq=wq, b9=b9)
    assert not torch.equal(new[0], par[0])
    assert torch.equal(new[1].cpu(), want)
    assert float(new[0].float().abs().max()) > 10 * float(b9.abs().max())


@pytest.mark.parametrize("BT,h,w", [(1, 9, 11), (1, 17, 9)])
def test_source_route_border_impulses(BT, h, w):
    """One non-zero source pixel at each corner, on each edge, in the interior and beside a tile edge: the whole
    output against the float64 chain and against the parent route, under the stage bar of that input.  Pins the
    tap mask and the clamped footprint at every border class."""
    c = Case3(BT, h, w)
    wq, b9 = _composed(c)
    x_full = c.x.clone()
    spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0),
             (h // 2, w - 1), (h // 2, w // 2), (min(7, h - 1), min(7, w - 1)), (min(8, h - 1), min(8, w - 1))]
    for py, px in spots:
        x = torch.zeros_like(x_full)
        x[:, :, py, px] = 8 * x_full[:, :, py, px]
        c.x = x
        r = c.ref()
        bars = SL.Bars(c.o16(), r)
        new, par = _both(c, "bias9", wq=wq, b9=b9)
        assert not torch.equal(new, par)
        vs_ref = SL.evaluate(SL.map_from_nhwc(new), r, bars.E, bars.max)
        vs_par = SL.evaluate(SL.map_from_nhwc(new), SL.map_from_nhwc(par), bars.E, bars.max)
        print(f"impulse ({py}, {px}) of {h}x{w}: new vs reference E / bar {vs_ref[0]:.3f}, max / bar {vs_ref[2]:.3f}; "
              f"new vs parent E / bar {vs_par[0]:.3f}, max / bar {vs_par[2]:.3f}")
        assert not vs_ref[3], vs_ref[3]
        assert not vs_par[3], vs_par[3]


def test_automatic_route_is_the_new_kernel_for_bias9_and_the_parent_for_a_plain_bias():
    """vda_debug_oc1_src(1), the product's constant: a bias9 call returns the new kernel's bits, a plain-bias call the
    parent's, which test_gpu_ops.py holds to the bits of resize + conv."""
    c = Case3(1, 9, 11)
    for kind in ("bias9", "bias"):
        new, par = _both(c, kind)
        up = (2 * c.h, 2 * c.w)
        if kind == "bias9":
            wq, b9 = _composed(c)
            auto = conv_up(1, SL.map_to_nhwc(c.x), wq, up, bias9=b9)
            assert torch.equal(auto, new) and not torch.equal(auto, par)
        else:
            y = ops.gemm(SL.map_to_rows(c.x), c.w0.reshape(256, 256).half().contiguous().cuda(), bias=c.b0.float().cuda())
            auto = conv_up(1, y.view(c.BT, c.h, c.w, 256), c.w1.permute(0, 2, 3, 1).half().contiguous().cuda(), up,
                           bias=c.b1.float().cuda())
            assert torch.equal(auto, par) and not torch.equal(auto, new)


@pytest.mark.parametrize("Cin,Cout,up", [(96, 128, (12, 10)), (256, 64, (12, 10)), (256, 128, (13, 10)),
                                         (256, 128, (12, 11)), (256, 128, None)])
def test_source_route_declines_and_the_parent_kernels_run(Cin, Cout, up):
    """Cin % 64 != 0, Cout != 128, a resize that is not exactly x2, no resize: the parent's kernels, the parent's
    bits."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 6, 5, Cin, generator=g).half().cuda()
    w = (torch.randn(Cout, 3, 3, Cin, generator=g) / (9 * Cin) ** 0.5).half().cuda()
    b = torch.randn(Cout, generator=g).cuda()
    new, par = (conv_up(r, x, w, up, bias=b) for r in (2, 0))
    assert torch.equal(new, par)
    assert float(new.float().abs().max()) > 0


def test_model_with_the_source_route_on_and_off_meets_the_golden_bar(monkeypatch):
    """ViT-L on the vitl_t4_70 golden clip with output_conv1 through the tuning library, route on and off: both
    rel-L1 to the reference's depth under the golden bar of test_gpu_model.py (1e-3), printed side by side."""
    x, depth, _, meta = load_golden("vitl_t4_70")
    m = vda_amd.build_model("vitl", recipe_state_dict("vitl"), device="cuda")
    xs = x.cuda()
    assert m._oc1_fold(m._pack(xs.device), 4, 5, 5)
    plain = ops.conv2d
    seen = []

    def routed(route):
        def conv2d(x, w, **kw):
            if kw.get("up") is not None and kw.get("bias9") is not None:
                seen.append(route)
                return conv_up(route, x, w, tuple(kw["up"]), bias9=kw["bias9"])
            return plain(x, w, **kw)
        return conv2d

    d = {}
    for route in (2, 0):
        monkeypatch.setattr(ops, "conv2d", routed(route))
        d[route] = m(xs, skip_tmp_block=meta["skip_tmp_block"]).float().cpu()
    monkeypatch.setattr(ops, "conv2d", plain)
    assert seen == [2, 0]
    e1, e0 = rel_l1(d[2], depth), rel_l1(d[0], depth)
    print(f"vitl_t4_70: rel-L1 vs reference source route {e1:.3e}, parent route {e0:.3e}; one vs the other "
          f"{rel_l1(d[2], d[0]):.3e}")
    assert torch.isfinite(d[2]).all() and torch.isfinite(d[0]).all()
    assert not torch.equal(d[2], d[0])
    assert e0 <= 1e-3
    assert e1 <= 1e-3
