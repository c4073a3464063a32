"""ConvTranspose(k = s) + conv3x3 composed into one sub-pixel conv (vda.h vda_subpixel_conv), on the GPU.

Reference of every case: the float64 chain ``conv_transpose2d -> conv2d(padding=1)`` on the fp16-rounded input with
the unrounded weights (head_linear_ref.Case.ref).  Bar: stagelib's, ``FACTOR`` x the distance of the
every-op-fp16-rounded chain O16 from that reference, per slice (frame x ring class, frame x 64-channel block) and
for the largest element.  The unfused device path (conv_transpose_ks + conv2d) runs on the same inputs and is held
to the same bar; both error ratios are printed side by side.  test_head_linear.py checks on the CPU that the bars
admit a model of either path for these seeds.

The same for refinenet1's out_conv composed into output_conv1 (vda.h vda_epilogue.bias9): reference ``conv2d 1x1 ->
interpolate(scale 2, align_corners) -> conv2d 3x3`` in float64 (head_linear_ref.Case3), unfused path GEMM + conv.
Then the isolated checks (border ring = the class-bias map bit for bit, a zero frame beside a large one), the
routing (ViT-S widths and fp32 mode keep the old path bit for bit) and the ViT-L golden clip with the switch on / off.
"""
import pytest
import torch

import stagelib as SL
import vda_amd
from head_linear_ref import CHAINS, MAPS, MAPS3, Case, Case3, class_map
from helpers import load_golden, recipe_state_dict, rel_l1
from vda_amd import ops, weights

pytestmark = pytest.mark.gpu


def _rows(x):  # [BT, C, h, w] -> [BT*h*w, C] fp16 on the GPU
    return SL.map_to_rows(x)


SENT, GUARD = -7776.0, 1024  # the sentinel (exact in fp16) and its count before and after the output


def _fused(c: Case, wq=None, b9=None, x=None):
    """vda_subpixel_conv through the C ABI into an output between sentinel guards that must be intact afterwards,
    its workspace of exactly vda_subpixel_conv_workspace() bytes inside a guard of its own; ops.subpixel_conv (the
    product's call, which allocates both) must return the same bits."""
    if wq is None:
        wq, b9 = weights.compose_subpixel(c.wt, c.bt, c.wr, c.s)
    x = c.x if x is None else x
    L = vda_amd._libvda()
    Cin, _, Cout = CHAINS[c.s]
    xr, wd, bd = _rows(x), wq.cuda(), b9.cuda()
    n = c.BT * c.s * c.h * c.s * c.w * Cout
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.float16, device="cuda")
    y = buf[GUARD:GUARD + n].view(c.BT, c.s * c.h, c.s * c.w, Cout)
    wsb = int(L.vda_subpixel_conv_workspace(c.BT, c.h, c.w, Cin, c.s))
    wbuf = torch.full((wsb + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    rc = L.vda_subpixel_conv(xr.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), c.BT, c.h, c.w, Cin, Cout, c.s,
                             wbuf[GUARD:].data_ptr(), wsb, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.vda_last_error().decode()
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all()), "a store outside the output"
    assert bool((wbuf[:GUARD] == 0x5A).all()) and bool((wbuf[-GUARD:] == 0x5A).all()), "a store outside the workspace"
    assert torch.equal(y, ops.subpixel_conv(xr, wd, bd, c.BT, c.h, c.w, c.s))
    return y


def _unfused(c: Case):
    s = c.s
    w = c.wt.permute(2, 3, 1, 0).reshape(s * s * c.wt.shape[1], c.wt.shape[0]).half().contiguous().cuda()  # model._pack
    l = ops.conv_transpose_ks(_rows(c.x), w, c.bt.repeat(s * s).float().cuda(), c.BT, c.h, c.w, s)
    return ops.conv2d(l, c.wr.permute(0, 2, 3, 1).half().contiguous().cuda())


@pytest.mark.parametrize("s", [4, 2])
@pytest.mark.parametrize("BT,h,w", MAPS)
def test_composed_conv_meets_the_bar_the_unfused_path_meets(s, BT, h, w):
    c = Case(s, BT, h, w)
    assert ops.subpixel_conv_accepts(BT, h, w, CHAINS[s][0], CHAINS[s][2], s)
    r = c.ref()
    bars = SL.Bars(c.o16(), r)
    yf, yu = SL.map_from_nhwc(_fused(c)), SL.map_from_nhwc(_unfused(c))
    res = {}
    for name, y in (("fused", yf), ("unfused", yu)):
        res[name] = SL.evaluate(y, r, bars.E, bars.max)
    print(f"s={s} {BT}x{h}x{w}: worst E / bar fused {res['fused'][0]:.3f} at [{res['fused'][1]}], unfused "
          f"{res['unfused'][0]:.3f} at [{res['unfused'][1]}]; max|y - r| / bar fused {res['fused'][2]:.3f}, unfused "
          f"{res['unfused'][2]:.3f} (bars {SL.FACTOR:g} x O16: E {bars.E:.3e}, max {bars.max:.3e})")
    assert not res["unfused"][3], res["unfused"][3]
    assert not res["fused"][3], res["fused"][3]


@pytest.mark.parametrize("s", [4, 2])
@pytest.mark.parametrize("BT,h,w", [(3, 5, 7), (2, 1, 2)])
def test_border_ring_is_the_class_bias_map(s, BT, h, w):
    """Weights zero, biases non-zero: every output pixel is its class's row of the host table, bit for bit."""
    c = Case(s, BT, h, w)
    wq, b9 = weights.compose_subpixel(c.wt, c.bt, c.wr, s)
    assert len({tuple(r.tolist()) for r in b9[:, :4]}) == 9  # nine distinct classes
    y = _fused(c, torch.zeros_like(wq), b9)
    want = b9[class_map(s * h, s * w)].half()[None].expand(BT, -1, -1, -1)
    assert torch.equal(y.cpu(), want)


@pytest.mark.parametrize("s", [4, 2])
def test_frames_are_isolated(s):
    """Frame 0 large, frame 1 all zeros, 6 x 8 corners per frame (one 256-row tile holds both frames): frame 1
    is exactly its bias map, so no window read the neighbouring frame's rows."""
    c = Case(s, 2, 5, 7)
    x = c.x.clone()
    x[0] *= 64
    x[1] = 0
    wq, b9 = weights.compose_subpixel(c.wt, c.bt, c.wr, s)
    y = _fused(c, wq, b9, x=x)
    assert torch.equal(y[1].cpu(), b9[class_map(s * 5, s * 7)].half())
    assert float(y[0].float().abs().max()) > 10 * float(b9.abs().max())


def _fused3(c: Case3, wq=None, b9=None, x=None):
    if wq is None:
        wq, b9 = weights.compose_pointwise_conv3(c.w0, c.b0, c.w1, c.b1)
    x = c.x if x is None else x
    assert ops.conv2d_bias9_accepts(c.BT, c.h, c.w, 256, 128, (2 * c.h, 2 * c.w))
    return ops.conv2d(SL.map_to_nhwc(x), wq.cuda(), bias9=b9.cuda(), up=(2 * c.h, 2 * c.w))


def _unfused3(c: Case3):  # model._fusion's out_conv GEMM, then output_conv1 through the fused resize
    y = ops.gemm(SL.map_to_rows(c.x), c.w0.reshape(256, 256).half().contiguous().cuda(), bias=c.b0.float().cuda())
    return ops.conv2d(y.view(c.BT, c.h, c.w, 256), c.w1.permute(0, 2, 3, 1).half().contiguous().cuda(),
                      bias=c.b1.float().cuda(), up=(2 * c.h, 2 * c.w))


@pytest.mark.parametrize("BT,h,w", MAPS3)
def test_composed_out_conv_meets_the_bar_the_unfused_path_meets(BT, h, w):
    """out_conv (1x1) -> x2 bilinear -> output_conv1 (3x3) as one conv with a 9-class bias, against the float64
    chain ``conv2d 1x1 -> interpolate(scale 2, align_corners) -> conv2d 3x3``; same bar and side-by-side print."""
    c = Case3(BT, h, w)
    r = c.ref()
    bars = SL.Bars(c.o16(), r)
    res = {name: SL.evaluate(SL.map_from_nhwc(y), r, bars.E, bars.max)
           for name, y in (("fused", _fused3(c)), ("unfused", _unfused3(c)))}
    print(f"out_conv.oc1 {BT}x{h}x{w}: worst E / bar fused {res['fused'][0]:.3f} at [{res['fused'][1]}], unfused "
          f"{res['unfused'][0]:.3f} at [{res['unfused'][1]}]; max|y - r| / bar fused {res['fused'][2]:.3f}, unfused "
          f"{res['unfused'][2]:.3f} (bars {SL.FACTOR:g} x O16: E {bars.E:.3e}, max {bars.max:.3e})")
    assert not res["unfused"][3], res["unfused"][3]
    assert not res["fused"][3], res["fused"][3]


@pytest.mark.parametrize("BT,h,w", MAPS3)
def test_out_conv_border_ring_and_frame_isolation(BT, h, w):
    """Weights zero: the output is the bias9 class map bit for bit.  A zero frame beside a large one: exactly its
    bias map."""
    c = Case3(BT, h, w)
    wq, b9 = weights.compose_pointwise_conv3(c.w0, c.b0, c.w1, c.b1)
    assert len({tuple(r.tolist()) for r in b9[:, :4]}) == 9
    want = b9[class_map(2 * h, 2 * w)].half()
    y = _fused3(c, torch.zeros_like(wq), b9)
    assert torch.equal(y.cpu(), want[None].expand(BT, -1, -1, -1))
    c2 = Case3(2, h, w)
    x = c2.x.clone()
    x[0] *= 64
    x[1] = 0
    y = _fused3(c2, wq, b9, x=x)
    assert torch.equal(y[1].cpu(), want)
    assert float(y[0].float().abs().max()) > 10 * float(b9.abs().max())


def test_route_declines_and_model_takes_old_path_bit_for_bit():
    """The route check declines ViT-S widths; fp32 mode never asks.  The model's forward is then the
    ConvTranspose + conv3x3 path whatever the switch says: same bits with the switch on and off."""
    assert not ops.subpixel_conv_accepts(4, 5, 7, 48, 64, 4) and not ops.subpixel_conv_accepts(4, 5, 7, 96, 64, 2)
    g = torch.Generator().manual_seed(21)
    x = torch.randn(1, 4, 3, 70, 98, generator=g).cuda()
    m = vda_amd.build_model("vits", recipe_state_dict("vits"), device="cuda")
    assert not m._head_fold(m._pack(x.device), 4, 5, 7) and not m._oc1_fold(m._pack(x.device), 4, 5, 7)
    assert not ops.conv2d_bias9_accepts(4, 20, 28, 64, 32, (40, 56))
    d1 = m(x)
    m.fold_head_linear = False
    d0 = m(x)
    assert torch.equal(d0, d1)
    ml = _vitl()
    assert ml.fold_head_linear and not ml._head_fold(ml._pack(x.device, True), 4, 5, 7)
    assert not ml._oc1_fold(ml._pack(x.device, True), 4, 5, 7)
    assert ml._head_fold(ml._pack(x.device), 4, 5, 7) and ml._oc1_fold(ml._pack(x.device), 4, 5, 7)
    xs = x[:, :2, :, :28, :42].contiguous()
    f1 = ml(xs, fp32=True)
    ml.fold_head_linear = False
    try:
        f0 = ml(xs, fp32=True)
    finally:
        ml.fold_head_linear = True
    assert torch.equal(f0, f1)


_VITL = []


def _vitl():
    if not _VITL:
        _VITL.append(vda_amd.build_model("vitl", recipe_state_dict("vitl"), device="cuda"))
    return _VITL[0]


def test_model_folded_forward_meets_the_golden_bar():
    """ViT-L on the vitl_t4_70 golden clip: fold_head_linear on (the default) and off are both held to the golden
    bar of test_gpu_model.py (rel-L1 <= 1e-3 against the reference's depth); their mutual rel-L1 is printed."""
    x, depth, _, meta = load_golden("vitl_t4_70")
    m = _vitl()
    xs = x.cuda()
    assert m._head_fold(m._pack(xs.device), 4, 5, 5) and m._oc1_fold(m._pack(xs.device), 4, 5, 5)
    d1 = m(xs, skip_tmp_block=meta["skip_tmp_block"]).float().cpu()
    m.fold_head_linear = False
    try:
        d0 = m(xs, skip_tmp_block=meta["skip_tmp_block"]).float().cpu()
    finally:
        m.fold_head_linear = True
    e1, e0 = rel_l1(d1, depth), rel_l1(d0, depth)
    print(f"vitl_t4_70: rel-L1 vs reference folded {e1:.3e}, unfolded {e0:.3e}; folded vs unfolded {rel_l1(d1, d0):.3e}")
    assert torch.isfinite(d1).all() and e0 <= 1e-3
    assert e1 <= 1e-3
