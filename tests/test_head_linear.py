"""ConvTranspose(k = s) + conv3x3 composed into one sub-pixel conv: the host side, on the CPU.

The algebra (vda.h vda_subpixel_conv) is exact in real arithmetic; here it is checked in float64 with biases on
non-square maps, through the packed operands the kernels take (weights.compose_subpixel) and a torch restatement
of the kernels' route (head_linear_ref.emulate).  The fp16 bars the GPU tests use come from the reference alone;
the seeds of those tests are checked here against them with a CPU model of both device paths.
"""
import pytest
import torch

import stagelib as SL
from head_linear_ref import CHAINS, MAPS, MAPS3, Case, Case3, class_map, emulate
from vda_amd import _lib, weights


@pytest.mark.parametrize("s", [2, 4])
def test_block_structure(s):
    """Phase 0 sees source rows {-1, 0}, phase s - 1 rows {0, +1}, the phases between row 0 only (columns
    alike): 16 blocks of 36 for s = 2, 36 of 144 for s = 4, each in exactly one phase group."""
    g = torch.Generator().manual_seed(s)
    wt, wr = torch.randn(16, 8, s, s, generator=g), torch.randn(8, 8, 3, 3, generator=g)
    blocks = weights.subpixel_blocks(wt, wr, s)
    span = lambda a: {0: (-1, 0), s - 1: (0, 1)}.get(a, (0,))  # noqa: E731
    assert set(blocks) == {(a, b, di, dj) for a in range(s) for b in range(s) for di in span(a) for dj in span(b)}
    assert len(blocks) == {2: 16, 4: 36}[s]
    grouped = [(a, b, r + (a == s - 1), c + (b == s - 1)) for ph, win in weights.SUBPIXEL_GROUPS[s]
               for a, b in ph for r, c in win]
    assert sorted(grouped) == sorted(blocks)
    w, b9 = weights.compose_subpixel(wt, torch.randn(8, generator=g), wr, s)
    assert w.dtype == torch.float16 and w.numel() == 4 * 8 * 16 * {2: 4, 4: 9}[s] and b9.shape == (9, 8)


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("BT,h,w", [(2, 3, 5), (2, 1, 2), (1, 1, 1)])
def test_composition_exact_in_float64(s, BT, h, w):
    """The packed composition through the kernels' route equals conv_transpose2d -> conv2d(padding=1) in float64,
    biases included, on a non-square map, on a one-row map and on a single pixel."""
    g = torch.Generator().manual_seed(10 * s + h)
    Cin, Cmid, Cout = 24, 16, 8
    x = torch.randn(BT, Cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(Cin, Cmid, s, s, generator=g, dtype=torch.float64)
    bt = torch.randn(Cmid, generator=g, dtype=torch.float64)
    wr = torch.randn(Cout, Cmid, 3, 3, generator=g, dtype=torch.float64)
    ref = torch.nn.functional.conv2d(torch.nn.functional.conv_transpose2d(x, wt, bt, stride=s), wr, padding=1)
    blocks = weights.subpixel_blocks(wt, wr, s)
    parts = []
    for phases, window in weights.SUBPIXEL_GROUPS[s]:  # compose_subpixel's packing, kept in float64
        parts.append(torch.cat([torch.cat([blocks[(a, b, r + (a == s - 1), c + (b == s - 1))] for r, c in window], 1)
                                for a, b in phases], 0).reshape(-1))
    y = emulate(x, torch.cat(parts), weights.subpixel_bias9(bt, wr), s, Cout)
    assert float((y - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_frame_isolation_and_bias_ring_on_the_cpu():
    """Zero input: the output is the class-bias map, whatever the neighbouring frame holds."""
    c = Case(4, 2, 2, 3)
    w, b9 = weights.compose_subpixel(c.wt, c.bt, c.wr, 4)
    x = c.x.clone()
    x[1] = 0
    x[0] *= 100
    y = emulate(x, w, b9, 4, 256)
    assert torch.equal(y[1].permute(1, 2, 0), b9.double()[class_map(8, 12)])


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("BT,h,w", MAPS)
def test_bars_admit_both_device_paths_for_the_gpu_seeds(s, BT, h, w):
    """The bar of the GPU tests is 4 x the distance of the every-op-fp16-rounded chain O16 from the float64
    chain, per slice (stagelib).  For the seeds those tests use, a CPU model of the unfused device path (O16 on
    fp16-rounded weights) and of the fused one (the route on compose_subpixel's operands, output rounded to
    fp16) both sit inside it."""
    c = Case(s, BT, h, w)
    r = c.ref()
    bars = SL.Bars(c.o16(), r)
    unfused = c.o16(round_w=True)
    wq, b9 = weights.compose_subpixel(c.wt, c.bt, c.wr, s)
    fused = SL.r16(emulate(c.x, wq, b9, s, CHAINS[s][2]))
    for name, y in (("unfused model", unfused), ("fused model", fused)):
        rE, where, rmax, lines = SL.evaluate(y, r, bars.E, bars.max)
        print(f"s={s} {BT}x{h}x{w} {name}: worst E / bar {rE:.3f} at [{where}], max / bar {rmax:.3f}")
        assert not lines, lines


@pytest.mark.parametrize("BT,h,w", MAPS3 + [(1, 1, 2)])
def test_out_conv_composition(BT, h, w):
    """out_conv -> x2 resize -> output_conv1 is one 3x3 conv with weights W_1[t] W_o on the resized input and the
    9-class bias b_1 + sum of in-bounds W_1[t] b_o: exact in float64; and for the GPU tests' seeds the bars (4 x
    O16's distance from the float64 chain) admit a CPU model of the unfused and of the composed device path."""
    c = Case3(BT, h, w)
    r = c.ref()
    w0, w1 = c.w0.double().reshape(256, 256), c.w1.double()
    wc64 = torch.einsum("omyx,mi->oiyx", w1, w0)
    b9 = weights.subpixel_bias9(c.b0, c.w1) + c.b1.double()[None]
    u = torch.nn.functional.interpolate(c.x, scale_factor=2, mode="bilinear", align_corners=True)
    y = torch.nn.functional.conv2d(u, wc64, padding=1) + b9[class_map(2 * h, 2 * w)].permute(2, 0, 1)[None]
    assert float((y - r).abs().max()) <= 1e-12 * float(r.abs().max())
    if (BT, h, w) not in MAPS3:
        return
    bars = SL.Bars(c.o16(), r)
    wq, b9q = weights.compose_pointwise_conv3(c.w0, c.b0, c.w1, c.b1)
    assert wq.shape == (128, 3, 3, 256) and b9q.shape == (9, 128)
    for name, m in (("unfused model", c.o16(round_w=True)), ("fused model", c.fused_model(wq, b9q))):
        rE, where, rmax, lines = SL.evaluate(m, r, bars.E, bars.max)
        print(f"out_conv.oc1 {BT}x{h}x{w} {name}: worst E / bar {rE:.3f} at [{where}], max / bar {rmax:.3f}")
        assert not lines, lines


def test_route_check():
    lib = _lib.lib()
    assert lib.vda_subpixel_conv_check(32, 37, 37, 256, 256, 4) == 0
    assert lib.vda_subpixel_conv_check(32, 37, 37, 512, 256, 2) == 0
    assert lib.vda_subpixel_conv_check(32, 37, 66, 512, 256, 2) == 0      # 518 x 924 input
    assert lib.vda_subpixel_conv_workspace(32, 37, 37, 256, 4) == 32 * 38 * 38 * 4 * 256 * 2
    assert lib.vda_subpixel_conv_check(1, 1, 2, 256, 256, 4) == 0
    assert lib.vda_subpixel_conv_check(32, 37, 37, 48, 64, 4) == -22       # ViT-S widths
    assert b"Cout == 256" in lib.vda_last_error()
    assert lib.vda_subpixel_conv_check(32, 37, 37, 96, 128, 4) == -22      # ViT-B
    assert lib.vda_subpixel_conv_check(32, 37, 37, 256, 256, 3) == -22
    assert lib.vda_subpixel_conv_check(400, 37, 37, 512, 256, 2) == -22    # the corner matrix passes 2 GiB
    assert b"2 GiB" in lib.vda_last_error()
    assert lib.vda_subpixel_conv_workspace(32, 37, 37, 48, 4) == 0
    fake = 0x1000
    assert lib.vda_subpixel_conv(fake, fake, fake, fake, 32, 37, 37, 256, 256, 4, fake, 1024, None) == -22
    assert b"workspace too small" in lib.vda_last_error()
    assert lib.vda_subpixel_conv(fake, fake, fake, 0x1008, 32, 37, 37, 256, 256, 4, fake, 1 << 31, None) == -22
    assert b"16-byte aligned" in lib.vda_last_error()
    # the 9-class bias table: output_conv1 through the fused x2 resize only
    assert lib.vda_conv2d_bias9_ok(32, 148, 148, 256, 128, 296, 296) == 1
    assert lib.vda_conv2d_bias9_ok(32, 148, 264, 256, 128, 296, 528) == 1
    assert lib.vda_conv2d_bias9_ok(32, 148, 148, 256, 128, 0, 0) == 0
    assert lib.vda_conv2d_bias9_ok(32, 148, 148, 64, 32, 296, 296) == 0     # ViT-S: 32 outputs
    e = _lib.Epilogue(rdiv=1, rmod=1, bias9=0x2000)
    assert lib.vda_gemm(fake, 64, fake, fake, 256, 4096, 256, 64, e, None) == -22
    assert b"bias9" in lib.vda_last_error()
    assert lib.vda_conv2d(fake, fake, fake, 32, 148, 148, 256, 128, 3, 1, 1, 0, 0, 0, e, None, 0, None) == -22
    assert b"bias9" in lib.vda_last_error()
    e = _lib.Epilogue(rdiv=1, rmod=1, bias9=0x2000, bias=0x3000)
    assert lib.vda_conv2d(fake, fake, fake, 32, 148, 148, 256, 128, 3, 1, 1, 0, 296, 296, e, None, 0, None) == -22
    assert lib.vda_conv2d_f32(fake, fake, fake, 2, 9, 11, 32, 64, 3, 1, 1, 0, _lib.Epilogue(rdiv=1, rmod=1, bias9=0x2000),
                              None) == -22


def test_model_fold_decision_on_meta():
    """forward composes the two chains for ViT-L in fp16 only; ViT-S / ViT-B widths, fp32 mode and the switch
    turned off keep ConvTranspose + conv3x3."""
    import vda_amd
    meta = torch.device("meta")

    def decide(enc, fp32=False, BT=32, ph=37, pw=37, **kw):
        m = vda_amd.VideoDepthAnything.from_config(enc, device="meta")
        for k, v in kw.items():
            setattr(m, k, v)
        P = m._pack(meta, fp32)
        return m._head_fold(P, BT, ph, pw), m._oc1_fold(P, BT, ph, pw)

    assert decide("vitl") == (True, True) and decide("vitl", pw=66) == (True, True)
    assert decide("vitl", BT=4, ph=5, pw=5)[0]
    assert decide("vitl", fp32=True) == (False, False)
    assert decide("vitl", fold_head_linear=False) == (False, False)
    assert decide("vits") == (False, False) and decide("vitb") == (False, False)
