"""The algebra of the source-resolution output_conv1 (csrc/vda_oc1_src.hip), restated in torch on the CPU.

``conv3x3(pad 1) . resize(x2, align_corners)`` is evaluated the kernel's way: z_t = W_t x at the source resolution
for each of the nine taps, and per 16 x 16 output tile the blend of z_t through the two staged slots of every ring
row / column (slot k >> 1 and the next, counted from source row y0 / 2 - 1), with the slot weights formed from the
resize's own (i0, i1, w) in fp32 and zero for a ring row / column outside the map.  Against the float64 chain
``F.interpolate -> F.conv2d`` the only difference is the fp32 weight arithmetic (<= 1e-6 relative), so the test pins
the slot pattern, the padding mask and the border handling at every size the GPU test uses, without a GPU.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

T = 16


def _coord(o, n_in, sc):
    """(i0, i1, w) of output coordinate o: csrc/vda_common.h ac_coord in fp32."""
    f = np.float32(sc) * np.float32(o)
    i0 = int(f)
    i1 = min(i0 + 1, n_in - 1)
    w = float(np.float32(np.float64(np.float32(sc)) * o - i0))  # the fma: exact product minus i0, rounded once
    return i0, i1, w


def _slot_weights(o, n_out, n_in, sc, g):
    if not 0 <= o < n_out:
        return 0.0, 0.0
    i0, i1, w = _coord(o, n_in, sc)
    u = 1.0 - w
    return (u if i0 == g else 0.0) + (w if i1 == g else 0.0), (u if i0 == g + 1 else 0.0) + (w if i1 == g + 1 else 0.0)


def emulate(x, w):
    """x [B, C, h, w] float64, w [Co, C, 3, 3] float64 -> [B, Co, 2h, 2w] by the kernel's route."""
    B, C, h, wd = x.shape
    H, W = 2 * h, 2 * wd
    scy = np.float32(h - 1) / np.float32(H - 1) if H > 1 else np.float32(0)
    scx = np.float32(wd - 1) / np.float32(W - 1) if W > 1 else np.float32(0)
    z = [F.conv2d(x, w[:, :, t // 3, t % 3][:, :, None, None]) for t in range(9)]  # z_t at h x w
    zp = [F.pad(t, (1, 10, 1, 10)) for t in z]  # source index s -> s + 1; zeros outside the map
    out = torch.zeros(B, w.shape[0], H, W, dtype=torch.float64)
    for y0 in range(0, H, T):
        for x0 in range(0, W, T):
            by, bx = y0 // 2 - 1, x0 // 2 - 1
            for i in range(min(T, H - y0)):
                for j in range(min(T, W - x0)):
                    acc = 0
                    for t in range(9):
                        ky, kx = i + t // 3, j + t % 3  # ring row / column
                        a, b = _slot_weights(y0 - 1 + ky, H, h, scy, by + (ky >> 1))
                        c, d = _slot_weights(x0 - 1 + kx, W, wd, scx, bx + (kx >> 1))
                        r, q = by + (ky >> 1) + 1, bx + (kx >> 1) + 1  # padded indices of the first slot
                        acc = acc + a * (c * zp[t][:, :, r, q] + d * zp[t][:, :, r, q + 1]) \
                            + b * (c * zp[t][:, :, r + 1, q] + d * zp[t][:, :, r + 1, q + 1])
                    out[:, :, y0 + i, x0 + j] = acc
    return out


@pytest.mark.parametrize("B,h,w", [(2, 6, 5), (1, 9, 11), (1, 17, 9), (2, 1, 2), (1, 24, 8), (1, 2, 1)])
def test_source_resolution_route_is_the_resize_then_conv(B, h, w):
    g = torch.Generator().manual_seed(100 * h + w)
    x = torch.randn(B, 8, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(4, 8, 3, 3, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True), wt, padding=1)
    got = emulate(x, wt)
    assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


@pytest.mark.parametrize("n", [1, 2, 3, 20, 148, 264, 1448])
def test_two_slots_cover_the_source_pair_of_every_coordinate(n):
    """The host check of the route (axis_ok): slot (o + 1) / 2 - 1 and the next hold i0 and i1 of every output
    coordinate, up to the few ulp of weight the last coordinate can leave on the row before."""
    sc = np.float32(n - 1) / np.float32(2 * n - 1) if n > 1 else np.float32(0)
    for o in range(2 * n):
        a, b = _slot_weights(o, 2 * n, n, sc, ((o + 1) >> 1) - 1)
        assert a + b > 1 - 1e-5, (n, o, a, b)
