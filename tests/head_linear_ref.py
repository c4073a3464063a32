"""ConvTranspose(k = s) -> conv3x3 chains for the composed sub-pixel conv tests (shared by test_head_linear.py and
test_gpu_head_linear.py; no tests here).

* ``Case``: one seeded chain: input [BT, Cin, h, w] rounded to fp16, unrounded fp32 weights, random biases of the
  weights' own scale (not the synthetic recipe's small ones).
* ``Case.ref``: the float64 chain ``conv_transpose2d -> conv2d(padding=1)`` on the fp16-rounded input with the
  unrounded weights.
* ``Case.o16(round_w)``: the same chain with every op's output stored as fp16 (``stagelib.r16``); with ``round_w``
  the weight matrices are rounded to fp16 first, which is what the unfused device path multiplies by.
* ``emulate``: the library's route (vda.h vda_subpixel_conv) restated in torch on the packed operands: corner
  matrix, one matmul per phase group on its K slice, class bias, corner -> output pixel store.
"""
import torch
import torch.nn.functional as F

from stagelib import r16
from vda_amd.weights import SUBPIXEL_GROUPS

# (s, Cin, Cmid, Cout): resize_layers[0] + layer1_rn and resize_layers[1] + layer2_rn of the ViT-L head
CHAINS = {4: (256, 256, 256), 2: (512, 512, 256)}
# (BT, h, w): a 256-row tile spans frames of 6 x 8 corners; top and bottom phases on one source row; several
# tiles with a frame that is no multiple of the tile
MAPS = [(3, 5, 7), (2, 1, 2), (1, 37, 37)]


class Case:
    def __init__(self, s: int, BT: int, h: int, w: int, seed: int = 0):
        Cin, Cmid, Cout = CHAINS[s]
        g = torch.Generator().manual_seed(1000 * s + 100 * BT + 10 * h + w + seed)
        self.s, self.BT, self.h, self.w = s, BT, h, w
        self.x = r16(torch.randn(BT, Cin, h, w, generator=g, dtype=torch.float64))
        self.wt = (torch.randn(Cin, Cmid, s, s, generator=g) / Cin ** 0.5)
        self.bt = 0.5 * torch.randn(Cmid, generator=g)
        self.wr = (torch.randn(Cout, Cmid, 3, 3, generator=g) / (9 * Cmid) ** 0.5)

    def chain(self, x, wt, bt, wr, store=lambda t: t):
        y = store(F.conv_transpose2d(x, wt, bt, stride=self.s))
        return store(F.conv2d(y, wr, padding=1))

    def ref(self):
        return self.chain(self.x, self.wt.double(), self.bt.double(), self.wr.double())

    def o16(self, round_w: bool = False):
        wt, wr = (r16(self.wt), r16(self.wr)) if round_w else (self.wt, self.wr)
        return self.chain(self.x, wt.double(), self.bt.double(), wr.double(), store=r16)


# (BT, h, w) of the out_conv . output_conv1 cases: -> 12 x 10; -> 18 x 22, past the 16 x 16 output tile on both axes
MAPS3 = [(2, 6, 5), (1, 9, 11)]


class Case3:
    """refinenet1.out_conv (1x1, 256 -> 256, bias) -> x2 bilinear align_corners resize -> output_conv1 (3x3,
    256 -> 128, bias): fp16-rounded input, unrounded fp32 weights, random biases of the activations' scale."""

    def __init__(self, BT: int, h: int, w: int, seed: int = 0, C: int = 256, Cout: int = 128):
        g = torch.Generator().manual_seed(7000 + 100 * BT + 10 * h + w + seed)
        self.BT, self.h, self.w = BT, h, w
        self.x = r16(torch.randn(BT, C, h, w, generator=g, dtype=torch.float64))
        self.w0 = torch.randn(C, C, 1, 1, generator=g) / C ** 0.5
        self.b0 = 0.5 * torch.randn(C, generator=g)
        self.w1 = torch.randn(Cout, C, 3, 3, generator=g) / (9 * C) ** 0.5
        self.b1 = 0.5 * torch.randn(Cout, generator=g)

    def chain(self, x, w0, w1, store=lambda t: t):
        y = store(F.conv2d(x, w0, self.b0.double()))
        y = store(F.interpolate(y, scale_factor=2, mode="bilinear", align_corners=True))
        return store(F.conv2d(y, w1, self.b1.double(), padding=1))

    def ref(self):
        return self.chain(self.x, self.w0.double(), self.w1.double())

    def o16(self, round_w: bool = False):
        w0, w1 = (r16(self.w0), r16(self.w1)) if round_w else (self.w0, self.w1)
        return self.chain(self.x, w0.double(), w1.double(), store=r16)

    def fused_model(self, wc: torch.Tensor, b9: torch.Tensor):
        """The device's composed path on the CPU: the fp16 resize of x, the composed fp16 weights wc [Cout, 3, 3,
        Cin], the class bias, one rounding."""
        u = r16(F.interpolate(self.x, scale_factor=2, mode="bilinear", align_corners=True))
        y = F.conv2d(u, wc.double().permute(0, 3, 1, 2), padding=1)
        return r16(y + b9.double()[class_map(2 * self.h, 2 * self.w)].permute(2, 0, 1)[None])


def class_map(H: int, W: int) -> torch.Tensor:
    """[H, W] long: 3 * (0 top / 1 middle / 2 bottom row) + (0 left / 1 middle / 2 right column)."""
    r = torch.ones(H, dtype=torch.long)
    r[0], r[-1] = 0, 2
    c = torch.ones(W, dtype=torch.long)
    c[0], c[-1] = 0, 2
    return 3 * r[:, None] + c[None, :]


def emulate(x: torch.Tensor, w_flat: torch.Tensor, bias9: torch.Tensor, s: int, Cout: int) -> torch.Tensor:
    """x [BT, Cin, h, w], packed (w_flat, bias9) -> [BT, Cout, s h, s w] float64, by the route of vda_subpixel_conv."""
    BT, Cin, h, w = x.shape
    p = x.double().permute(0, 2, 3, 1)  # NHWC
    pad = torch.zeros(BT, h + 2, w + 2, Cin, dtype=torch.float64)
    pad[:, 1:h + 1, 1:w + 1] = p
    # corner (ci, cj) block (r, c) = p[ci + r, cj + c] (zero outside the frame)
    order = ((-1, -1), (0, -1), (0, 0), (-1, 0))
    corner = torch.stack([pad[:, 1 + r:2 + r + h, 1 + c:2 + c + w] for r, c in order], 3)  # [BT, h+1, w+1, 4, Cin]
    corner = corner.reshape(BT, h + 1, w + 1, 4 * Cin)
    out = torch.full((BT, s * h, s * w, Cout), float("nan"), dtype=torch.float64)
    cls = class_map(s * h, s * w)
    b9 = bias9.double()
    off = 0
    wf = w_flat.double()
    for phases, window in SUBPIXEL_GROUPS[s]:
        koff = order.index(window[0]) * Cin
        K = len(window) * Cin
        assert tuple(order[order.index(window[0]):order.index(window[0]) + len(window)]) == tuple(window)
        wg = wf[off:off + 4 * Cout * K].view(4, Cout, K)
        off += 4 * Cout * K
        acc = corner[..., koff:koff + K] @ wg.permute(0, 2, 1)[:, None, None]  # [4, BT, h+1, w+1, Cout]
        for t, (a, b) in enumerate(phases):
            ea, eb = int(a == s - 1), int(b == s - 1)
            v = acc[t][:, ea:ea + h, eb:eb + w]  # corner (i + ea, j + eb) -> source pixel (i, j)
            out[:, a::s, b::s] = v + b9[cls[a::s, b::s]]
    assert off == wf.numel() and not bool(torch.isnan(out).any())
    return out.permute(0, 3, 1, 2)
