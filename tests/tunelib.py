"""The tuning build of libvda (make tune -> build/tune/libvda.so, include/vda_tune.h) for the tests that
compare an alternative kernel route with the product library's automatic one.

The product libvda.so has no route knobs (no mutable global state): the tests call the product through
vda_amd.ops, and the alternative route through this second copy of the kernels, loaded side by side
(both libraries are linked -Bsymbolic) and called straight through the C ABI on torch-allocated buffers.
"""
import contextlib
import ctypes
import os

import pytest
import torch

from vda_amd import _lib

_TUNE = None


def tune_lib():
    global _TUNE
    if _TUNE is None:
        if not os.path.exists(_lib.TUNE_LIB_PATH):
            pytest.fail(f"{_lib.TUNE_LIB_PATH} not built: run `make tune` (or __graft_entry__.build())")
        _TUNE = TuneLib(_lib.TUNE_LIB_PATH)
    return _TUNE


def _attn_scale(D):
    """1 / sqrt(D) formed in fp32 as the torch op does (csrc/vda_torch.cpp): the float64 D ** -0.5 rounded to
    fp32 can differ from it by one ulp (D = 24), and with it the last bit of some outputs."""
    one = torch.ones((), dtype=torch.float32)
    return float(one / torch.sqrt(torch.tensor(float(D), dtype=torch.float32)))


class TuneLib:
    DEFAULTS = dict(force_tile=-1, strip_split=0, hconv=-1, dconv=-1, attn=0, gemm_sched=-1)

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        _lib._declare(self.lib)
        assert self.lib.vda_epilogue_size() == ctypes.sizeof(_lib.Epilogue)

    def set(self, **knobs):
        for k, v in knobs.items():
            assert getattr(self.lib, "vda_debug_" + k)(v) == 0

    @contextlib.contextmanager
    def route(self, **knobs):
        """Run the block with the given knobs (vda_debug_<name>), restoring the automatic routes after."""
        self.set(**knobs)
        try:
            yield self
        finally:
            self.set(**{k: self.DEFAULTS[k] for k in knobs})

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: {self.lib.vda_last_error().decode()}")

    def conv2d(self, x, w, *, ks=3, stride=1, pad=1, bias=None, pre_relu=False, act=0, res=None, res2=None, up=None,
               rowbias=None, rdiv=1, rmod=1, out=None, res2_up=False):
        """vda_conv2d on NHWC fp16 x [BT, H, W, Cin], w [Cout, ks, ks, Cin] (the ops.conv2d contract).
        `up=(Hu, Wu)` reads x through the bilinear resize; `out` is a contiguous [BT, Ho, Wo, Cout] fp16 tensor
        to write into (e.g. a view inside a sentinel-filled buffer), else a fresh one; res2_up reads res2 through
        the epilogue's upsample even when it already has the output's size."""
        BT, H, W, Cin = x.shape
        Cout = w.shape[0]
        Hi, Wi = (H, W) if up is None else up
        Ho, Wo = (Hi + 2 * pad - ks) // stride + 1, (Wi + 2 * pad - ks) // stride + 1
        if out is None:
            y = torch.empty(BT, Ho, Wo, Cout, dtype=torch.float16, device=x.device)
        else:
            assert tuple(out.shape) == (BT, Ho, Wo, Cout) and out.dtype == torch.float16 and out.is_contiguous()
            y = out
        e = _lib.Epilogue(rdiv=rdiv, rmod=rmod, act=act)
        if bias is not None:
            e.bias = bias.data_ptr()
        if rowbias is not None:
            e.rowbias = rowbias.data_ptr()
        if res is not None:
            e.res, e.ldres = res.data_ptr(), Cout
        if res2 is not None:
            e.res2, e.ldres2 = res2.data_ptr(), Cout
            if res2_up or tuple(res2.shape[1:3]) != (Ho, Wo):  # read through the upsample in the epilogue
                e.res2_h, e.res2_w = res2.shape[1], res2.shape[2]
        wsb = self.lib.vda_conv2d_workspace(BT, H, W, Cin, Cout, ks, stride, pad)
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=x.device)
        st = torch.cuda.current_stream().cuda_stream
        uh, uw = (0, 0) if up is None else up
        self._check(self.lib.vda_conv2d(x.data_ptr(), w.data_ptr(), y.data_ptr(), BT, H, W, Cin, Cout, ks, stride, pad,
                                        int(pre_relu), uh, uw, ctypes.byref(e), ws.data_ptr() if wsb > 0 else None, wsb,
                                        st), "vda_conv2d")
        return y

    def depth_head_workspace(self, BT, H, W, C, Ho, Wo):
        return self.lib.vda_depth_head_workspace(BT, H, W, C, Ho, Wo)

    def depth_head(self, x, w1_split, b1, w2, b2, Ho, Wo):
        """vda_depth_head on NHWC fp16 x [BT, H, W, C] (the ops.depth_head contract)."""
        BT, H, W, C = x.shape
        d = torch.empty(BT, Ho, Wo, dtype=torch.float32, device=x.device)
        wsb = self.depth_head_workspace(BT, H, W, C, Ho, Wo)
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=x.device)
        st = torch.cuda.current_stream().cuda_stream
        self._check(self.lib.vda_depth_head(x.data_ptr(), w1_split.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                                            d.data_ptr(), ws.data_ptr() if wsb > 0 else None, BT, H, W, C, Ho, Wo, st),
                    "vda_depth_head")
        return d

    def gemm(self, x, w, y, e, M, N, K, ldy=None):
        st = torch.cuda.current_stream().cuda_stream
        self._check(self.lib.vda_gemm(x.data_ptr(), x.stride(0), w.data_ptr(), y.data_ptr(),
                                      y.stride(0) if ldy is None else ldy, M, N, K, ctypes.byref(e), st), "vda_gemm")
        return y

    def gemm_kw(self, x, w, out, *, bias=None, rowbias=None, rdiv=1, rmod=1, gamma=None, res=None, res2=None, act=0,
                ps=None, ln_stats=None, ln_colsum=None, ln_parts=0, ln_eps=1e-6, stats_out=None, drop_period=0,
                sched=None):
        """vda_gemm with the epilogue given by keyword (the ops.gemm names) into `out`, any row-strided 2-D fp16
        view (or, with ps=(k, cout, hin, win), the contiguous pixel-shuffled NHWC output).  x [M, K] and res /
        res2 may be row-strided views; the tensors must stay alive until the stream has run the launch."""
        M, K = x.shape
        N = w.shape[0]
        e = _lib.Epilogue(rdiv=rdiv, rmod=rmod, act=act, ln_parts=ln_parts, ln_eps=ln_eps, drop_period=drop_period)
        for name, t in (("bias", bias), ("rowbias", rowbias), ("gamma", gamma), ("ln_stats", ln_stats),
                        ("ln_colsum", ln_colsum), ("stats_out", stats_out), ("sched", sched)):
            if t is not None:
                setattr(e, name, t.data_ptr())
        if res is not None:
            e.res, e.ldres = res.data_ptr(), res.stride(0)
        if res2 is not None:
            e.res2, e.ldres2 = res2.data_ptr(), res2.stride(0)
        if ps is not None:
            e.store, e.ps_k, e.ps_cout, e.ps_hin, e.ps_win = 1, *ps
        return self.gemm(x, w, out, e, M, N, K, ldy=N if ps is not None else None)

    def spatial_attention(self, qkv, B, N, H, D=64, out=None):
        """`out`: a contiguous [B * N, H * D] fp16 tensor to write into (else a fresh one)."""
        if out is None:
            out = torch.empty(B * N, H * D, dtype=torch.float16, device=qkv.device)
        assert tuple(out.shape) == (B * N, H * D) and out.dtype == torch.float16 and out.is_contiguous()
        st = torch.cuda.current_stream().cuda_stream
        self._check(self.lib.vda_spatial_attention(qkv.data_ptr(), out.data_ptr(), B, N, H, D, _attn_scale(D), st),
                    "vda_spatial_attention")
        return out

    def temporal_attention(self, qkv, B, T, S, H, D, rope_theta=0.0, out=None):
        if out is None:
            out = torch.empty(B * T * S, H * D, dtype=torch.float16, device=qkv.device)
        assert tuple(out.shape) == (B * T * S, H * D) and out.dtype == torch.float16 and out.is_contiguous()
        st = torch.cuda.current_stream().cuda_stream
        self._check(self.lib.vda_temporal_attention(qkv.data_ptr(), out.data_ptr(), B, T, S, H, D, _attn_scale(D),
                                                    rope_theta, st), "vda_temporal_attention")
        return out
