"""The ViT-g encoder variant without a GPU: schema, SwiGLU packing, the SwiGLU bound's CPU proof, C-ABI checks.

ViT-g is DINOv2 ``vit_giant2`` with ``ffn_layer="swiglufused"`` (dinov2.py:381-415, dinov2_layers/swiglu_ffn.py): per
block ``mlp.w12`` [8192, 1536] and ``mlp.w3`` [1536, 4096] instead of fc1 / fc2.  The key list comes from the
reference itself (tests/golden/make_vitg_golden.py); the SwiGLU GEMM's bound and emulation are tests/swiglu_bounds.py.
"""
import ctypes
import json
import os

import pytest
import torch
import torch.nn.functional as F

import vda_amd  # noqa: F401
from vda_amd import _lib, ops
from vda_amd import model as vm
from vda_amd.weights import synthetic_state_dict
import swiglu_bounds as sb
from helpers import assert_elementwise

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
D4 = dict(embed_dim=1536, depth=4, heads=24, taps=[0, 1, 2, 3], ffn="swiglu")


def test_vitg_schema_matches_reference():
    """from_config("vitg") has exactly the reference's 743 keys and shapes (KeyError before the variant existed)."""
    want = [(k, tuple(s)) for k, s in json.load(open(os.path.join(GOLDEN, "state_dict_keys_vitg.json")))]
    m = vm.VideoDepthAnything.from_config("vitg", device="meta")
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert len(want) == 743
    assert sorted(got) == sorted(want)
    assert m.intermediate_layer_idx["vitg"] == [9, 19, 29, 39]
    blk = m.pretrained.blocks[0]
    assert tuple(blk.mlp.w12.weight.shape) == (8192, 1536) and tuple(blk.mlp.w3.weight.shape) == (1536, 4096)
    assert vm.ENCODER_CFG["vitl"].get("ffn", "mlp") == "mlp" and hasattr(m.pretrained, "blocks")


def test_vitg_d4_state_dict_round_trip(monkeypatch):
    """A reduced-depth entry registered in ENCODER_CFG is what the module tree builds; strict load round-trips."""
    monkeypatch.setitem(vm.ENCODER_CFG, "vitg", D4)
    m = vm.VideoDepthAnything.from_config("vitg", device="meta")
    keys = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert len(m.pretrained.blocks) == 4 and m.intermediate_layer_idx["vitg"] == [0, 1, 2, 3]
    small = [(k, s) for k, s in keys if ".blocks." not in k or ".blocks.0." in k]  # one block's worth is loaded for real
    sd = synthetic_state_dict(small)
    full = {k: sd[k] if k in sd else torch.empty(s, device="meta") for k, s in keys}
    res = m.load_state_dict(full, strict=True, assign=True)
    assert not res.missing_keys and not res.unexpected_keys
    back = m.state_dict()
    assert list(back) == [k for k, _ in keys]
    assert torch.equal(back["pretrained.blocks.0.mlp.w12.weight"], sd["pretrained.blocks.0.mlp.w12.weight"])


@torch.no_grad()
def test_swiglu_pack_is_the_reference_ffn_in_float64():
    """silu(x1) * x2 formed from the interleaved, LN-folded w12 pack equals SwiGLUFFNFused's gate on LayerNorm(x) in
    float64 to 1e-12 relative, on two random blocks (dim 64: hidden (int(256 * 2 / 3) + 7) // 8 * 8 = 176)."""
    torch.manual_seed(5)
    for seed in (0, 1):
        blk = vm.Block(64, 2, "swiglu").double()
        g = torch.Generator().manual_seed(seed)
        for p in blk.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * (0.3 if p.dim() > 1 else 1.0))
        I = blk.mlp.w3.weight.shape[1]
        assert I == 176 and blk.mlp.w12.weight.shape[0] == 2 * I
        x = torch.randn(37, 64, generator=g, dtype=torch.float64) * 2 + 0.5
        # the reference (swiglu_ffn.py:34-37 on block.py:87's norm2)
        x12 = F.linear(F.layer_norm(x, (64,), blk.norm2.weight, blk.norm2.bias, 1e-6), blk.mlp.w12.weight, blk.mlp.w12.bias)
        x1, x2 = x12.chunk(2, dim=-1)
        want = F.silu(x1) * x2
        # the pack, evaluated as the kernel does: rstd (x W'^T - mean colsum) + b', 16-row [h | g] blocks
        w, c1, b = vm._pack_ffn_in(blk, torch.float64, True)
        mean, rstd = x.mean(1, keepdim=True), (x.var(1, unbiased=False, keepdim=True) + 1e-6) ** -0.5
        pre = rstd * (x @ w.t() - mean * c1[None, :]) + b
        blocks = pre.view(37, I // 16, 2, 16)
        hv, gv = blocks[:, :, 0].reshape(37, I), blocks[:, :, 1].reshape(37, I)
        got = hv * (gv / (1 + torch.exp(-gv)))
        err = float((got - want).abs().max() / want.abs().max())
        print(f"SwiGLU pack block {seed}: max error / max |ref| = {err:.2e}")
        assert err < 1e-12
        # unfolded (fp32 mode's layout): the same rows, not normalised
        wu, cu, bu = vm._pack_ffn_in(blk, torch.float64, False)
        assert cu is None
        pu = (x @ wu.t() + bu.double()).view(37, I // 16, 2, 16)
        x12u = F.linear(x, blk.mlp.w12.weight, blk.mlp.w12.bias)
        assert float((pu[:, :, 1].reshape(37, I) - x12u[:, :I]).abs().max()) < 1e-6  # bias goes through fp32
        assert float((pu[:, :, 0].reshape(37, I) - x12u[:, I:]).abs().max()) < 1e-6


# ---- the SwiGLU bound: the faithful emulation inside, three mutants outside ---------------------------------
SHAPES = [(1, 32, 8), (127, 64, 24), (129, 160, 40), (257, 288, 160), (65, 128, 96)]


@pytest.mark.parametrize("staged", [False, True], ids=["tile", "phased"])
def test_swiglu_emulation_within_bound(staged):
    worst = 0.0
    for M, N, K in SHAPES:
        c = sb.swiglu_case(M, N, K, seed=M)
        ref, bound = sb.swiglu_ref_bound(c["x"], c["w"], staged=staged, **c["kw"])
        worst = max(worst, assert_elementwise(sb.emulate_swiglu(c["x"], c["w"], staged=staged, **c["kw"]), ref, bound,
                                              f"swiglu {M}x{N}x{K}"))
    for parts in (False, True):
        c = sb.swiglu_ln_case(257, 256, 192, seed=3, parts=parts)
        ref, bound = sb.swiglu_ref_bound(c["x"], c["w"], staged=staged, **c["kw"])
        worst = max(worst, assert_elementwise(sb.emulate_swiglu(c["x"], c["w"], staged=staged, **c["kw"]), ref, bound,
                                              f"swiglu LN fold parts={parts}"))
    print(f"swiglu staged={staged}: worst emulation |y - ref| / bound = {worst:.3f}")
    assert worst > 0.05  # the bound is within a small factor of what fp16 arithmetic really does


def test_swiglu_planted_gate_values_within_bound():
    """Gate pre-activations at +-30, +-100 and around exp's fp32 range: the kernel's form is finite and inside the
    bound; silu(-100) is -0 or a denormal, silu(100) is 100."""
    c = sb.planted_case(96, 64, 48, seed=2)
    ref, bound = sb.swiglu_ref_bound(c["x"], c["w"], **c["kw"])
    y = sb.emulate_swiglu(c["x"], c["w"], **c["kw"])
    assert bool(torch.isfinite(y).all())
    assert_elementwise(y, ref, bound, "swiglu planted")
    v = torch.tensor([-100.0, 100.0, -65504.0, 65504.0])
    s = sb.silu_kernel32(v)
    assert float(s[0]) == 0.0 and float(s[1]) == 100.0 and float(s[2]) == 0.0 and float(s[3]) == 65504.0


@pytest.mark.parametrize("mutant", ["swap", "gelu", "expform"])
def test_swiglu_mutants_leave_the_bound(mutant):
    """The gate on the wrong half, GELU in place of SiLU, and exp(v) / (1 + exp(v)) (NaN beyond v = 88.7: caught on
    the planted inputs, |v| up to 100; on ordinary inputs it is a correct SiLU and stays inside)."""
    if mutant == "expform":
        c = sb.planted_case(96, 64, 48, seed=2)
        ordinary = sb.swiglu_case(129, 160, 40, seed=1)
        ro, bo = sb.swiglu_ref_bound(ordinary["x"], ordinary["w"], **ordinary["kw"])
        assert_elementwise(sb.emulate_swiglu(ordinary["x"], ordinary["w"], mutant=mutant, **ordinary["kw"]), ro, bo,
                           "expform on ordinary inputs")
    else:
        c = sb.swiglu_case(129, 160, 40, seed=1)
    ref, bound = sb.swiglu_ref_bound(c["x"], c["w"], **c["kw"])
    y = sb.emulate_swiglu(c["x"], c["w"], mutant=mutant, **c["kw"])
    bad = ~((y.double() - ref).abs() <= bound)
    print(f"swiglu mutant {mutant}: {int(bad.sum())} of {bad.numel()} elements outside the bound")
    assert int(bad.sum()) > 0
    with pytest.raises(AssertionError):
        assert_elementwise(y, ref, bound, f"mutant {mutant}")


# ---- C ABI ---------------------------------------------------------------------------------------------
def _rejected(rc, msg):
    assert rc == -22
    err = _lib.lib().vda_last_error()
    assert msg in err, err


def test_swiglu_rejections_mirror_geglu():
    """Every argument rule of GEGLU holds for SwiGLU with the same message, on vda_gemm, vda_gemm_f32 and the convs."""
    lib = _lib.lib()
    fake = ctypes.c_void_p(0x1000)
    assert _lib.ACT_SWIGLU == 4 and ops.ACT_SWIGLU == 4
    E = lambda **kw: _lib.Epilogue(rdiv=1, rmod=1, **kw)  # noqa: E731
    ps = dict(store=_lib.STORE_PIXEL_SHUFFLE, ps_k=2, ps_cout=64, ps_hin=64, ps_win=64)
    for act in (_lib.ACT_GEGLU, _lib.ACT_SWIGLU):
        for gemm in (lib.vda_gemm, lib.vda_gemm_f32):
            _rejected(gemm(fake, 64, fake, fake, 128, 4096, 240, 64, E(act=act), None), b"N % 32")
            _rejected(gemm(fake, 64, fake, fake, 128, 4096, 256, 64, E(act=act, rowbias=0x2000), None),
                      b"no rowbias/res2, row store")
            _rejected(gemm(fake, 64, fake, fake, 128, 4096, 256, 64, E(act=act, res2=0x2000, ldres2=128), None),
                      b"no rowbias/res2, row store")
            _rejected(gemm(fake, 64, fake, fake, 256, 4096, 256, 64, E(act=act, **ps), None), b"no rowbias/res2, row store")
        _rejected(lib.vda_gemm(fake, 64, fake, fake, 128, 4096, 256, 64, E(act=act, stats_out=0x2000), None), b"stats_out")
        _rejected(lib.vda_gemm_f32(fake, 64, fake, fake, 128, 4096, 256, 64, E(act=act, stats_out=0x2000), None),
                  b"no row statistics")
        _rejected(lib.vda_conv2d_f32(fake, fake, fake, 2, 9, 11, 32, 64, 3, 1, 1, 0, E(act=act), None),
                  b"no GEGLU / pixel shuffle")
        ws = lib.vda_conv2d_workspace(2, 9, 11, 32, 64, 3, 1, 1)
        _rejected(lib.vda_conv2d(fake, fake, fake, 2, 9, 11, 32, 64, 3, 1, 1, 0, 0, 0, E(act=act), fake if ws else None, ws,
                                 None), b"activation none/relu")
    _rejected(lib.vda_gemm(fake, 64, fake, fake, 256, 4096, 256, 64, E(act=5), None), b"unknown activation")
    _rejected(lib.vda_gemm_f32(fake, 64, fake, fake, 256, 4096, 256, 64, E(act=5), None), b"unknown activation")


def test_gemm_check_accepts_the_model_w12_shape():
    """ViT-g's w12 GEMM at 32 x 518^2 (M 43,840, N 8,192, K 1,536) with norm2 folded in, [M, 2] statistics (C = 1536
    is six 256-column parts: more than ln_parts serves, so the encoder takes row_stats passes); and the streaming
    mode's one-frame M = 1,370 on the tile kernels."""
    for M in (43840, 1370, 300):
        assert ops.gemm_accepts(M, 8192, 1536, ln_fold=True, ln_parts=0, act=ops.ACT_SWIGLU)
        assert ops.gemm_accepts(M, 8192, 1536, act=ops.ACT_SWIGLU)
        assert ops.gemm_accepts(M, 1536, 4096, res=True)
    assert not ops.gemm_accepts(43840, 8192, 1536, ln_fold=True, ln_parts=6, act=ops.ACT_SWIGLU)
    assert not ops.gemm_accepts(43840, 8192, 1536, act=ops.ACT_SWIGLU, stats_out=True)


def test_temporal_attention_head_dim_contract():
    """D % 8 == 0, D <= 192 (fp32 entry point: even D <= 192); refused before any launch otherwise."""
    lib = _lib.lib()
    fake = ctypes.c_void_p(0x1000)
    _rejected(lib.vda_temporal_attention(fake, fake, 1, 4, 3, 8, 200, 0.07, 0.0, None), b"<= 192")
    _rejected(lib.vda_temporal_attention(fake, fake, 1, 4, 3, 8, 188, 0.07, 0.0, None), b"multiple of 8")
    _rejected(lib.vda_temporal_attention_f32(fake, fake, 1, 4, 3, 8, 194, 0.07, 0.0, None), b"even D <= 192")
    _rejected(lib.vda_temporal_attention_f32(fake, fake, 1, 4, 3, 8, 191, 0.07, 0.0, None), b"even D <= 192")
