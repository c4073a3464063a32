"""The ViT-B encoder variant without a GPU: schema, the oracle against the reference golden, the routes it takes, and
a negative control for the conv cases of tests/test_gpu_vitb.py.

ViT-B is embed 768, 12 heads, ``features=128``, ``out_channels=[96, 192, 384, 768]``; its motion modules run at
C = 384, 768, 128, 128 (head dims 48, 96, 16, 16).  The key list and the golden clip come from the reference itself
(tests/golden/make_vitb_golden.py: the reference's model at full depth on the synthetic weight recipe, with
``intermediate_layer_idx['vitb'] = [2, 5, 8, 11]`` set on the instance).
"""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import vda_amd
from vda_amd import _lib, ops
import fp16_bounds as fb
from helpers import GOLDEN, assert_elementwise, load_golden, recipe_state_dict, rel_l1, vda_oracle

NAME = "vitb_t4_70x98"


def test_vitb_schema_matches_reference_and_loads_strict():
    """from_config("vitb") has exactly the reference's keys and shapes, and the recipe loads with strict=True."""
    with open(os.path.join(GOLDEN, "state_dict_keys_vitb.json")) as f:
        want = [(k, tuple(s)) for k, s in json.load(f)]
    m = vda_amd.VideoDepthAnything.from_config("vitb", device="meta")
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert len(want) == 351 and sorted(got) == sorted(want)
    assert m.intermediate_layer_idx["vitb"] == [2, 5, 8, 11]
    assert len(m.pretrained.blocks) == 12 and m.features == 128 and list(m.out_channels) == [96, 192, 384, 768]
    res = m.load_state_dict(recipe_state_dict("vitb"), strict=True, assign=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert [tuple(v.shape) for v in m.state_dict().values()] == [s for _, s in got]


def test_vitb_oracle_matches_reference_golden():
    """vda_oracle's 'vitb' entry against the reference's own forward, at test_oracle.py's bar (rel-L1 <= 1e-5)."""
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    x, depth, tap_stats, meta = load_golden(NAME)
    assert meta["encoder"] == "vitb" and meta["taps"] == [2, 5, 8, 11] and not meta["skip_tmp_block"]
    sd = recipe_state_dict("vitb")
    d = vda_oracle.forward(sd, "vitb", x)
    assert d.shape == depth.shape
    err = rel_l1(d, depth)
    print(f"{NAME}: oracle vs reference rel-L1 {err:.3e}")
    assert err <= 1e-5
    feats = vda_oracle.encoder_taps({k: v.float() for k, v in sd.items()}, "vitb", x.flatten(0, 1))
    for f, (mu, sd_, am) in zip(feats, tap_stats):  # test_oracle_taps_match_reference_stats' comparison
        assert abs(float(f.mean()) - mu) <= 1e-4 * max(1.0, abs(mu))
        assert abs(float(f.std()) - sd_) <= 1e-4 * sd_
        assert abs(float(f.abs().mean()) - am) <= 1e-4 * am


def test_vitb_fold_decisions_at_full_size():
    """The glue's decisions for ViT-B at 32 x 518 x 518 (37 x 37 patches), on meta tensors: a later route change
    cannot silently move ViT-B off the kernels tests/test_gpu_vitb.py holds.

    * ``_tap_fold`` declined as a whole: the projects GEMMs are N = 96 / 192 / 384 / 768 and the row-drop epilogue
      needs N % 256 == 0; only the last would be served.
    * ``_head_fold`` / ``_oc1_fold`` declined (the sub-pixel conv is Cout = 256 only; features = 128).
    * ``_qkv_fold`` accepted for module 1 (C = 768: N = 2304, three 256-column statistics parts) and declined for
      modules 0 (C = 384: N = 1152) and 2, 3 (C = 128: N = 384), which take LayerNorm + the row-bias GEMM.
    * ``groupnorm_linear`` is the fused kernel at C = 128 and GroupNorm + GEMM at C = 384 / 768."""
    meta = torch.device("meta")
    m = vda_amd.VideoDepthAnything.from_config("vitb", device="meta")
    P = m._pack(meta, False)
    BT, ph, pw = 32, 37, 37
    ntok = ph * pw + 1
    assert P.C == 768 and [q.C for q in P.mm] == [384, 768, 128, 128]
    assert not m._tap_fold(P, BT, ntok)
    served = [ops.gemm_accepts(BT * ntok, N, 768, ln_fold=True, ln_parts=3, drop_period=ntok) for N in (96, 192, 384, 768)]
    assert served == [False, False, False, True]
    assert not m._head_fold(P, BT, ph, pw) and not m._oc1_fold(P, BT, ph, pw)
    sites = (ph * pw, 19 * 19, ph * pw, 4 * ph * pw)
    assert [m._qkv_fold(q, BT * S, S, BT) for q, S in zip(P.mm, sites)] == [[False, False], [True, True], [False, False],
                                                                           [False, False]]
    assert ops.gemm_accepts(BT * 361, 2304, 768, ln_fold=True, ln_parts=3, rowbias=True, rdiv=361, rmod=BT)
    assert not ops.gemm_accepts(BT * 1369, 1152, 384, ln_fold=True, ln_parts=2, rowbias=True, rdiv=1369, rmod=BT)
    assert not ops.gemm_accepts(BT * 1369, 384, 128, ln_fold=True, ln_parts=1, rowbias=True, rdiv=1369, rmod=BT)
    # what those modules run instead, and ff2 (N = 128, K = 512, in-place residual) at M = 43,808
    assert ops.gemm_accepts(BT * 1369, 1152, 384, bias=False, rowbias=True, rdiv=1369, rmod=BT)
    assert ops.gemm_accepts(BT * 1369, 128, 512, res=True)
    lib = _lib.lib()
    assert lib.vda_groupnorm_linear_fused(128, 32, 128) == 1
    assert lib.vda_groupnorm_linear_fused(384, 32, 384) == 0 and lib.vda_groupnorm_linear_fused(768, 32, 768) == 0
    assert m.features // 2 == 64  # the depth tail's width


# ---- negative control: the bound rejects the faults the Cin = 96 conv case is there to catch ---------------------
@pytest.fixture(scope="module")
def cin96():
    """ViT-B's layer1_rn shape of tests/test_gpu_vitb.py (96 -> 128 at 1 x 91 x 91, rcu2; K = 864 in tiles of 64:
    tile 4 = k 256 .. 319 straddles taps 2 and 3, the last tile holds k 832 .. 863 only) with its staged bound."""
    c = fb.vitb_conv_case(1, 96, 91, 91, "rcu2")
    ref, bound = fb.conv_ref_bound(c["x"], c["w"], staged=True, **c["kw"])
    return c, ref, bound


def _conv64(c, w):
    kw = c["kw"]
    return F.conv2d(c["x"].double(), w, kw["bias"].double(), 1, 1) + kw["res"].double() + kw["res2"].double()


def test_cin96_reference_is_inside_its_own_bound(cin96):
    c, ref, bound = cin96
    assert assert_elementwise(_conv64(c, c["w"].double()), ref, bound, "float64 conv") < 1e-6
    assert assert_elementwise(fb.emulate_conv(c["x"], c["w"], staged=True, **c["kw"]), ref, bound, "emulation") <= 1.0


def test_cin96_transposed_tap_on_a_straddling_k_tile_is_outside_the_bound(cin96):
    """Tap 2 = (ky, kx) = (0, 2) read at (2, 0) for its last 32 channels (k = 256 .. 287, the part of tap 2 in the
    K tile it shares with tap 3): what a wrong k / Cin decode on that tile gives."""
    c, ref, bound = cin96
    w = c["w"].double().clone()
    w[:, 64:, 2, 0] += w[:, 64:, 0, 2]
    w[:, 64:, 0, 2] = 0
    with pytest.raises(AssertionError, match="outside the bound"):
        assert_elementwise(_conv64(c, w), ref, bound, "transposed tap")


def test_cin96_dropped_k_tail_is_outside_the_bound(cin96):
    """k >= 832 left out: tap 8 = (2, 2), channels 64 .. 95, the half-filled last K tile."""
    c, ref, bound = cin96
    w = c["w"].double().clone()
    w[:, 64:, 2, 2] = 0
    with pytest.raises(AssertionError, match="outside the bound"):
        assert_elementwise(_conv64(c, w), ref, bound, "K tail dropped")
