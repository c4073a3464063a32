"""Shared test helpers: golden loading, the synthetic-recipe state_dict, the oracle import."""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
if REPO not in sys.path:
    sys.path.insert(0, REPO)
ORACLE_DIR = os.path.join(REPO, "oracle")
if ORACLE_DIR not in sys.path:
    sys.path.insert(0, ORACLE_DIR)

import vda_oracle  # noqa: E402  (test infrastructure only)
import vda_amd  # noqa: E402
from vda_amd.weights import synthetic_state_dict  # noqa: E402

GOLDEN_CASES = ["vits_t8_126", "vits_t8_126_skip", "vits_t4_70x126", "vits_t1_518", "vitl_t4_70",
                "vitl_t3_84x56_b2"]


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    return torch.from_numpy(z["x"].astype(np.float32)), torch.from_numpy(z["depth"]), z["tap_stats"], meta


_SD = {}


def recipe_state_dict(enc):
    if enc not in _SD:
        m = vda_amd.VideoDepthAnything.from_config(enc, device="meta")
        _SD[enc] = synthetic_state_dict((k, tuple(v.shape)) for k, v in m.state_dict().items())
    return _SD[enc]


def rel_l1(a, b):
    return vda_oracle.rel_l1(a, b)


def device_at_offset(a: np.ndarray, offset: int = 1, fill=None) -> torch.Tensor:
    """a on the GPU with its shape, starting ``offset`` elements past an allocation boundary (a multiple of 16
    bytes): one fp32 element past it is 4-byte aligned, not 16.  ``fill``: the value of the buffer's elements
    around a (unset otherwise)."""
    flat = torch.from_numpy(np.array(a).reshape(-1))  # a copy: shared references may be read-only
    buf = torch.empty(offset + flat.numel() + 16, dtype=flat.dtype, device="cuda")
    if fill is not None:
        buf.fill_(fill)
    v = buf[offset:offset + flat.numel()]
    v.copy_(flat)
    assert v.data_ptr() % 16 == offset * flat.element_size() % 16
    return v.view(a.shape)


def assert_elementwise(y, ref64, bound64, what):
    """Assert |y - ref| <= bound at EVERY element (y any dtype / device; ref64, bound64 float64 of y's
    shape, a bound from tests/fp16_bounds.py).  A non-finite y counts as a violation.  The failure message
    gives the number of violations, the worst ratio |y - ref| / bound and the worst element's index
    unravelled over y's shape ((frame, row, column, channel) for an NHWC map, (row, column) for a
    matrix), so a tile edge can be read off it.  Returns the worst ratio."""
    y64 = y.detach().to("cpu", torch.float64)
    ref64, bound64 = ref64.to(torch.float64), bound64.to(torch.float64)
    assert y64.shape == ref64.shape == bound64.shape, f"{what}: shapes {tuple(y64.shape)} {tuple(ref64.shape)} {tuple(bound64.shape)}"
    assert bool((bound64 > 0).all()) and bool(torch.isfinite(ref64).all()), f"{what}: bad reference / bound"
    ratio = (y64 - ref64).abs() / bound64
    ratio = torch.where(torch.isfinite(y64), ratio, torch.full_like(ratio, float("inf")))
    worst = float(ratio.max())
    if worst > 1.0:
        bad = ratio > 1.0
        idx = tuple(int(i) for i in np.unravel_index(int(ratio.argmax()), tuple(ratio.shape)))
        first = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {ratio.numel()} elements outside the bound; worst |y - ref| / bound = "
            f"{worst:.3g} at index {idx} of shape {tuple(ratio.shape)} (y {float(y64[idx]):.6g}, ref {float(ref64[idx]):.6g}, "
            f"bound {float(bound64[idx]):.3g}); first violation at {first}")
    return worst
