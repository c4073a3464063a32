"""vda_cloud_count / vda_cloud_write on the GPU against ``TorchCloud`` on the CPU, bit for bit: points, colours,
frame_offsets and N in both layouts, at the smallest shapes where the compaction can go wrong (under a wave, rows
across wave ends, blocks that end mid-row with a ragged last one), keep patterns that leave waves and frames empty,
every operand placed in poison (tests/placement.py), outputs at odd byte addresses, a cap below N."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cloud_ref as R
import placement as P
import vda_amd  # noqa: F401
from vda_amd import _lib
from vda_amd import pointcloud as PC

pytestmark = pytest.mark.gpu

TRUNC = PC.depth_trunc(80.)
BYTE_SENT = 0xA5
LAYOUTS = {"split": _lib.CLOUD_SPLIT, "packed": _lib.CLOUD_PACKED}


def span():
    return int(_lib.lib().vda_cloud_span())


def big_shape():
    """F = 3 frames of 2 * span + 37 candidates, in as many rows as that number allows (blocks end mid-row)."""
    n = 2 * span() + 37
    h = max(d for d in range(1, 65) if n % d == 0)
    return 3, h, n // h


def cameras(F, H, W, seed=1):
    g = np.random.default_rng(seed)
    K = np.stack([g.uniform(300, 900, F), g.uniform(300, 900, F), g.uniform(0, W, F), g.uniform(0, H, F)], 1).astype(np.float32)
    M = np.zeros((F, 3, 4), dtype=np.float32)
    for f in range(F):
        q, _ = np.linalg.qr(g.normal(size=(3, 3)))
        M[f, :, :3], M[f, :, 3] = q, g.uniform(-20, 20, 3)
    return K, M


@functools.lru_cache(maxsize=None)
def clip(F, H, W, seed=0):
    """Good depths everywhere (patterns come from `valid`) and colours; read-only, shared between tests."""
    g = np.random.default_rng(seed)
    depth = g.uniform(0.5, 60., (F, H, W)).astype(np.float32)
    rgb = g.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    K, M = cameras(F, H, W)
    for a in (depth, rgb, K, M):
        a.setflags(write=False)
    return depth, rgb, K, M


def pattern(name, F, H, W):
    S = H * W
    idx = np.arange(F * S).reshape(F, S)
    v = np.zeros((F, S), dtype=np.uint8)
    if name == "all":
        v[:] = 1
    elif name == "none":
        pass
    elif name == "checker":
        ii, jj = np.divmod(np.arange(S), W)
        v[:] = ((ii + jj) % 2 == 0)[None]
    elif name == "first":
        v[F - 1, 0] = 1
    elif name == "last":
        v[0, S - 1] = 1
    elif name == "runs":  # 70 dropped, then 50 kept: whole waves come up empty
        v[:] = (idx % 120) >= 70
    elif name == "half":
        v[:] = np.random.default_rng(7).random((F, S)) < 0.5
    elif name == "empty_frame":
        v[:] = 1
        v[F // 2] = 0
    else:
        raise KeyError(name)
    return v.reshape(F, H, W)


PATTERNS = ["all", "none", "checker", "first", "last", "runs", "half", "empty_frame"]


def reference(depth, valid, rgb, K, M, step, trunc=TRUNC):
    t = lambda a: None if a is None else torch.from_numpy(np.array(a))  # noqa: E731
    offs, _ = PC.TorchCloud.count(t(depth), t(valid), step, trunc)
    n = int(offs[-1])
    pts, col = PC.TorchCloud.write(t(depth), t(valid), t(rgb), t(K), t(M), step, trunc, None, n, "split")
    return pts, col, offs, n


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def run_case(depth, valid, rgb, K, M, step, layout, *, out_align=4, cap=None, trunc=TRUNC, what=""):
    """count + write through the C ABI with every operand placed in poison (depth 4-byte but not 16-byte aligned),
    the workspace exact and guarded, the outputs framed in sentinels; the outputs are held to ``TorchCloud``'s bits.
    With `cap` the outputs still have room for all N records and everything from record `cap` on keeps its sentinel."""
    lib = _lib.lib()
    F, H, W = depth.shape
    pts, col, offs, n = reference(depth, valid, rgb, K, M, step, trunc)
    cap = n if cap is None else cap
    rec = 15 if rgb is not None else 12
    ops = dict(depth=P.In(torch.from_numpy(np.array(depth)), align=4), K=P.In(torch.from_numpy(np.array(K)), align=4))
    if valid is not None:
        ops["valid"] = P.In(torch.from_numpy(np.array(valid)), align=1)
    if rgb is not None:
        ops["rgb"] = P.In(torch.from_numpy(np.array(rgb)), align=3)
    if M is not None:
        ops["M"] = P.In(torch.from_numpy(np.array(M)), align=4)
    outs = dict(offs=P.Out((F + 1,), torch.int64, align=8, sentinel=-7776))
    if layout == "packed":
        outs["body"] = P.Out((n * rec,), torch.uint8, align=out_align, sentinel=BYTE_SENT)
    else:
        outs["points"] = P.Out((n, 3), torch.float32, align=4)
        if rgb is not None:
            outs["colors"] = P.Out((n, 3), torch.uint8, align=out_align, sentinel=BYTE_SENT)
    wsb = lib.vda_cloud_workspace(F, H, W, step)
    assert wsb == 8 * (F * -(-(-(-H // step) * -(-W // step)) // span()) + F)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(i, o, w):
        rc = lib.vda_cloud_count(ptr(i["depth"]), ptr(i.get("valid")), F, H, W, step, trunc, ptr(o["offs"]), ptr(w["ws"]),
                                 wsb, stream)
        assert rc == 0, lib.vda_last_error()
        out = o["body"] if layout == "packed" else o["points"]
        rc = lib.vda_cloud_write(ptr(i["depth"]), ptr(i.get("valid")), ptr(i.get("rgb")), F, H, W, step, trunc, ptr(i["K"]),
                                 ptr(i.get("M")), LAYOUTS[layout], ctypes.c_void_p(out.data_ptr()) if n else ctypes.c_void_p(256),
                                 ptr(o.get("colors")) if n else ctypes.c_void_p(256), cap, ptr(w["ws"]), wsb, stream)
        assert rc == 0, lib.vda_last_error()

    def check(o):
        assert torch.equal(o["offs"], offs), f"frame_offsets {o['offs'].tolist()} != {offs.tolist()}"
        if layout == "packed":
            want = torch.full((n * rec,), BYTE_SENT, dtype=torch.uint8)
            body = pts.view(torch.uint8).reshape(-1, 12)
            body = body if col is None else torch.cat([body, col], 1)
            want[:cap * rec] = body.reshape(-1)[:cap * rec]
            bad = (o["body"] != want).nonzero()
            assert not len(bad), f"{len(bad)} body bytes differ, first at byte {int(bad[0])} (record {int(bad[0]) // rec})"
        else:
            want = torch.full((n, 3), P.SENT, dtype=torch.float32)
            want[:cap] = pts[:cap]
            bad = (o["points"].view(torch.int32) != want.view(torch.int32)).any(1).nonzero()
            assert not len(bad), f"{len(bad)} points differ, first at {int(bad[0])}"
            if col is not None:
                wantc = torch.full((n, 3), BYTE_SENT, dtype=torch.uint8)
                wantc[:cap] = col[:cap]
                bad = (o["colors"] != wantc).any(1).nonzero()
                assert not len(bad), f"{len(bad)} colours differ, first at {int(bad[0])}"
        return 0.

    P.run_placed(call, ops, outs, {"ws": wsb}, check=check, what=what or f"cloud {layout} {depth.shape} step {step}",
                 device="cuda")
    return n


@pytest.mark.parametrize("layout", ["split", "packed"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 3, 5), (2, 7, 67), (2, 37, 113)])
@pytest.mark.parametrize("with_m", [True, False])
@pytest.mark.parametrize("with_rgb", [True, False])
def test_small_shapes(shape, layout, with_m, with_rgb):
    depth, rgb, K, M = clip(*shape)
    valid = pattern("half", *shape) if shape[1] > 1 else None
    run_case(depth, valid, rgb if with_rgb else None, K, M if with_m else None, 1, layout)


@pytest.mark.parametrize("layout", ["split", "packed"])
@pytest.mark.parametrize("name", PATTERNS)
def test_keep_patterns_across_block_ends(name, layout):
    shape = big_shape()
    assert shape[1] * shape[2] == 2 * span() + 37
    depth, rgb, K, M = clip(*shape)
    n = run_case(depth, pattern(name, *shape), rgb, K, M, 1, layout, out_align=1)
    assert (n == 0) == (name == "none")


@pytest.mark.parametrize("layout", ["split", "packed"])
def test_dropped_depths_select_out(layout):
    """The predicate on the depth itself, no mask: 0, negative, NaN, +-Inf, trunc and the clip value drop out; the
    fp32 just below trunc stays."""
    shape = big_shape()
    depth, rgb, K, M = clip(*shape)
    depth = np.array(depth)
    bad = np.random.default_rng(5).random(shape)
    below = np.nextafter(np.float32(TRUNC), np.float32(0))
    for k, v in enumerate([0., -1., np.nan, np.inf, -np.inf, TRUNC, 80., -0., below]):
        depth[(bad > 0.05 * k) & (bad < 0.05 * (k + 1))] = v
    n = run_case(depth, None, rgb, K, M, 1, layout)
    assert n == int(((bad >= 0.45) | ((bad > 0.40) & (bad < 0.45))).sum())


@pytest.mark.parametrize("layout", ["split", "packed"])
@pytest.mark.parametrize("step", [2, 3])
@pytest.mark.parametrize("shape", [(2, 7, 67), "big"])
def test_step(shape, step, layout):
    shape = big_shape() if shape == "big" else shape
    shape = (shape[0], shape[1] * step - 1, shape[2] * step - (step - 1))  # H, W no multiples of step
    assert shape[1] % step and shape[2] % step
    depth, rgb, K, M = clip(*shape)
    run_case(depth, pattern("half", *shape), rgb, K, M, step, layout)


@pytest.mark.parametrize("with_rgb", [True, False])
@pytest.mark.parametrize("off", [1, 2, 3])
def test_packed_body_at_any_byte_address(off, with_rgb):
    shape = big_shape()
    depth, rgb, K, M = clip(*shape)
    run_case(depth, pattern("runs", *shape), rgb if with_rgb else None, K, M, 1, "packed", out_align=off)
    shape = (1, 3, 5)
    depth, rgb, K, M = clip(*shape)
    run_case(depth, None, rgb if with_rgb else None, K, None, 1, "packed", out_align=off)


@pytest.mark.parametrize("layout", ["split", "packed"])
@pytest.mark.parametrize("cap", ["n-5", "0", "mid"])
def test_cap_stores_only_the_first_records(cap, layout):
    shape = big_shape()
    depth, rgb, K, M = clip(*shape)
    valid = pattern("half", *shape)
    n = reference(depth, valid, None, K, None, 1)[3]
    cap = {"n-5": n - 5, "0": 0, "mid": span() // 2 + 3}[cap]  # mid: the cut lies about where the first block's records end
    assert run_case(depth, valid, rgb, K, M, 1, layout, out_align=3, cap=cap) == n


def device_cloud(depth, valid, rgb, K, M, layout="split", step=1):
    dev = torch.device("cuda")
    t = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)  # noqa: E731
    d, v, c, k, m = t(depth), t(valid), t(rgb), t(K), t(M)
    offs, ws = PC.LibCloud.count(d, v, step, TRUNC)
    out, col = PC.LibCloud.write(d, v, c, k, m, step, TRUNC, ws, int(offs[-1]), layout)
    return out.cpu(), None if col is None else col.cpu(), offs.cpu()


def test_repeatable_and_frame_independent():
    shape = big_shape()
    depth, rgb, K, M = clip(*shape)
    valid = pattern("half", *shape)
    a = device_cloud(depth, valid, rgb, K, M, "packed")
    b = device_cloud(depth, valid, rgb, K, M, "packed")
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    one = device_cloud(depth[1:2], valid[1:2], rgb[1:2], K[1:2], M[1:2], "packed")
    lo, hi = int(a[2][1]), int(a[2][2])
    assert hi - lo == int(one[2][1]) > 0 and torch.equal(a[0][15 * lo:15 * hi], one[0])


@pytest.mark.parametrize("with_m", [True, False])
def test_error_bound_against_float64(with_m):
    shape = (2, 37, 113)
    depth, _, K, M = clip(*shape)
    valid = pattern("half", *shape)
    M = M if with_m else None
    pts, _, _ = device_cloud(depth, valid, None, K, M)
    ref, bound = R.cloud_f64(depth, valid, K, M, 1, TRUNC)
    ratio = np.abs(pts.numpy().astype(np.float64) - ref) / bound
    print(f"worst |err| / bound = {ratio.max():.3f}")
    assert ratio.max() <= 1.


def test_argument_checks_return_before_any_launch():
    lib = _lib.lib()
    fake = ctypes.c_void_p(0x1000)
    F, H, W = 2, 4, 6
    wsb = lib.vda_cloud_workspace(F, H, W, 1)

    def count(depth=fake, F=F, H=H, W=W, step=1, offs=fake, ws=fake, wsb=wsb):
        return lib.vda_cloud_count(depth, None, F, H, W, step, 80., offs, ws, wsb, None)

    def write(depth=fake, rgb=None, F=F, H=H, W=W, step=1, K=fake, layout=0, out=fake, out_rgb=None, cap=5, ws=fake, wsb=wsb):
        return lib.vda_cloud_write(depth, None, rgb, F, H, W, step, 80., K, None, layout, out, out_rgb, cap, ws, wsb, None)

    def rejected(rc, msg):
        assert rc == -22 and msg in lib.vda_last_error(), (rc, lib.vda_last_error())

    for fn in (count, write):
        rejected(fn(depth=None), b"null pointer")
        rejected(fn(ws=None), b"null pointer")
        rejected(fn(F=0), b"F >= 1")
        rejected(fn(F=65536), b"65535")
        rejected(fn(H=0), b"H >= 1")
        rejected(fn(W=0), b"W >= 1")
        rejected(fn(step=0), b"step >= 1")
        rejected(fn(wsb=wsb - 1), b"workspace smaller")
        rejected(fn(depth=ctypes.c_void_p(0x1002)), b"4-byte aligned")
        rejected(fn(H=2 ** 16, W=2 ** 16, wsb=2 ** 40), b"candidates per frame")
    rejected(count(offs=None), b"null pointer")
    rejected(write(K=None), b"null pointer")
    rejected(write(layout=2), b"unknown layout")
    rejected(write(cap=-1), b"cap >= 0")
    rejected(write(out=None), b"needs out")
    rejected(write(rgb=fake), b"needs out_rgb")
    rejected(write(out=ctypes.c_void_p(0x1001)), b"4-byte aligned out")
    assert lib.vda_cloud_workspace(0, 4, 6, 1) == 0 and lib.vda_cloud_workspace(2, 4, 6, 0) == 0
    assert lib.vda_cloud_span() % 64 == 0
    assert write(layout=1, out=ctypes.c_void_p(0x1001), cap=0) == 0  # nothing to store: no launch, any address


def test_unproject_on_the_device_equals_the_cpu_mirror():
    shape = (3, 37, 113)
    depth, rgb, K, _ = clip(*shape)
    intr = np.zeros((3, 3, 3), np.float32)
    intr[:, 0, 0], intr[:, 1, 1], intr[:, 0, 2], intr[:, 1, 2], intr[:, 2, 2] = K[:, 0], K[:, 1], K[:, 2], K[:, 3], 1
    E = np.tile(np.eye(4), (3, 1, 1))
    E[:, :3, 3] = np.arange(9).reshape(3, 3)
    valid = pattern("checker", *shape).astype(bool)
    kw = dict(rgb=np.array(rgb), valid=valid, max_depth=80., flip=np.diag([1., -1., -1., 1.]), step=2, frames=[2, 0, 2])
    cpu = PC.unproject_depths(np.array(depth), intr, E, **kw)
    gpu = PC.unproject_depths(torch.from_numpy(np.array(depth)).cuda(), intr, E, **kw)
    assert gpu.points.is_cuda and gpu.colors.is_cuda and gpu.frame_offsets.is_cuda and len(cpu) > 100
    assert torch.equal(gpu.points.cpu().view(torch.int32), cpu.points.view(torch.int32))
    assert torch.equal(gpu.colors.cpu(), cpu.colors) and torch.equal(gpu.frame_offsets.cpu(), cpu.frame_offsets)


def test_evaluate_then_cloud_then_ply(tmp_path):
    """evaluate_depth(return_aligned=True) on the device -> unproject_to_ply_bytes -> write_ply: the file is the CPU
    mirror's byte for byte, the mirror fed with the device's aligned tensor (only the new code is compared)."""
    from vda_amd.evaluate import evaluate_depth
    g = np.random.default_rng(2)
    N, H, W = 3, 37, 113
    gt = g.uniform(2., 70., (N, H, W)).astype(np.float32)
    valid = g.random((N, H, W)) < 0.8
    pred = (2.5 / gt + 0.3 + g.normal(0, 1e-3, gt.shape)).astype(np.float32)
    pred[:, :4] = 0.  # sky: aligned to max_depth, drops out of the cloud
    _, rgb, K, _ = clip(N, H, W)
    intr = np.array([[500., 0., W / 2], [0., 500., H / 2], [0., 0., 1.]], np.float32)
    res = evaluate_depth(torch.from_numpy(pred).cuda(), gt, valid, max_depth=80., return_aligned=True)
    assert res.aligned.is_cuda
    body = PC.unproject_to_ply_bytes(res.aligned, intr, rgb=np.array(rgb), max_depth=80.)
    assert body.is_cuda and body.dtype == torch.uint8
    n = PC.write_ply(str(tmp_path / "gpu.ply"), body, colors=True)
    ref = PC.unproject_to_ply_bytes(res.aligned.cpu(), intr, rgb=np.array(rgb), max_depth=80.)
    PC.write_ply(str(tmp_path / "cpu.ply"), ref, colors=True)
    assert 0 < n <= N * (H - 4) * W
    assert open(tmp_path / "gpu.ply", "rb").read() == open(tmp_path / "cpu.ply", "rb").read()
