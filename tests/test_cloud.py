"""Point clouds on the CPU: ``TorchCloud`` (the op-by-op torch mirror of vda_cloud_count / vda_cloud_write) against
the numpy restatements of tests/cloud_ref.py, the camera matrices, the PLY file, the reference-named wrappers and
the command line.  The GPU kernels are held to ``TorchCloud`` bit for bit in tests/test_gpu_cloud.py."""
import os
import sys

import numpy as np
import pytest
import torch

import cloud_ref as R
import vda_amd  # noqa: F401
from vda_amd import pointcloud as PC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scene(F=3, H=7, W=67, seed=0, keep=0.7):
    """depth with every kind of dropped value mixed in, valid, rgb, K, M (a rotation + translation per frame)."""
    g = np.random.default_rng(seed)
    depth = g.uniform(0.5, 60., (F, H, W)).astype(np.float32)
    bad = g.random((F, H, W))
    for k, v in enumerate([0., -1., np.nan, np.inf, -np.inf, 80., 1000.]):
        depth[(bad > 0.02 * k) & (bad < 0.02 * (k + 1))] = v
    valid = (g.random((F, H, W)) < keep).astype(np.uint8)
    rgb = g.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    K = np.stack([g.uniform(300, 900, F), g.uniform(300, 900, F), g.uniform(0, W, F), g.uniform(0, H, F)], 1).astype(np.float32)
    M = np.zeros((F, 3, 4), dtype=np.float32)
    for f in range(F):
        q, _ = np.linalg.qr(g.normal(size=(3, 3)))
        M[f, :, :3] = q
        M[f, :, 3] = g.uniform(-20, 20, 3)
    return depth, valid, rgb, K, M


def torch_cloud(depth, valid, rgb, K, M, step, trunc, layout="split", n=None):
    t = lambda a: None if a is None else torch.from_numpy(a)  # noqa: E731
    offs, ws = PC.TorchCloud.count(t(depth), t(valid), step, trunc)
    n = int(offs[-1]) if n is None else n
    out, col = PC.TorchCloud.write(t(depth), t(valid), t(rgb), t(K), t(M), step, trunc, ws, n, layout)
    return out.numpy(), None if col is None else col.numpy(), offs.numpy()


@pytest.mark.parametrize("step", [1, 2, 3])
@pytest.mark.parametrize("with_m", [True, False])
@pytest.mark.parametrize("with_rgb", [True, False])
def test_bit_identical_to_the_float32_restatement(step, with_m, with_rgb):
    depth, valid, rgb, K, M = scene()
    M, rgb = (M if with_m else None), (rgb if with_rgb else None)
    trunc = PC.depth_trunc(80.)
    pts, col, offs = torch_cloud(depth, valid, rgb, K, M, step, trunc)
    rp, rc, ro = R.cloud_f32(depth, valid, rgb, K, M, step, trunc)
    assert pts.dtype == np.float32 and pts.shape == rp.shape and len(rp) > 50
    assert np.array_equal(pts.view(np.uint32), rp.view(np.uint32))
    assert np.array_equal(offs, ro) and offs.dtype == np.int64 and offs[-1] == len(rp)
    assert (col is None and rc is None) or np.array_equal(col, rc)
    body, none, _ = torch_cloud(depth, valid, rgb, K, M, step, trunc, "packed")
    assert none is None and np.array_equal(body, R.packed(rp, rc))
    # no mask: all valid, as in the reference
    pts, _, offs = torch_cloud(depth, None, None, K, M, step, trunc)
    rp, _, ro = R.cloud_f32(depth, None, None, K, M, step, trunc)
    assert np.array_equal(pts.view(np.uint32), rp.view(np.uint32)) and np.array_equal(offs, ro)


@pytest.mark.parametrize("with_m", [True, False])
def test_error_bound_against_float64(with_m):
    worst = 0.
    for seed in range(20):
        depth, valid, _, K, M = scene(F=2, H=9, W=31, seed=seed)
        M = M if with_m else None
        trunc = PC.depth_trunc(1000.)
        pts, _, _ = torch_cloud(depth, valid, None, K, M, 1, trunc)
        ref, bound = R.cloud_f64(depth, valid, K, M, 1, trunc)
        assert pts.shape == ref.shape and bool((bound > 0).all())
        ratio = np.abs(pts.astype(np.float64) - ref) / bound
        assert np.isfinite(pts).all() and ratio.max() <= 1., f"seed {seed}: worst |err| / bound = {ratio.max():.3f}"
        worst = max(worst, float(ratio.max()))
    print(f"worst |err| / bound over 20 scenes = {worst:.3f} (the bound is 8 units of 2^-24 per magnitude)")


def test_predicate_edges():
    trunc = PC.depth_trunc(80.)
    below = float(np.nextafter(np.float32(trunc), np.float32(0)))
    row = np.array([[0., -1., np.nan, np.inf, trunc, below, 5., -np.inf, -0.]], dtype=np.float32)[None]  # [1, 1, 9]
    K = np.array([[100., 100., 4., 0.]], dtype=np.float32)
    pts, _, offs = torch_cloud(row, None, None, K, None, 1, trunc)
    assert offs.tolist() == [0, 2]
    assert pts[:, 2].tolist() == [below, 5.]
    assert pts[:, 0].tolist() == [float(np.float32(np.float32(1.) * np.float32(below)) / np.float32(100.)), float(np.float32(0.1))]
    # valid == 0 drops the two
    valid = np.ones_like(row, dtype=np.uint8)
    valid[0, 0, 6] = 0
    pts, _, offs = torch_cloud(row, valid, None, K, None, 1, trunc)
    assert offs.tolist() == [0, 1] and pts[:, 2].tolist() == [below]
    # nothing kept, everything kept
    pts, col, offs = torch_cloud(np.zeros((2, 3, 4), np.float32), None, np.zeros((2, 3, 4, 3), np.uint8),
                                 np.ones((2, 4), np.float32), None, 1, trunc)
    assert pts.shape == (0, 3) and col.shape == (0, 3) and offs.tolist() == [0, 0, 0]
    pts, _, offs = torch_cloud(np.full((2, 3, 4), 2., np.float32), None, None, np.ones((2, 4), np.float32), None, 1, trunc)
    assert pts.shape == (24, 3) and offs.tolist() == [0, 12, 24]
    # candidate order: row-major, the original i and j with a step
    pts, _, _ = torch_cloud(np.full((1, 3, 5), 2., np.float32), None, None, np.array([[2., 2., 0., 0.]], np.float32), None, 2, trunc)
    assert pts[:, :2].tolist() == [[0., 0.], [2., 0.], [4., 0.], [0., 2.], [2., 2.], [4., 2.]]


@pytest.mark.parametrize("max_depth", [10., 80., 655.35, 1000.])
def test_trunc_decides_as_the_double_compare(max_depth):
    t64 = np.float64(max_depth) - np.float64(1e-4)
    trunc = np.float32(PC.depth_trunc(max_depth))
    assert float(trunc) == PC.depth_trunc(max_depth) and np.float64(trunc) >= t64
    d = np.float32(max_depth)
    for _ in range(64):  # the floats around the threshold
        assert bool(d < trunc) == bool(np.float64(d) < t64)
        d = np.nextafter(d, np.float32(0))
    assert not np.float32(max_depth) < trunc  # the clip value of the aligned depth drops out


def test_camera_matrices():
    g = np.random.default_rng(3)
    E = np.tile(np.eye(4), (4, 1, 1))
    for f in range(4):
        q, _ = np.linalg.qr(g.normal(size=(3, 3)))
        E[f, :3, :3], E[f, :3, 3] = q, g.uniform(-5, 5, 3)
    flip = np.diag([1., -1., -1., 1.])
    flip[0, 3] = 2.  # not commuting with the pose: the order shows
    M = PC.camera_matrices(E.astype(np.float32), flip=flip)
    E32 = E.astype(np.float32).astype(np.float64)
    want = (flip[None] @ np.linalg.inv(E32))[:, :3].astype(np.float32)
    assert M.dtype == torch.float32 and tuple(M.shape) == (4, 3, 4) and np.array_equal(M.numpy(), want)
    assert not np.allclose(want, (np.linalg.inv(E32) @ flip[None])[:, :3])
    c2w = PC.camera_matrices(torch.from_numpy(E), cam_to_world=True)
    assert np.array_equal(c2w.numpy(), E[:, :3].astype(np.float32))
    assert np.array_equal(PC.camera_matrices(None, frames=2).numpy(), np.tile(np.eye(4)[:3], (2, 1, 1)).astype(np.float32))
    bad = E.copy()
    bad[1, 3] = [0., 0., 1e-3, 1.]
    with pytest.raises(ValueError, match="affine"):
        PC.camera_matrices(bad)
    with pytest.raises(ValueError, match="affine"):
        PC.camera_matrices(E, flip=np.diag([1., 1., 1., 2.]))


def test_unproject_depths_frames_and_intrinsics_layouts():
    depth, valid, rgb, K, _ = scene(F=4, H=5, W=9)
    intr = np.zeros((4, 3, 3), np.float32)
    intr[:, 0, 0], intr[:, 1, 1], intr[:, 0, 2], intr[:, 1, 2], intr[:, 2, 2] = K[:, 0], K[:, 1], K[:, 2], K[:, 3], 1
    E = np.tile(np.eye(4), (4, 1, 1))
    E[:, :3, 3] = np.arange(12).reshape(4, 3)
    c = PC.unproject_depths(depth, intr, E, rgb=rgb, valid=valid, max_depth=80., frames=[2, 0, 2])
    M = PC.camera_matrices(E).numpy()
    pick = [2, 0, 2]
    rp, rc, ro = R.cloud_f32(depth[pick], valid[pick], rgb[pick], K[pick], M[pick], 1, PC.depth_trunc(80.))
    assert np.array_equal(c.points.numpy().view(np.uint32), rp.view(np.uint32))
    assert np.array_equal(c.colors.numpy(), rc) and np.array_equal(c.frame_offsets.numpy(), ro) and len(c) == len(rp)
    one = PC.unproject_depths(torch.from_numpy(depth), intr[0], max_depth=80.)  # one pinhole for all, no pose
    rp, _, _ = R.cloud_f32(depth, None, None, np.tile(K[:1], (4, 1)), None, 1, PC.depth_trunc(80.))
    assert one.colors is None and np.array_equal(one.points.numpy().view(np.uint32), rp.view(np.uint32))


def test_ply_files(tmp_path):
    depth, valid, rgb, K, M = scene(F=2, H=5, W=9)
    trunc = PC.depth_trunc(80.)
    pts, col, offs = torch_cloud(depth, valid, rgb, K, M, 1, trunc)
    n = len(pts)
    head = ("ply\nformat binary_little_endian 1.0\ncomment Created by vda-mi355x\nelement vertex %d\n"
            "property float x\nproperty float y\nproperty float z\n%send_header\n")
    rgb_props = "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    for colors in (True, False):
        cloud = PC.PointCloud(torch.from_numpy(pts), torch.from_numpy(col) if colors else None, torch.from_numpy(offs))
        path = str(tmp_path / f"c{int(colors)}.ply")
        assert PC.write_ply(path, cloud) == n
        data = open(path, "rb").read()
        want_head = (head % (n, rgb_props if colors else "")).encode()
        assert data[:len(want_head)] == want_head and len(data) == len(want_head) + (15 if colors else 12) * n
        assert data[len(want_head):] == R.packed(pts, col if colors else None).tobytes()
        back = PC.read_ply(path)
        assert np.array_equal(back.points.numpy().view(np.uint32), pts.view(np.uint32))
        assert (back.colors is None) == (not colors) and (not colors or np.array_equal(back.colors.numpy(), col))
        # the byte body gives the same file
        body, _, _ = torch_cloud(depth, valid, rgb if colors else None, K, M, 1, trunc, "packed")
        path2 = str(tmp_path / f"b{int(colors)}.ply")
        assert PC.write_ply(path2, torch.from_numpy(body), colors=colors) == n
        assert open(path2, "rb").read() == data
        # an empty cloud is a valid file
        empty = str(tmp_path / f"e{int(colors)}.ply")
        assert PC.write_ply(empty, torch.zeros(0, dtype=torch.uint8), colors=colors) == 0
        assert open(empty, "rb").read() == (head % (0, rgb_props if colors else "")).encode()
        assert len(PC.read_ply(empty)) == 0
    with pytest.raises(ValueError, match="whole number"):
        PC.write_ply(str(tmp_path / "x.ply"), torch.zeros(13, dtype=torch.uint8), colors=False)


def synthetic_sample(N=3, H=6, W=10, seed=5):
    g = np.random.default_rng(seed)
    E = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))
    E[:, :3, 3] = g.uniform(-3, 3, (N, 3)).astype(np.float32)
    intr = np.tile(np.array([[400., 0., W / 2], [0., 410., H / 2], [0., 0., 1.]], np.float32), (N, 1, 1))
    depth = g.uniform(1., 30., (N, H, W)).astype(np.float32)
    depth[:, 0, :3] = 1000.  # clipped sky
    return dict(image=torch.from_numpy(g.random((N, 3, H, W)).astype(np.float32)), depth=torch.from_numpy(depth),
                valid_depth=torch.ones(N, H, W, dtype=torch.bool), intrinsics=torch.from_numpy(intr),
                extrinsics=torch.from_numpy(E))


def test_project_scene_to_3d_is_the_concatenation_of_its_frames(tmp_path):
    sample = synthetic_sample()
    flip = np.diag([1., -1., -1., 1.])
    path = str(tmp_path / "scene.ply")
    n = PC.project_scene_to_3d(sample, [2, 0, 2], path, max_depth=1000., Flip_to_open3d=flip, Visualise_cam_pos=True)
    merged = PC.read_ply(path)
    singles = [PC.project_image_to_pointcloud(sample, i, max_depth=1000., Flip_to_open3d=flip) for i in (2, 0, 2)]
    assert n == len(merged) == sum(len(s) for s in singles) == 3 * (6 * 10 - 3)
    assert torch.equal(merged.points.view(torch.int32), torch.cat([s.points for s in singles]).view(torch.int32))
    assert torch.equal(merged.colors, torch.cat([s.colors for s in singles]))
    # the colours: image * 255 truncated, as the reference's astype(np.uint8)
    img = (sample["image"][0].permute(1, 2, 0).numpy() * 255.).astype(np.uint8)
    keep = sample["depth"][0].numpy() < 999.
    assert np.array_equal(singles[1].colors.numpy(), img[keep])
    one = str(tmp_path / "one.ply")
    assert PC.project_image_to_3d(sample, 1, one, Flip_to_open3d=flip) == 57
    assert torch.equal(PC.read_ply(one).points, PC.project_image_to_pointcloud(sample, 1, Flip_to_open3d=flip).points)
    # extrinsics None: the reference's TypeError fallback, identity
    nopose = dict(sample, extrinsics=None)
    c = PC.project_image_to_pointcloud(nopose, 1)
    assert torch.equal(c.points[:, 2], sample["depth"][1][sample["depth"][1] < 999.])


def test_cli_on_the_cpu(tmp_path):
    import cloud as cli
    g = np.random.default_rng(11)
    N, H, W = 4, 6, 8
    gt = g.uniform(2., 40., (N, H, W)).astype(np.float32)
    valid = g.random((N, H, W)) < 0.9
    pred = (1. / gt * 3. + 0.5).astype(np.float32)  # inverse depth up to scale and shift
    pred[:, 0, 0] = 0.  # aligned to max_depth: drops out
    valid[:, 0, 0] = False  # and takes no part in the fit
    np.savez(tmp_path / "pred.npz", depths=pred)
    np.savez(tmp_path / "scene.npz", depth=gt, valid_depth=valid, max_depth=80.)
    E = np.tile(np.eye(4), (N, 1, 1))
    E[:, 0, 3] = np.arange(N)
    intr = np.array([[300., 0., 4.], [0., 300., 3.], [0., 0., 1.]], np.float32)
    np.savez(tmp_path / "cams.npz", intrinsics=intr, extrinsics=E)
    rgb = g.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    np.save(tmp_path / "clip.npy", rgb)
    out = str(tmp_path / "o" / "scene.ply")
    n = cli.main(["--depth", str(tmp_path / "pred.npz"), "--gt", str(tmp_path / "scene.npz"), "--camera",
                  str(tmp_path / "cams.npz"), "--rgb", str(tmp_path / "clip.npy"), "--every", "2", "--step", "2", "--out", out,
                  "--device", "cpu"])
    from vda_amd.evaluate import evaluate_depth
    aligned = evaluate_depth(pred, gt, valid, max_depth=80., align="all", return_aligned=True).aligned
    want = PC.unproject_depths(aligned, intr, E, rgb=rgb, max_depth=80., step=2, frames=[0, 2])
    got = PC.read_ply(out)
    assert n == len(got) == len(want) == 2 * (3 * 4 - 1)
    assert torch.equal(got.points.view(torch.int32), want.points.view(torch.int32)) and torch.equal(got.colors, want.colors)
    assert np.allclose(got.points[:, 2].numpy(), gt[[0, 2]][:, ::2, ::2].reshape(-1)[np.r_[1:12, 13:24]], rtol=1e-3)
    # without --gt: metric depth as it is (a cloud of the ground truth itself), no colours, one pinhole
    out2 = str(tmp_path / "gt.ply")
    n2 = cli.main(["--depth", str(tmp_path / "scene.npz"), "--intrinsics", "300", "300", "4", "3", "--frames", "3", "1",
                   "--out", out2, "--device", "cpu"])
    want = PC.unproject_depths(gt, intr, max_depth=1000., frames=[3, 1])
    got = PC.read_ply(out2)
    assert n2 == len(want) == 2 * H * W and got.colors is None
    assert torch.equal(got.points.view(torch.int32), want.points.view(torch.int32))


def test_ops_wrappers_reject_before_the_device():
    from vda_amd import ops
    d = torch.zeros(1, 2, 2)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.cloud_count(d, trunc=1.)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.cloud_write(d, None, None, torch.ones(1, 4), None, trunc=1., ws=torch.zeros(8, dtype=torch.uint8), n=0)


def test_meta_shapes():
    import vda_amd.torch_ops  # noqa: F401
    d = torch.empty(3, 10, 20, device="meta")
    offs, ws = torch.ops.vda.cloud_count(d, None, 2, 80.)
    assert offs.shape == (4,) and offs.dtype == torch.int64 and ws.dtype == torch.uint8 and ws.numel() == (3 + 3) * 8
    K, M = torch.empty(3, 4, device="meta"), torch.empty(3, 3, 4, device="meta")
    rgb = torch.empty(3, 10, 20, 3, device="meta", dtype=torch.uint8)
    p, c = torch.ops.vda.cloud_write(d, None, rgb, K, M, 2, 80., 0, ws, 17)
    assert p.shape == (17, 3) and p.dtype == torch.float32 and c.shape == (17, 3) and c.dtype == torch.uint8
    b, c = torch.ops.vda.cloud_write(d, None, rgb, K, None, 2, 80., 1, ws, 17)
    assert b.shape == (17 * 15,) and b.dtype == torch.uint8 and c is None
    b, _ = torch.ops.vda.cloud_write(d, None, None, K, None, 2, 80., 1, ws, 17)
    assert b.shape == (17 * 12,)
