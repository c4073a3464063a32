"""Point clouds from metric depth: the reference's ``datasets/visualisation_utils.py:82-187`` without Open3D.

The reference unprojects each frame through the pinhole intrinsics (``RGBDImage.create_from_color_and_depth``
with ``depth_trunc = max_depth - 1e-4``, ``PointCloud.create_from_rgbd_image``), moves it to world space with
the extrinsics and a flip (two ``transform`` calls), merges the frames (``+=``) and writes a ``.ply``
(``write_point_cloud``), all on the host.  Here a clip that lies on the device (for instance the aligned metric
depth ``evaluate_depth(..., return_aligned=True)`` leaves there) becomes a cloud in two bandwidth-bound passes
(``vda_cloud_count`` / ``vda_cloud_write``, csrc/vda_cloud.hip): an order-preserving stream compaction fused
with the unprojection.  The points come back as tensors or as the finished body of a binary PLY.

The arithmetic is stated once, in include/vda.h: candidates are every ``step``-th row and column in row-major
order, frames in index order; a candidate is kept when it is valid, ``d > 0`` and ``d < trunc``; per point
every operation is one rounded fp32 operation.  Deviations from the reference: Open3D computes in double,
divides by the homogeneous ``w`` and writes double coordinates; here the arithmetic is fp32, the matrix affine
(a projective last row is rejected) and the file holds floats.  Open3D is not a dependency, and parity with it
is not pinned by a test.

* ``LibCloud`` / ``TorchCloud`` - the two backends: libvda kernels, and the same arithmetic op by op in plain
  torch on any device (the CPU tests and ``--device cpu`` run on it; it is not a fallback of the product path).
* ``camera_matrices`` - extrinsics and flip to the [F, 3, 4] fp32 matrices the kernels take.
* ``unproject_depths`` -> ``PointCloud``; ``unproject_to_ply_bytes`` -> the PLY body as one uint8 tensor.
* ``write_ply`` / ``read_ply`` - binary little-endian PLY, float coordinates, optional uchar colours.
* ``project_image_to_pointcloud`` / ``project_image_to_3d`` / ``project_scene_to_3d`` - the reference's names
  on the reference's sample dict.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

LAYOUTS = ("split", "packed")


def depth_trunc(max_depth: float) -> float:
    """The fp32 threshold that decides ``d < trunc`` for every fp32 ``d`` as Open3D's compare of the float
    pixel against the double ``max_depth - 1e-4`` does: the smallest fp32 that is >= that double."""
    t = np.float64(max_depth) - np.float64(1e-4)
    f = np.float32(t)
    if np.float64(f) < t:
        f = np.nextafter(f, np.float32(np.inf))
    return float(f)


class LibCloud:
    """The cloud arithmetic on libvda kernels (GPU tensors only):
    ``count(depth, valid, step, trunc)`` -> (frame_offsets [F + 1] int64, ws) and
    ``write(depth, valid, rgb, K, M, step, trunc, ws, n, layout)`` -> (points [n, 3] fp32, colors [n, 3] uint8 or
    None) for ``"split"``, (body [n * 12 | n * 15] uint8, None) for ``"packed"``; all on the device.  ``ws``
    carries the block offsets from ``count`` to ``write``."""

    @staticmethod
    def count(depth, valid, step: int, trunc: float):
        from . import ops
        return ops.cloud_count(depth, valid, step=step, trunc=trunc)

    @staticmethod
    def write(depth, valid, rgb, K, M, step: int, trunc: float, ws, n: int, layout: str = "split"):
        from . import ops
        return ops.cloud_write(depth, valid, rgb, K, M, step=step, trunc=trunc, ws=ws, n=n, layout=layout)


class TorchCloud:
    """``LibCloud``'s contract in plain torch on any device: the same fp32 operations, every one a separate,
    separately rounded op (divisions by tensors), a boolean gather for the compaction.  ``ws`` is None."""

    @staticmethod
    def _keep(depth, valid, step, trunc):
        d = depth[:, ::step, ::step]
        keep = (d > 0) & (d < torch.tensor(trunc, dtype=torch.float32, device=depth.device))
        if valid is not None:
            keep = keep & (valid[:, ::step, ::step] != 0)
        return d, keep

    @staticmethod
    def count(depth, valid, step: int, trunc: float):
        _, keep = TorchCloud._keep(depth, valid, step, trunc)
        counts = keep.reshape(keep.shape[0], -1).sum(1, dtype=torch.int64)
        return torch.cat([counts.new_zeros(1), counts.cumsum(0)]), None

    @staticmethod
    def write(depth, valid, rgb, K, M, step: int, trunc: float, ws, n: int, layout: str = "split"):
        if layout not in LAYOUTS:
            raise ValueError(f"layout must be one of {LAYOUTS}, got {layout!r}")
        F, H, W = depth.shape
        dev = depth.device
        z, keep = TorchCloud._keep(depth, valid, step, trunc)
        jj = torch.arange(0, W, step, device=dev).to(torch.float32)[None, None, :]
        ii = torch.arange(0, H, step, device=dev).to(torch.float32)[None, :, None]
        fx, fy, cx, cy = (K[:, c].reshape(F, 1, 1) for c in range(4))
        x = (jj - cx) * z / fx
        y = (ii - cy) * z / fy
        p = [x, y, z]
        if M is not None:
            m = M.reshape(F, 3, 4, 1, 1)
            p = [((m[:, r, 0] * x + m[:, r, 1] * y) + m[:, r, 2] * z) + m[:, r, 3] for r in range(3)]
        points = torch.stack(p, -1)[keep][:n].contiguous()
        colors = None if rgb is None else rgb[:, ::step, ::step][keep][:n].contiguous()
        if layout == "split":
            return points, colors
        body = points.view(torch.uint8).reshape(-1, 12)
        if colors is not None:
            body = torch.cat([body, colors], 1)
        return body.reshape(-1), None


def camera_matrices(extrinsics, cam_to_world: bool = False, flip=None, frames: Optional[int] = None) -> torch.Tensor:
    """[F, 3, 4] fp32 camera-to-output matrices: in float64 ``flip @ (E if cam_to_world else inv(E))`` per frame,
    rounded once to fp32 (the reference inverts in the sample's float32 and applies the two transforms one after
    the other in double).  ``extrinsics`` [F, 4, 4] (or [4, 4]); None gives identity poses for ``frames`` frames,
    the reference's ``TypeError`` fallback.  ``flip`` [4, 4], None = identity.  The kernels' matrix is affine: a
    last row other than (0, 0, 0, 1) in ``extrinsics`` or ``flip`` is rejected."""
    last = np.array([0., 0., 0., 1.])
    if extrinsics is None:
        if frames is None:
            raise ValueError("camera_matrices needs `frames` when extrinsics is None")
        E = np.broadcast_to(np.eye(4), (int(frames), 4, 4)).copy()
    else:
        E = np.asarray(extrinsics.detach().cpu() if isinstance(extrinsics, torch.Tensor) else extrinsics, dtype=np.float64)
        if E.ndim == 2:
            E = E[None]
        if E.ndim != 3 or E.shape[1:] != (4, 4):
            raise ValueError(f"extrinsics must be [F, 4, 4], got {E.shape}")
        if frames is not None and E.shape[0] != frames:
            raise ValueError(f"{E.shape[0]} extrinsics for {frames} frames")
    Fl = np.eye(4) if flip is None else np.asarray(flip.detach().cpu() if isinstance(flip, torch.Tensor) else flip,
                                                     dtype=np.float64)
    if Fl.shape != (4, 4):
        raise ValueError(f"flip must be [4, 4], got {Fl.shape}")
    if not (np.array_equal(Fl[3], last) and bool((E[:, 3] == last).all())):
        raise ValueError("extrinsics and flip must be affine: their last row must be (0, 0, 0, 1)")
    T = E if cam_to_world else np.linalg.inv(E)
    M = (Fl[None] @ T)[:, :3, :]
    return torch.from_numpy(np.ascontiguousarray(M.astype(np.float32)))


@dataclass
class PointCloud:
    """``points`` [N, 3] fp32, ``colors`` [N, 3] uint8 or None, ``frame_offsets`` [F + 1] int64 (frame f owns the
    points ``frame_offsets[f] : frame_offsets[f + 1]``); tensors on the input's device."""
    points: torch.Tensor
    colors: Optional[torch.Tensor]
    frame_offsets: torch.Tensor

    def __len__(self):
        return int(self.points.shape[0])


def _tensor(x, dtype, device, name):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{name} must be a numpy array or a tensor, got {type(x).__name__}")
    if device is not None and x.device != device:
        x = x.to(device)
    if dtype is not None and x.dtype != dtype:
        x = x.to(dtype)
    return x


def _prepare(depth, intrinsics, extrinsics, rgb, valid, max_depth, cam_to_world, flip, step, frames):
    depth = _tensor(depth, torch.float32, None, "depth")
    if depth.dim() != 3 or depth.numel() < 1:
        raise ValueError(f"depth must be a non-empty [F, H, W], got {tuple(depth.shape)}")
    if int(step) != step or int(step) < 1:
        raise ValueError(f"step must be an integer >= 1, got {step!r}")
    if not float(max_depth) - 1e-4 > 0:
        raise ValueError(f"max_depth must be greater than 1e-4, got {max_depth}")
    dev, N = depth.device, depth.shape[0]
    intr = _tensor(intrinsics, torch.float32, torch.device("cpu"), "intrinsics")
    if intr.dim() == 2:
        intr = intr[None].expand(N, 3, 3)
    if tuple(intr.shape) != (N, 3, 3):
        raise ValueError(f"intrinsics must be [F, 3, 3] or [3, 3], got {tuple(intr.shape)}")
    K = torch.stack([intr[:, 0, 0], intr[:, 1, 1], intr[:, 0, 2], intr[:, 1, 2]], 1)
    if rgb is not None:
        rgb = _tensor(rgb, None, dev, "rgb")
        if rgb.dtype != torch.uint8 or tuple(rgb.shape) != tuple(depth.shape) + (3,):
            raise ValueError(f"rgb must be uint8 [F, H, W, 3], got {rgb.dtype} {tuple(rgb.shape)}")
    if valid is not None:
        valid = _tensor(valid, None, dev, "valid")
        if valid.dtype not in (torch.bool, torch.uint8) or valid.shape != depth.shape:
            raise ValueError(f"valid must be bool / uint8 with depth's shape, got {valid.dtype} {tuple(valid.shape)}")
    M = None
    if extrinsics is not None or flip is not None:
        M = camera_matrices(extrinsics, cam_to_world, flip, frames=N)
    if frames is not None:  # any index list, repeated and unordered: gather the frames first
        idx = torch.as_tensor(list(frames), dtype=torch.int64)
        if idx.numel() < 1 or int(idx.min()) < -N or int(idx.max()) >= N:
            raise ValueError(f"frames must index the {N} frames, got {list(frames)}")
        K = K[idx]
        M = None if M is None else M[idx]
        idx = idx.to(dev)
        depth = depth[idx]
        rgb = None if rgb is None else rgb[idx]
        valid = None if valid is None else valid[idx]
    depth = depth.contiguous()
    rgb = None if rgb is None else rgb.contiguous()
    valid = None if valid is None else valid.contiguous()
    return depth, valid, rgb, K.contiguous().to(dev), (None if M is None else M.contiguous().to(dev)), int(step), \
        depth_trunc(max_depth)


def _run(layout, depth, intrinsics, extrinsics, rgb, valid, max_depth, cam_to_world, flip, step, frames, backend):
    depth, valid, rgb, K, M, step, trunc = _prepare(depth, intrinsics, extrinsics, rgb, valid, max_depth, cam_to_world,
                                                    flip, step, frames)
    if backend is None:
        backend = LibCloud if depth.is_cuda else TorchCloud
    offs, ws = backend.count(depth, valid, step, trunc)
    n = int(offs[-1])  # the one host sync: it sizes the output
    out, colors = backend.write(depth, valid, rgb, K, M, step, trunc, ws, n, layout)
    return out, colors, offs


def unproject_depths(depth, intrinsics, extrinsics=None, rgb=None, valid=None, max_depth: float = 1000.,
                     cam_to_world: bool = False, flip=None, step: int = 1, frames=None, backend=None) -> PointCloud:
    """Metric ``depth`` [F, H, W] (metres; numpy or tensor, used where it lies) to one merged cloud.

    ``intrinsics`` [F, 3, 3] or [3, 3] pinhole matrices (the reference's sample layout); ``extrinsics`` [F, 4, 4]
    world-to-camera (camera-to-world with ``cam_to_world``) or None (identity); ``flip`` a [4, 4] applied after
    the pose; ``rgb`` [F, H, W, 3] uint8; ``valid`` [F, H, W] bool / uint8 (None = all valid, as in the
    reference); depths outside ``0 < d < max_depth - 1e-4`` drop out; ``step`` takes every step-th row and
    column; ``frames`` any index list (repeated, unordered), applied by gathering the frames first.  The result
    stays on ``depth``'s device; the only host sync reads the number of points to size the output."""
    points, colors, offs = _run("split", depth, intrinsics, extrinsics, rgb, valid, max_depth, cam_to_world, flip, step,
                                frames, backend)
    return PointCloud(points, colors, offs)


def unproject_to_ply_bytes(depth, intrinsics, extrinsics=None, rgb=None, valid=None, max_depth: float = 1000.,
                           cam_to_world: bool = False, flip=None, step: int = 1, frames=None, backend=None) -> torch.Tensor:
    """``unproject_depths``'s arguments -> the body of the binary PLY as one uint8 tensor on ``depth``'s device:
    records of 12 bytes (float x y z), or 15 with ``rgb`` (+ uchar r g b), little-endian."""
    body, _, _ = _run("packed", depth, intrinsics, extrinsics, rgb, valid, max_depth, cam_to_world, flip, step, frames,
                      backend)
    return body


def ply_header(n: int, colors: bool) -> bytes:
    props = "property float x\nproperty float y\nproperty float z\n"
    if colors:
        props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    return (f"ply\nformat binary_little_endian 1.0\ncomment Created by vda-mi355x\nelement vertex {int(n)}\n"
            f"{props}end_header\n").encode("ascii")


def write_ply(path: str, cloud_or_bytes, colors: Optional[bool] = None) -> int:
    """Write a binary little-endian PLY: a ``PointCloud``, or the uint8 body of ``unproject_to_ply_bytes`` with
    ``colors`` saying whether its records carry colours (15 bytes) or not (12).  Returns the number of points;
    none gives a valid empty file.  Deviation: Open3D writes double coordinates, this file holds floats."""
    if isinstance(cloud_or_bytes, PointCloud):
        c = cloud_or_bytes
        body = c.points.detach().cpu().contiguous().view(torch.uint8).reshape(-1, 12)
        colors = c.colors is not None
        if colors:
            body = torch.cat([body, c.colors.detach().cpu()], 1)
        body = body.reshape(-1)
    else:
        if colors is None:
            raise ValueError("write_ply of a byte body needs colors=True / False")
        body = _tensor(cloud_or_bytes, None, None, "body").detach().cpu().reshape(-1)
        if body.dtype != torch.uint8:
            raise ValueError(f"a PLY body is uint8, got {body.dtype}")
    rec = 15 if colors else 12
    if body.numel() % rec:
        raise ValueError(f"a body of {body.numel()} bytes is not a whole number of {rec}-byte records")
    n = body.numel() // rec
    with open(path, "wb") as f:
        f.write(ply_header(n, bool(colors)))
        body.contiguous().numpy().tofile(f)
    return n


def read_ply(path: str) -> PointCloud:
    """Read back a file ``write_ply`` wrote (that subset of PLY only); ``frame_offsets`` is [0, N]."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if end < 0:
        raise ValueError(f"{path}: no PLY header")
    lines = data[:end].decode("ascii").split("\n")
    body = data[end + len(b"end_header\n"):]
    if lines[:2] != ["ply", "format binary_little_endian 1.0"]:
        raise ValueError(f"{path}: not a binary little-endian PLY")
    n = [int(l.split()[2]) for l in lines if l.startswith("element vertex ")]
    props = [l for l in lines if l.startswith("property ")]
    xyz = ["property float x", "property float y", "property float z"]
    col = ["property uchar red", "property uchar green", "property uchar blue"]
    if len(n) != 1 or props not in (xyz, xyz + col):
        raise ValueError(f"{path}: not a PLY this module writes")
    n, colors = n[0], props == xyz + col
    rec = 15 if colors else 12
    if len(body) != n * rec:
        raise ValueError(f"{path}: {len(body)} body bytes for {n} records of {rec}")
    raw = np.frombuffer(body, dtype=np.uint8).reshape(n, rec)
    points = torch.from_numpy(np.ascontiguousarray(raw[:, :12]).view("<f4").reshape(n, 3).copy())
    cols = torch.from_numpy(raw[:, 12:].copy()) if colors else None
    return PointCloud(points, cols, torch.tensor([0, n], dtype=torch.int64))


def _sample_args(sample, idx):
    """The reference's sample dict -> unproject arguments for the frames ``idx``: ``image`` [N, 3, H, W] in 0..1
    (-> uint8 by truncation, as the reference's astype does), ``depth`` [N, H, W], ``intrinsics`` [N, 3, 3],
    ``extrinsics`` [N, 4, 4] or None.  ``valid_depth`` is not applied: the reference's mask line is commented out."""
    idx = [int(i) for i in idx]
    depth = _tensor(sample["depth"], torch.float32, None, "sample['depth']")[idx]
    image = _tensor(sample["image"], None, None, "sample['image']")[idx]
    rgb = (image.permute(0, 2, 3, 1) * 255.).to(torch.uint8)
    intr = _tensor(sample["intrinsics"], torch.float32, None, "sample['intrinsics']")[idx]
    ext = sample.get("extrinsics")
    if ext is not None:
        ext = _tensor(ext, None, None, "sample['extrinsics']")[idx]
    return depth, intr, ext, rgb.to(depth.device)


def project_image_to_pointcloud(sample, image_idx, max_depth: float = 1000., Cam_to_World: bool = False,
                                Flip_to_open3d=None, step: int = 1, backend=None) -> PointCloud:
    """visualisation_utils.py:82-127: one frame of the sample as a coloured cloud."""
    depth, intr, ext, rgb = _sample_args(sample, [image_idx])
    return unproject_depths(depth, intr, ext, rgb=rgb, max_depth=max_depth, cam_to_world=Cam_to_World,
                            flip=Flip_to_open3d, step=step, backend=backend)


def project_image_to_3d(sample, image_idx, save_path, max_depth: float = 1000., Cam_to_World: bool = False,
                        Flip_to_open3d=None, step: int = 1, backend=None) -> int:
    """visualisation_utils.py:129-133: one frame's cloud written to ``save_path``."""
    return project_scene_to_3d(sample, [image_idx], save_path, max_depth, Cam_to_World, Flip_to_open3d, step=step,
                               backend=backend)


def project_scene_to_3d(sample, multiple_img_idx, save_path, max_depth: float = 1000., Cam_to_World: bool = False,
                        Flip_to_open3d=None, Visualise_cam_pos: bool = False, step: int = 1, backend=None) -> int:
    """visualisation_utils.py:135-187: the frames ``multiple_img_idx`` (repeated and unordered as given) merged in
    that order and written to ``save_path``; returns the number of points.  ``Visualise_cam_pos`` (a matplotlib
    plot of the camera path in the reference) is accepted and ignored."""
    depth, intr, ext, rgb = _sample_args(sample, multiple_img_idx)
    body = unproject_to_ply_bytes(depth, intr, ext, rgb=rgb, max_depth=max_depth, cam_to_world=Cam_to_World,
                                  flip=Flip_to_open3d, step=step, backend=backend)
    return write_ply(save_path, body, colors=True)
