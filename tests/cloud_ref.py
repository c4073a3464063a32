"""Host restatements of the point-cloud arithmetic of include/vda.h (vda_cloud_count / vda_cloud_write).

``cloud_f32``: numpy float32, op by op - what the kernels and ``TorchCloud`` must equal bit for bit.
``cloud_f64``: the same formulas in float64 on the fp32-rounded K and M promoted to double, with the bound
``8 * 2^-24 * (sum_c |M_rc p_c| + |M_r3|)`` per coordinate (seven roundings: three for x / y, one product and
three sums, plus second-order terms).
"""
import numpy as np

U = 2.0 ** -24


def keep_mask(depth, valid, step, trunc):
    d = depth[:, ::step, ::step]
    with np.errstate(invalid="ignore"):
        keep = (d > np.float32(0)) & (d < np.float32(trunc))
    if valid is not None:
        keep &= valid[:, ::step, ::step] != 0
    return d, keep


def frame_offsets(keep):
    counts = keep.reshape(keep.shape[0], -1).sum(1).astype(np.int64)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def cloud_f32(depth, valid, rgb, K, M, step, trunc):
    """depth [F, H, W] f32, valid [F, H, W] or None, rgb [F, H, W, 3] u8 or None, K [F, 4] f32, M [F, 3, 4] f32
    or None -> (points [N, 3] f32, colors [N, 3] u8 or None, frame_offsets [F + 1] i64)."""
    F, H, W = depth.shape
    z, keep = keep_mask(depth, valid, step, trunc)
    jj = np.arange(0, W, step).astype(np.float32)[None, None, :]
    ii = np.arange(0, H, step).astype(np.float32)[None, :, None]
    fx, fy, cx, cy = (K[:, c].astype(np.float32).reshape(F, 1, 1) for c in range(4))
    with np.errstate(all="ignore"):
        x = (jj - cx) * z / fx
        y = (ii - cy) * z / fy
        p = [x, y, z]
        if M is not None:
            m = M.astype(np.float32).reshape(F, 3, 4, 1, 1)
            p = [((m[:, r, 0] * x + m[:, r, 1] * y) + m[:, r, 2] * z) + m[:, r, 3] for r in range(3)]
    pts = np.stack(p, -1)
    assert pts.dtype == np.float32
    colors = None if rgb is None else rgb[:, ::step, ::step][keep]
    return pts[keep], colors, frame_offsets(keep)


def cloud_f64(depth, valid, K, M, step, trunc):
    """-> (points [N, 3] f64, bound [N, 3] f64) for the candidates ``cloud_f32`` keeps."""
    F, H, W = depth.shape
    z32, keep = keep_mask(depth, valid, step, trunc)
    z = z32.astype(np.float64)
    jj = np.arange(0, W, step).astype(np.float64)[None, None, :]
    ii = np.arange(0, H, step).astype(np.float64)[None, :, None]
    fx, fy, cx, cy = (K[:, c].astype(np.float64).reshape(F, 1, 1) for c in range(4))
    with np.errstate(all="ignore"):
        x = (jj - cx) * z / fx
        y = (ii - cy) * z / fy
        z = np.broadcast_to(z, x.shape)
        if M is None:
            m = np.broadcast_to(np.eye(4)[:3], (F, 3, 4)).reshape(F, 3, 4, 1, 1)
        else:
            m = M.astype(np.float64).reshape(F, 3, 4, 1, 1)
        p = [m[:, r, 0] * x + m[:, r, 1] * y + m[:, r, 2] * z + m[:, r, 3] for r in range(3)]
        mag = [np.abs(m[:, r, 0] * x) + np.abs(m[:, r, 1] * y) + np.abs(m[:, r, 2] * z) + np.abs(m[:, r, 3])
               for r in range(3)]
    pts = np.stack(p, -1)[keep]
    bound = 8 * U * np.stack(mag, -1)[keep]
    return pts, bound


def packed(points, colors):
    """The body of the binary PLY: 12- or 15-byte records."""
    body = np.ascontiguousarray(points.astype("<f4")).view(np.uint8).reshape(-1, 12)
    if colors is not None:
        body = np.concatenate([body, colors], 1)
    return body.reshape(-1)
