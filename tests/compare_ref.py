"""The comparison canvas as a plain numpy composition, written from the contract in include/vda.h: what
``TorchCompare`` (tests/test_compare.py) and ``LibCompare`` (tests/test_gpu_compare.py) must reproduce bit for
bit.  Per tile ``np.abs`` / slicing, the ``colorize_depths`` index expression with an explicit range (and the
stated clamp where numpy's cast is undefined), ``matplotlib.colormaps[...]``, tile placement with slicing, then
``video_io._rgb_to_yuv`` and ``_subsample_420`` on the whole canvas."""
import numpy as np
import torch

from vda_amd import compare as CMP
from vda_amd import video_io as VIO


def scene(N, H, W, offsets=(0,), seed=0, with_rgb=True, with_valid=False):
    """gt [N, H, W] metres, per method an aligned metric depth [N - o, H, W] (some pixels far off, one NaN),
    rgb, valid."""
    g = np.random.default_rng(seed)
    gt = g.uniform(1., 60., (N, H, W)).astype(np.float32)
    preds = []
    for o in offsets:
        p = (gt[o:] * g.uniform(0.7, 1.4, (N - o, H, W))).astype(np.float32)
        p.reshape(-1)[g.integers(0, p.size)] = np.float32(80.)
        if p.size > 8:
            p.reshape(-1)[g.integers(0, p.size)] = np.nan
        preds.append(p)
    rgb = g.integers(0, 256, (N, H, W, 3), dtype=np.uint8) if with_rgb else None
    valid = (g.random((N, H, W)) < 0.7) if with_valid else None
    return gt, preds, rgb, valid


def error_map(gt, pred, valid):
    e = np.abs(gt - pred)
    return e if valid is None else np.where(valid, e, np.float32(0.)).astype(np.float32)


def ranges(gt, preds, valid):
    """(depth range over the predictions, error range over the maps as displayed); NaNs skipped."""
    N = gt.shape[0]
    errs = [error_map(gt[N - len(p):], p, None if valid is None else valid[N - len(p):]) for p in preds]
    dr = np.array([min(np.nanmin(p) for p in preds), max(np.nanmax(p) for p in preds)], dtype=np.float32)
    er = np.array([min(np.nanmin(e) for e in errs), max(np.nanmax(e) for e in errs)], dtype=np.float32)
    return dr, er


def index(v, rng):
    """colorize_depths' ``((d - min) / (max - min) * 255).astype(np.uint8)`` with an explicit range; NaN and
    x <= 0 give 0, x >= 255 gives 255 (numpy's cast is undefined there)."""
    lo, hi = np.float32(rng[0]), np.float32(rng[1])
    with np.errstate(invalid="ignore", divide="ignore"):
        x = (v.astype(np.float32) - lo) / (hi - lo) * np.float32(255)
        x = np.where(x >= 255, np.float32(255), np.where(x > 0, x, np.float32(0)))
    return x.astype(np.uint8)


def table(name):
    import matplotlib
    return (matplotlib.colormaps[name](np.arange(256, dtype=np.uint8))[..., :3] * 255).astype(np.uint8)


def stability(v, o, N, t, xstar, W):
    """The tile of the [H, N] stability image at output frame t: column c = v[c - o, :, xstar] for o <= c <= t,
    0.0 elsewhere, stretched to W columns by c = (px * N) // W."""
    img = np.zeros((v.shape[1], N), dtype=np.float32)
    for c in range(o, min(t, N - 1) + 1):
        img[:, c] = v[c - o, :, xstar]
    return img[:, (np.arange(W, dtype=np.int64) * N) // W]


def canvas_rgb(gt, preds, rgb, valid, dr, er, xstar):
    """[N, (1 + M) H, 3 W, 3] uint8 RGB."""
    N, H, W = gt.shape
    spectral, rdylgn = table("Spectral"), table("RdYlGn")
    out = np.zeros((N, (1 + len(preds)) * H, 3 * W, 3), dtype=np.uint8)
    zero = np.zeros((H, W), dtype=np.float32)
    for t in range(N):
        if rgb is not None:
            out[t, :H, :W] = rgb[t]
        out[t, :H, W:2 * W] = spectral[index(gt[t], dr)]
        out[t, :H, 2 * W:] = spectral[index(stability(gt, 0, N, t, xstar, W), dr)]
        for i, p in enumerate(preds):
            o = N - len(p)
            r = slice((1 + i) * H, (2 + i) * H)
            live = t >= o
            e = error_map(gt[t], p[t - o], None if valid is None else valid[t]) if live else zero
            out[t, r, :W] = rdylgn[index(e, er)]
            out[t, r, W:2 * W] = spectral[index(p[t - o] if live else zero, dr)]
            out[t, r, 2 * W:] = spectral[index(stability(p, o, N, t, xstar, W), dr)]
    return out


def to_layout(canvas, layout):
    """RGB canvas frames -> the bytes of ``layout``, as ``write_y4m`` makes them for the planar ones."""
    if layout == "hwc":
        return canvas
    frames = []
    for f in canvas:
        y, u, v = VIO._rgb_to_yuv(f)
        if layout == "planar444":
            frames.append(np.stack([y, u, v]))
        else:
            frames.append(np.concatenate([y.reshape(-1), VIO._subsample_420(u).reshape(-1),
                                          VIO._subsample_420(v).reshape(-1)]))
    return np.stack(frames)


def result_of(gt, preds, rgb, valid, dr, er, stability_line, device, backend):
    """A ``CompareResult`` over already aligned predictions (no fit)."""
    dev = torch.device(device)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    N = gt.shape[0]
    methods = {f"m{i}": CMP.MethodResult(scale=1., shift=0., abs_error=0., mse=0., frame_mse=np.zeros(len(p)),
                                         offset=N - len(p), aligned=t(p)) for i, p in enumerate(preds)}
    v = None if valid is None else t(valid).view(torch.uint8)
    return CMP.CompareResult(methods=methods, depth_range=t(dr), error_range=t(er), gt=t(gt), rgb=t(rgb), valid=v,
                             stability_line=stability_line, backend=backend)


def frames_of(result, layout, chunk=32):
    return np.concatenate([b.copy() for b in CMP.compose_frames(result, layout, chunk)])


def y4m_payloads(path, nbytes):
    """The frame payloads of a y4m file: [n, nbytes] uint8."""
    data = open(path, "rb").read()
    body = data[data.index(b"\n") + 1:]
    rec = len(b"FRAME\n") + nbytes
    assert len(body) % rec == 0
    return np.stack([np.frombuffer(body, np.uint8, nbytes, i * rec + 6) for i in range(len(body) // rec)])
