"""Golden fixtures for the ViT-B encoder variant, generated from the REFERENCE (container only).

``DINOv2("vitb")`` is ``vit_base``: embed dim 768, 12 blocks, 12 heads, the Mlp FFN.  No checkpoint of
Video-Depth-Anything exists for it and the reference's own ``forward`` has no tap list for it, so the instance gets
``intermediate_layer_idx["vitb"] = [2, 5, 8, 11]``, the Depth-Anything-V2 taps DESIGN.md cites, and the variant is pinned
the way ViT-g is: by the reference's modules on the synthetic weight recipe, here at full depth.  Writes

    state_dict_keys_vitb.json   the (key, shape) pairs of the reference's
                                VideoDepthAnything(encoder="vitb", features=128, out_channels=[96, 192, 384, 768])
    vitb_t4_70x98.npz           x fp16, depth fp32, tap_stats, meta (the keys helpers.load_golden reads): that model
                                through the reference's own forward

with the import shims of ``make_golden.py``; only inputs and outputs are stored.

    python tests/golden/make_vitb_golden.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

FULL = dict(encoder="vitb", features=128, out_channels=[96, 192, 384, 768])
TAPS = [2, 5, 8, 11]
NAME, B, T, H, W = "vitb_t4_70x98", 1, 4, 70, 98


def main():
    import make_golden as MG
    import vda_amd.weights as Wt
    VDA = MG.import_reference()
    torch.set_num_threads(8)
    torch.manual_seed(0)
    m = VDA(**FULL).eval()
    m.intermediate_layer_idx["vitb"] = TAPS
    keys = [(k, list(v.shape)) for k, v in m.state_dict().items()]
    with open(os.path.join(HERE, "state_dict_keys_vitb.json"), "w") as f:
        json.dump(keys, f)
    m.load_state_dict(Wt.synthetic_state_dict((k, tuple(s)) for k, s in keys), strict=True)
    print("vitb keys", len(keys), sum(p.numel() for p in m.parameters()) / 1e6, "M parameters")
    g = torch.Generator().manual_seed(1234 + T * 7 + H)
    x = torch.randn(B, T, 3, H, W, generator=g).half().float()
    taps = []
    with torch.no_grad():
        for f, _cls in m.pretrained.get_intermediate_layers(x.flatten(0, 1), TAPS, return_class_token=True):
            taps.append([float(f.mean()), float(f.std()), float(f.abs().mean())])
        d = m(x)
    np.savez_compressed(os.path.join(HERE, NAME + ".npz"), x=x.half().numpy(), depth=d.numpy().astype(np.float32),
                        tap_stats=np.array(taps, dtype=np.float64),
                        meta=np.array(json.dumps(dict(encoder="vitb", taps=TAPS, B=B, T=T, H=H, W=W, skip_tmp_block=False))))
    print(NAME, tuple(d.shape), float(d.mean()), float(d.min()), float(d.max()))


if __name__ == "__main__":
    main()
