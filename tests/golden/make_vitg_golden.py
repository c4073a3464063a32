"""Golden fixtures for the ViT-g encoder variant, generated from the REFERENCE (container only).

``DINOv2("vitg")`` (dinov2.py:398-415) is ``vit_giant2`` with ``ffn_layer="swiglufused"``: embed dim 1536, 40
blocks, 24 heads, SwiGLUFFNFused (``mlp.w12`` [8192, 1536], ``mlp.w3`` [1536, 4096]).  No checkpoint of
Video-Depth-Anything exists for it and the reference's own ``forward`` has no tap list for it, so the variant is
pinned the way pe='rope' is: by the reference's modules on the synthetic weight recipe.  Writes

    state_dict_keys_vitg.json   the (key, shape) pairs of the reference's full model
                                VideoDepthAnything(encoder="vitg", features=384, out_channels=[1536] * 4)
    vitg_d4_t4_70x98.npz        x fp16, depth fp32, meta: a reduced-depth model (4 blocks, taps [0, 1, 2, 3]) built
                                from the reference's DinoVisionTransformer and DPTHeadTemporal with the arguments
                                DINOv2("vitg") passes, and run through the reference's forward

with the import shims of ``make_golden.py``; only inputs and outputs are stored.

    python tests/golden/make_vitg_golden.py
"""
import json
import os
import sys
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

FULL = dict(encoder="vitg", features=384, out_channels=[1536] * 4)
D4_DEPTH, D4_TAPS = 4, [0, 1, 2, 3]


def main():
    import make_golden as MG
    import vda_amd.weights as W
    VDA = MG.import_reference()
    from video_depth_anything import dinov2 as RD
    from video_depth_anything.dpt_temporal import DPTHeadTemporal
    torch.set_num_threads(8)
    torch.manual_seed(0)

    full = VDA(**FULL)  # key names and shapes only (its constructor does not run on the meta device)
    keys = [(k, list(v.shape)) for k, v in full.state_dict().items()]
    with open(os.path.join(HERE, "state_dict_keys_vitg.json"), "w") as f:
        json.dump(keys, f)
    print("vitg keys", len(keys), sum(int(np.prod(s)) for k, s in keys if not k.endswith("pos_encoder.pe")) / 1e9, "G")
    del full

    m = VDA.__new__(VDA)
    torch.nn.Module.__init__(m)
    m.intermediate_layer_idx = {"vitg": D4_TAPS}
    m.encoder = "vitg"
    m.pretrained = RD.DinoVisionTransformer(
        img_size=518, patch_size=14, embed_dim=1536, depth=D4_DEPTH, num_heads=24, mlp_ratio=4,
        block_fn=partial(RD.Block, attn_class=RD.MemEffAttention), init_values=1.0, ffn_layer="swiglufused",
        block_chunks=0, num_register_tokens=0, interpolate_antialias=False, interpolate_offset=0.1)
    m.head = DPTHeadTemporal(1536, 384, False, out_channels=[1536] * 4, use_clstoken=False, num_frames=32, pe="ape")
    m.eval()
    k4 = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    m.load_state_dict(W.synthetic_state_dict(k4), strict=True)
    print("d4 parameters", sum(p.numel() for p in m.parameters()) / 1e6, "M")
    g = torch.Generator().manual_seed(1234 + 4 * 7 + 70)
    x = torch.randn(1, 4, 3, 70, 98, generator=g).half().float()
    with torch.no_grad():
        d = m(x)
    np.savez_compressed(os.path.join(HERE, "vitg_d4_t4_70x98.npz"), x=x.half().numpy(), depth=d.numpy().astype(np.float32),
                        meta=np.array(json.dumps(dict(encoder="vitg", depth=D4_DEPTH, taps=D4_TAPS, B=1, T=4, H=70, W=98,
                                                      skip_tmp_block=False))))
    print("vitg_d4_t4_70x98", tuple(d.shape), float(d.mean()), float(d.min()), float(d.max()))


if __name__ == "__main__":
    main()
