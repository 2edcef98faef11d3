"""Time BEVFormer's decoder, head and NMS-free decode (paddle3d_amd/bevformer_head.py, csrc/bevformer_decoder.hip) at the
tiny config's shape: B = 1, 900 object queries, a 50 x 50 BEV map, E = 256, 8 heads, P = 4, 6 layers, 10 classes,
max_num = 300, on two paths over the same inputs and weights on the same commit:

  fused      every kernel asked for (the self-attention's in its own cfg, where it is opt-in): pd3_mha_forward and
             pd3_bevformer_dec_ca once per layer, pd3_nms_free_decode once per forward
  unfused    fused=False: the [8, 900, 900] score tensor, softmax and two matmuls in torch; softmax and sampling
             locations in torch around ms_deform_attn; the decode as torch sort / gather / where (no host sync either)

and pd3_mha_forward alone against the torch formulation (scale, matmul, softmax, matmul on the projected q, k, v).

Reported in us as the median of `--repeats` windows of `--iters` calls with the smallest and largest window; the two
paths alternate inside each repeat, after a warm-up of each.  A window is a host clock around calls that end in a
device synchronise.  Also printed: the largest difference between the paths' outputs, and what is derived from the
shape rather than measured (the kernel's bytes, MFMA count and dependent chain, the score tensor it does not form).

    python tools/prof/bevformer_decoder.py [--iters 50] [--repeats 7]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from paddle3d_amd import bevformer_head as bh  # noqa: E402
from paddle3d_amd.ops import bevformer_decoder as ops  # noqa: E402

PC_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
POST_RANGE = [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]
SHAPE = dict(B=1, Q=900, bev=(50, 50), E=256, M=8, P=4, layers=6, K=10, max_num=300, ffn=512, code=10)
ORDER = ("self_attn", "norm", "cross_attn", "norm", "ffn", "norm")


def head_cfg(c, fused):
    attn = [dict(type_name="MultiheadAttention", embed_dims=c["E"], num_heads=c["M"], dropout=0.1, fused=fused),
            dict(type_name="CustomMSDeformableAttention", embed_dims=c["E"], num_heads=c["M"], num_levels=1,
                 num_points=c["P"])]
    layer = dict(type_name="DetrTransformerDecoderLayer", attn_cfgs=attn, feedforward_channels=c["ffn"], ffn_dropout=0.1,
                 operation_order=ORDER)
    decoder = dict(type_name="DetectionTransformerDecoder", num_layers=c["layers"], return_intermediate=True,
                   transformerlayers=layer)
    coder = dict(type_name="NMSFreeCoder", point_cloud_range=PC_RANGE, post_center_range=POST_RANGE, max_num=c["max_num"],
                 num_classes=c["K"])
    return dict(num_classes=c["K"], in_channels=c["E"], num_query=c["Q"], with_box_refine=True, bev_h=c["bev"][0],
                bev_w=c["bev"][1], code_size=c["code"], bbox_coder=coder, fused=fused,
                transformer=dict(type_name="PerceptionTransformer", embed_dims=c["E"], decoder=decoder))


def make_head(c, fused, device, seed=0):
    torch.manual_seed(seed)
    head = bh.BEVFormerHead(**head_cfg(c, fused))
    with torch.no_grad():
        head.query_embedding.weight.normal_(0, 1)
    return head.eval().to(device)


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def measure(fns, iters, repeats):
    """{name: (median, min, max)} us per call; the paths alternate inside each repeat, after a warm-up of each."""
    for fn in fns.values():
        for _ in range(5):
            fn()
    rows = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            rows[k].append(window(fn, iters))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in rows.items()}


def show(title, res, base):
    for k, (med, lo, hi) in res.items():
        print(f"  {title:22s} {k:8s} {med:10.1f} us  [{lo:.1f} .. {hi:.1f}]  {base} / this = {res[base][0] / med:5.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bevformer_decoder: needs the GPU (a CPU run says nothing about these times)")
    dev = torch.device("cuda", 0)
    c = SHAPE
    B, Q, E, M = c["B"], c["Q"], c["E"], c["M"]
    d, S = E // M, c["bev"][0] * c["bev"][1]
    heads = {"fused": make_head(c, True, dev), "unfused": make_head(c, False, dev)}
    bev = torch.randn(B, S, E, device=dev, generator=torch.Generator(dev).manual_seed(1))
    with torch.no_grad():
        outs = {k: h.forward_from_bev(bev) for k, h in heads.items()}
        dets = {k: h.get_bboxes(outs[k]) for k, h in heads.items()}
        for name in ("all_cls_scores", "all_bbox_preds"):
            print(f"{name}: max |fused - unfused| = {float((outs['fused'][name] - outs['unfused'][name]).abs().max()):.3g} "
                  f"(|max| {float(outs['unfused'][name].abs().max()):.3g})")
        print("decode: counts", dets["fused"][3].tolist(), dets["unfused"][3].tolist(), "labels equal",
              bool(torch.equal(dets["fused"][2], dets["unfused"][2])))
        whole = {k: (lambda h=h: h.get_bboxes(h.forward_from_bev(bev))) for k, h in heads.items()}
        show("decoder + head + decode", measure(whole, a.iters, a.repeats), "unfused")
        coder = {k: (lambda h=h, o=outs[k]: h.get_bboxes(o)) for k, h in heads.items()}
        show("decode alone", measure(coder, 4 * a.iters, a.repeats), "unfused")
        q, k, v = (torch.randn(B, Q, E, device=dev) for _ in range(3))
        core = heads["unfused"].transformer.decoder.layers[0].attentions[0].core
        got, want = ops.multihead_attention(q, k, v, M), core(q, k, v)
        print(f"pd3_mha_forward: max |kernel - torch| = {float((got - want).abs().max()):.3g}")
        mha = {"kernel": lambda: ops.multihead_attention(q, k, v, M), "torch": lambda: core(q, k, v)}
        show("attention core alone", measure(mha, 4 * a.iters, a.repeats), "torch")
    tiles, nt = -(-Q // 16), -(-Q // 16)
    mfma = B * M * tiles * (nt * (d // 4) + (d // 16) * nt * 4)
    print(f"  derived, per layer: q, k, v read and out written {4 * B * Q * E * 4 / 1e6:.2f} MB; score tensor not formed "
          f"{B * M * Q * Q * 4 / 1e6:.1f} MB (x about 3 passes in torch); {mfma} v_mfma_f32_16x16x4_f32 over "
          f"{B * M * tiles} workgroups = {mfma * 32} issue cycles in all, per workgroup {nt * (d // 4)} (scores, in "
          f"independent pairs) + {(d // 16) * nt * 4} (P V); the P V chain of one wave is {nt * 4} dependent MFMAs")


if __name__ == "__main__":
    main()
