"""Time BEVFormer's encoder attention (paddle3d_amd/bevformer.py, csrc/bevformer.hip) at the tiny config (50 x 50 BEV,
6 cameras, one 15 x 25 level, E = 256, M = 8, P = 8 / 4, 3 layers) and at the base shape (200 x 200 BEV, 4 levels,
6 layers), on three paths over the same inputs and weights:

  fused      the modules with fused=True: pd3_bevformer_point_sampling once, pd3_bevformer_sca / _tsa once per layer
  unfused    fused=False: every camera over all Q queries through ms_deform_attn, masked and summed; no host sync
  rebatch    THE YARDSTICK: the reference's algorithm written in torch around ms_deform_attn, with its host syncs
             (SpatialCrossAttention.forward: a nonzero() per camera, max_len read back, zero-filled rebatch, the two
             Linears on cams x max_len rows, softmax, sampling_locations, the op, an index_add per camera, count,
             divide; point_sampling as torch elementwise ops and a matmul; the prev_bev .any() read back).  TSA on this
             path is the reference's two transposes around the op, which is the unfused path.

Reported per shape: SCA and TSA module time per layer (Linears and output_proj included) and the whole encoder
forward, in us, as the median of `--repeats` windows of `--iters` calls with the smallest and largest window; the paths
alternate inside each repeat.  A window is a host clock around calls that end in a device synchronise (the yardstick
stalls the host, so device events alone would flatter it).  Also printed: the largest difference between the paths'
encoder outputs, and the bytes per layer of the tensors the fused path does not form.

    python tools/prof/prof_bevformer_encoder.py [--iters 20] [--repeats 5] [--shapes tiny base]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from paddle3d_amd import bevformer as bf  # noqa: E402

PC_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
SHAPES = {
    "tiny": dict(bev=(50, 50), cams=6, levels=[[15, 25]], E=256, M=8, P=8, tsa_P=4, D=4, layers=3, img=(480, 800),
                 ffn=512),
    "base": dict(bev=(200, 200), cams=6, levels=[[116, 200], [58, 100], [29, 50], [15, 25]], E=256, M=8, P=8, tsa_P=4,
                 D=4, layers=6, img=(928, 1600), ffn=512),
}
ORDER = ("self_attn", "norm", "cross_attn", "norm", "ffn", "norm")


def calibrations(cams, img, rng):
    """[1, cams, 4, 4]: a ring of pinhole cameras 1.5 m above the origin, 70 degrees of horizontal view each."""
    h, w = img
    f = w / 2 / np.tan(np.radians(35.0))
    K = np.array([[f, 0, w / 2, 0], [0, f, h / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
    out = np.zeros((1, cams, 4, 4))
    for i in range(cams):
        yaw = 2 * np.pi * i / cams + rng.uniform(-0.05, 0.05)
        R = np.stack([[np.sin(yaw), -np.cos(yaw), 0.0], [0.0, 0.0, -1.0], [np.cos(yaw), np.sin(yaw), 0.0]])
        E = np.eye(4)
        E[:3, :3], E[:3, 3] = R, -R @ np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), 1.5])
        out[0, i] = K @ E
    return out.astype(np.float32)


def encoder_cfg(c):
    tsa = dict(type_name="TemporalSelfAttention", embed_dims=c["E"], num_heads=c["M"], num_levels=1, num_points=c["tsa_P"])
    sca = dict(type_name="SpatialCrossAttention", embed_dims=c["E"], num_cams=c["cams"], pc_range=PC_RANGE,
               deformable_attention=dict(type_name="MSDeformableAttention3D", embed_dims=c["E"], num_heads=c["M"],
                                         num_points=c["P"], num_levels=len(c["levels"])))
    layer = dict(type_name="BEVFormerLayer", attn_cfgs=[tsa, sca], feedforward_channels=c["ffn"], operation_order=ORDER)
    return dict(transformerlayers=layer, num_layers=c["layers"], point_cloud_range=PC_RANGE, num_points_in_pillar=c["D"])


def make_encoder(c, fused, device, seed=0):
    torch.manual_seed(seed)
    enc = bf.BEVFormerEncoder(**encoder_cfg(c), fused=fused)
    with torch.no_grad():
        for name, p in enc.named_parameters():  # the reference's zero-initialised query Linears would sample one point
            if "sampling_offsets" in name or "attention_weights" in name:
                p.normal_(0, 0.5 if name.endswith("bias") else 0.05)
    return enc.eval().to(device)


def make_inputs(c, device, seed=1):
    rng = np.random.default_rng(seed)
    Q, S = c["bev"][0] * c["bev"][1], sum(h * w for h, w in c["levels"])
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(device)  # noqa: E731
    sh = torch.tensor(c["levels"], dtype=torch.int64)
    lsi = torch.cat([sh.new_zeros(1), (sh[:, 0] * sh[:, 1]).cumsum(0)[:-1]])
    mats = torch.from_numpy(calibrations(c["cams"], c["img"], rng)).to(device)
    feats = t(c["cams"], S, 1, c["E"])
    kw = dict(bev_h=c["bev"][0], bev_w=c["bev"][1], bev_pos=t(Q, 1, c["E"]), spatial_shapes=sh.to(device),
              level_start_index=lsi.to(device), prev_bev=t(Q, 1, c["E"]),
              shift=torch.from_numpy(rng.uniform(-0.01, 0.01, (1, 2)).astype(np.float32)).to(device),
              img_metas=[dict(lidar2img=mats[0], img_shape=[(*c["img"], 3)] * c["cams"])])
    return (t(Q, 1, c["E"]), feats, feats), kw


# ---- the yardstick: the reference's algorithm in torch around the existing op ------------------------------------------


def rebatch_point_sampling(ref_3d, pc_range, lidar2img, img):
    """encoders.py:120-176 as torch operators: ref_3d [bs, D, Q, 3] -> (reference_points_cam, bev_mask)."""
    pc = ref_3d.new_tensor(pc_range)
    pts = ref_3d * (pc[3:] - pc[:3]) + pc[:3]
    pts = torch.cat([pts, torch.ones_like(pts[..., :1])], -1).permute(1, 0, 2, 3)  # [D, B, Q, 4]
    D, B, Q = pts.shape[:3]
    cams = lidar2img.shape[1]
    pts = pts.reshape(D, B, 1, Q, 4).repeat(1, 1, cams, 1, 1).unsqueeze(-1)
    mats = lidar2img.reshape(1, B, cams, 1, 4, 4).repeat(D, 1, 1, Q, 1, 1)
    cam = torch.matmul(mats, pts).squeeze(-1)
    eps = 1e-5
    mask = cam[..., 2:3] > eps
    cam = cam[..., 0:2] / torch.maximum(cam[..., 2:3], torch.ones_like(cam[..., 2:3]) * eps)
    cam[..., 0] /= img[1]
    cam[..., 1] /= img[0]
    mask = mask & (cam[..., 1:2] > 0.0) & (cam[..., 1:2] < 1.0) & (cam[..., 0:1] < 1.0) & (cam[..., 0:1] > 0.0)
    return cam.permute(2, 1, 3, 0, 4), mask.permute(2, 1, 3, 0, 4).squeeze(-1)


def device_reference_points(H, W, Z, D, bs, dev):
    """encoders.py:69-117 with device operators, as the reference builds them at every forward."""
    lin = lambda a, b, n: torch.linspace(a, b, n, dtype=torch.float32, device=dev)  # noqa: E731
    zs = lin(0.5, Z - 0.5, D).reshape(-1, 1, 1).expand(D, H, W) / Z
    xs = lin(0.5, W - 0.5, W).reshape(1, 1, W).expand(D, H, W) / W
    ys = lin(0.5, H - 0.5, H).reshape(1, H, 1).expand(D, H, W) / H
    ref_3d = torch.stack((xs, ys, zs), -1).permute(0, 3, 1, 2).flatten(2).permute(0, 2, 1)[None].repeat(bs, 1, 1, 1)
    ref_y, ref_x = torch.meshgrid(lin(0.5, H - 0.5, H), lin(0.5, W - 0.5, W), indexing="ij")
    ref_2d = torch.stack((ref_x.reshape(-1)[None] / W, ref_y.reshape(-1)[None] / H), -1)
    return ref_3d, ref_2d.repeat(bs, 1, 1).unsqueeze(2)


def rebatch_sca(m, query, value, reference_points_cam, bev_mask, spatial_shapes, level_start_index):
    """spatial_cross_attention.py:128-212 on the module's weights (query_pos is None, batch of one)."""
    att = m.deformable_attention
    bs, Q, E = query.shape
    cams, S = value.shape[:2]
    D = reference_points_cam.shape[3]
    slots = torch.zeros_like(query)
    indexes = [mask_per_img[0].sum(-1).nonzero().squeeze(-1) for mask_per_img in bev_mask]
    max_len = int(bev_mask.any(-1).sum(-1).max().cpu().numpy())
    queries_rebatch = query.new_zeros([bs, cams, max_len, E])
    ref_rebatch = reference_points_cam.new_zeros([bs, cams, max_len, D, 2])
    for j in range(bs):
        for i, ref_per_img in enumerate(reference_points_cam):
            idx = indexes[i]
            queries_rebatch[j, i, :len(idx)] = query[j].index_select(0, idx)
            ref_rebatch[j, i, :len(idx)] = ref_per_img[j].index_select(0, idx)
    v = value.permute(2, 0, 1, 3).reshape(bs * cams, S, E)
    queries = att(query=queries_rebatch.reshape(bs * cams, max_len, E), key=v, value=v,
                  reference_points=ref_rebatch.reshape(bs * cams, max_len, D, 2), spatial_shapes=spatial_shapes,
                  level_start_index=level_start_index).reshape(bs, cams, max_len, E)
    for j in range(bs):
        for i, idx in enumerate(indexes):
            slots[j] = slots[j].index_add(0, idx, queries[j, i, :len(idx)])
    count = (bev_mask.sum(-1) > 0).permute(1, 2, 0).sum(-1).clamp(min=1.0)
    slots = slots / count[..., None]
    return m.output_proj(slots) + query


class RebatchSCA(torch.nn.Module):
    """Stands in for a layer's SpatialCrossAttention on the yardstick path (shares its weights)."""

    def __init__(self, m):
        super().__init__()
        self.m, self.embed_dims = m, m.embed_dims

    def forward(self, query, key, value, residual=None, reference_points_cam=None, bev_mask=None, spatial_shapes=None,
                level_start_index=None, **kwargs):
        return rebatch_sca(self.m, query, value, reference_points_cam, bev_mask, spatial_shapes, level_start_index)


def rebatch_encoder(enc, bev_query, key, value, bev_h=None, bev_w=None, bev_pos=None, spatial_shapes=None,
                    level_start_index=None, prev_bev=None, shift=0.0, img_metas=None):
    """encoders.py:211-302 over an unfused encoder whose SCA modules are RebatchSCA."""
    bs, dev = bev_query.shape[1], bev_query.device
    z = enc.point_cloud_range[5] - enc.point_cloud_range[2]
    ref_3d, ref_2d = device_reference_points(bev_h, bev_w, z, enc.num_points_in_pillar, bs, dev)
    lidar2img = torch.stack([meta["lidar2img"] for meta in img_metas])
    ref_cam, mask = rebatch_point_sampling(ref_3d, enc.point_cloud_range, lidar2img, img_metas[0]["img_shape"][0])
    ref_2d += shift[:, None, None, :]
    bev_query, bev_pos, prev_bev = bev_query.permute(1, 0, 2), bev_pos.permute(1, 0, 2), prev_bev.permute(1, 0, 2)
    valid = int(prev_bev.bool().any())  # the reference's read-back
    prev_bev = prev_bev * valid + bev_query * (1 - valid)
    prev_bev = torch.stack([prev_bev, bev_query], 1).reshape(bs * 2, bev_h * bev_w, -1)
    hybrid = torch.stack([ref_2d, ref_2d], 1).reshape(bs * 2, bev_h * bev_w, 1, 2)
    for layer in enc.layers:
        bev_query = layer(bev_query, key, value, bev_pos=bev_pos, ref_2d=hybrid, ref_3d=ref_3d, bev_h=bev_h, bev_w=bev_w,
                          spatial_shapes=spatial_shapes, level_start_index=level_start_index,
                          reference_points_cam=ref_cam, bev_mask=mask, prev_bev=prev_bev)
    return bev_query


# ---- timing ------------------------------------------------------------------------------------------------------------


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
        for _ in range(3):
            fn()
    rows = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            rows[k].append(window(fn, iters))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in rows.items()}


def show(title, res):
    base = res["rebatch"][0]
    for k, (med, lo, hi) in res.items():
        print(f"  {title:8s} {k:8s} {med:10.1f} us  [{lo:.1f} .. {hi:.1f}]  rebatch / this = {base / med:5.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prof_bevformer_encoder: needs the GPU (a CPU run says nothing about these times)")
    dev = torch.device("cuda", 0)
    for name in a.shapes:
        c = SHAPES[name]
        Q, L = c["bev"][0] * c["bev"][1], len(c["levels"])
        args, kw = make_inputs(c, dev)
        encs = {"fused": make_encoder(c, True, dev), "unfused": make_encoder(c, False, dev),
                "rebatch": make_encoder(c, False, dev)}
        for layer in encs["rebatch"].layers:
            layer.attentions[1] = RebatchSCA(layer.attentions[1])
        with torch.no_grad():
            outs = {"fused": encs["fused"](*args, **kw), "unfused": encs["unfused"](*args, **kw),
                    "rebatch": rebatch_encoder(encs["rebatch"], *args, **kw)}
            diff = {k: float((outs[k] - outs["rebatch"]).abs().max()) for k in ("fused", "unfused")}
            e = encs["fused"]
            ref_3d, ref_2d = e._reference_points(*c["bev"], 1, torch.float32, dev)
            ref_cam, mask, bits, count = e.point_sampling(ref_3d, PC_RANGE, kw["img_metas"], with_hits=True)
            hits = count.float()
            q = args[0].permute(1, 0, 2).contiguous()
            pos = kw["bev_pos"].permute(1, 0, 2).contiguous()
            queue = torch.stack([kw["prev_bev"].permute(1, 0, 2), q], 1).reshape(2, Q, c["E"])
            hybrid = torch.stack([ref_2d, ref_2d], 1).reshape(2, Q, 1, 2)
            bev_levels = bf._bev_levels(*c["bev"], dev)
            sca_kw = dict(reference_points_cam=ref_cam, bev_mask=mask, spatial_shapes=kw["spatial_shapes"],
                          level_start_index=kw["level_start_index"])
            tsa_kw = dict(query_pos=pos, reference_points=hybrid, spatial_shapes=bev_levels[0],
                          level_start_index=bev_levels[1])
            sca = {k: (lambda m=encs[k].layers[0].attentions[1], extra=(dict(hit_bits=bits) if k == "fused" else {}):
                       m(q, args[1], args[2], **sca_kw, **extra)) for k in encs}
            tsa = {k: (lambda m=encs[k].layers[0].attentions[0]: m(q, queue, queue, None, **tsa_kw)) for k in encs}
            whole = {"fused": lambda: encs["fused"](*args, **kw), "unfused": lambda: encs["unfused"](*args, **kw),
                     "rebatch": lambda: rebatch_encoder(encs["rebatch"], *args, **kw)}
            max_len = int(mask.any(-1).sum(-1).max())
            print(f"{name}: BEV {c['bev']}, Q {Q}, {c['cams']} cameras, levels {c['levels']}, E {c['E']}, M {c['M']}, "
                  f"P {c['P']} / {c['tsa_P']}, D {c['D']}, {c['layers']} layers; queries seen by >= 1 camera "
                  f"{float((hits > 0).float().mean()):.3f}, mean hits {float(hits.mean()):.2f}, max_len {max_len}")
            print(f"  encoder output: max |fused - rebatch| = {diff['fused']:.3g}, max |unfused - rebatch| = "
                  f"{diff['unfused']:.3g} (|max| {float(outs['rebatch'].abs().max()):.3g})")
            show("SCA", measure(sca, a.iters, a.repeats))
            show("TSA", measure(tsa, a.iters, a.repeats))
            show("encoder", measure(whole, max(a.iters // 4, 3), a.repeats))
        rows = c["cams"] * max_len
        mb = lambda n: f"{n * 4 / 1e6:.1f} MB"  # noqa: E731
        print(f"  per layer, not formed by the fused path: rebatched queries {mb(rows * c['E'])}, rebatched reference "
              f"points {mb(rows * c['D'] * 2)}, offsets on the rebatched rows {mb(rows * c['M'] * L * c['P'] * 2)} "
              f"(on the Q BEV queries, read by the kernel: {mb(Q * c['M'] * L * c['P'] * 2)}), sampling_locations "
              f"{mb(rows * c['M'] * L * c['P'] * 2)}, attention weights {mb(rows * c['M'] * L * c['P'])}, per-camera "
              f"outputs {mb(rows * c['E'])}; TSA's transposed offsets and locations {mb(2 * 2 * Q * c['M'] * c['tsa_P'] * 2)}")
        del encs, outs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
