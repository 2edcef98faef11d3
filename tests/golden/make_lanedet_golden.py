"""Golden vectors for BEV-LaneDet's lane head and lane post-processing from the reference's own Python:

    embedding_post, naive_cluster(_nd), collect_*      paddle3d/datasets/apollo/cluster.py (loaded by file path)
    bev_instance2points_with_offset_z                  paddle3d/datasets/apollo/post_process.py (loaded by file path)
    the cubic fit and its 40 samples                   paddle3d/datasets/apollo/apollo_lane_metric.py:376-383 (by line range)
    InstanceEmbeddingOffsetYZ, InstanceEmbedding, LaneHeadResidualInstanceWithOffsetZ, LaneHeadResidualInstance,
    FCTransform_, Residual, BEVLaneDet.__init__        paddle3d/models/detection/bev_lanedet/bev_lanedet.py:50-345, executed
                                                       by line range through tests/golden/paddle_shim.py

    python tests/golden/make_lanedet_golden.py   # needs the reference checkout; writes python_lanedet.npz

What the shim lacks is added here (paddle_shim.py stays as it is): nn.Upsample (nearest), nn.Dropout2D (identity at
inference), Sequential.sublayers, and the loss layers BEVLaneDet's constructor names.

Post-processing cases (POST_CASES: maps of at most 48 x 16, nd 1, 2 and 4, a width that is no multiple of 4): synthetic
lanes from lanedet_numpy.synthetic_lanes; the reference runs once on the float32 maps and once on the same maps cast to
float64.  Head cases (HEAD_CASES: s32 maps of 16 channels, BEV 3 x 2, output sizes (13, 7) and (12, 8)): a `down`
Residual composed as BEVLaneDet composes it, the two FCTransform_, the concatenation and the lane head run in fp32 and
fp64 from the same seeded state; the post-processing then runs on each run's maps.  Stored per case: the inputs, and per
run the canvas, the lanes' ids and row counts, the row points [(x_m, y_m, z)] and the [40, 3] fits.

Conditions, asserted here ("change the seed" otherwise) and stored as `<tag>_margins`: every clustering decision keeps a
margin, |d_best - gap| >= 1e-3 gap and, wherever a pixel joins, d_second - d_best >= 1e-3 gap (scipy's euclidean goes
through BLAS nrm2, which no restatement can promise to match bit for bit); the two runs agree on the canvas; every lane
has at least 4 rows (polyfit is rank deficient below); in head cases |seg - conf| >= 1e-2 at every pixel.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import lanedet_numpy as ln  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "python_lanedet.npz")
APOLLO = os.path.join(REF, "paddle3d/datasets/apollo")
MODEL = os.path.join(REF, "paddle3d/models/detection/bev_lanedet/bev_lanedet.py")

# tag -> (seed, H, W, nd, lanes)
POST_CASES = {"p48x16": (11, 48, 16, 2, 3), "p30x12_nd1": (12, 30, 12, 1, 2), "p40x13": (13, 40, 13, 2, 3),
              "p24x16_nd4": (14, 24, 16, 4, 3)}
# tag -> (seed, B, s32 (c, h, w), s64 channels, bev (c, h, w), output size)
HEAD_CASES = {"h13x7": (21, 2, (16, 4, 6), 32, (16, 3, 2), (13, 7)), "h12x8": (22, 1, (16, 4, 6), 32, (16, 3, 2), (12, 8))}
HEAD_POST = dict(ln.CFG, min_cluster_size=4, max_x=10.0)
MARGIN = 1e-3


def _load_file(name):
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(APOLLO, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def margins(seg, emb, conf, gap):
    """The clustering's decisions replayed in float64: (min |d_best - gap| / gap, min (d_second - d_best) / gap over
    the joining pixels)."""
    ys, xs = np.nonzero(seg >= np.float32(conf))
    cen, num = [], []
    m_gap, m_second = np.inf, np.inf
    for y, x in zip(ys, xs):
        e = emb[:, y, x].astype(np.float64)
        d = np.array([np.sqrt(((e - c) ** 2).sum()) for c in cen])
        if len(d):
            order = np.argsort(d, kind="stable")
            best = d[order[0]]
            m_gap = min(m_gap, abs(best - gap) / gap)
            if best < gap:
                if len(d) > 1:
                    m_second = min(m_second, (d[order[1]] - best) / gap)
                i = order[0]
                cen[i] = (cen[i] * num[i] + e) / (num[i] + 1)
                num[i] += 1
                continue
        cen.append(e)
        num.append(1)
    return float(m_gap), float(m_second)


def reference_post(ref, maps, cfg):
    """The reference's embedding_post, bev_instance2points_with_offset_z and lines :374-383 on one frame's
    [1, 1 + nd + 2, H, W] maps -> canvas, lane ids, row counts, points [sum rows, 3], fits [lanes, 40, 3]."""
    import paddle_shim as ps

    cluster, post, metric = ref
    nd = maps.shape[1] - 3
    prediction = (maps[:, 0:1], maps[:, 1:1 + nd])
    offset_y, z_pred = maps[:, 1 + nd:2 + nd][0][0], maps[:, 2 + nd:3 + nd][0][0]
    canvas, _ = cluster.embedding_post(prediction, cfg["conf"], emb_margin=cfg["emb_margin"],
                                       min_cluster_size=cfg["min_cluster_size"], canvas_color=False)
    mpp = cfg["meter_per_pixel"]
    lines = post.bev_instance2points_with_offset_z(canvas, max_x=cfg["max_x"], meter_per_pixal=(mpp[0], mpp[1]),
                                                   offset_y=offset_y, Z=z_pred)
    ids = [int(c) for c in np.unique(canvas[canvas > 0])]
    kept = [c for c in ids if len(np.unique(np.nonzero(canvas == c)[0])) >= 2]
    assert len(kept) == len(lines)
    fits = []
    for lane in lines:
        ns = dict(np=np, lane=lane, frame_lanes_pred=fits)
        ps.exec_lines(metric, [(376, 383)], ns)
    rows = [len(l[0]) for l in lines]
    pts = [np.stack([l[0], l[1], l[2]], 1) for l in lines]
    return (canvas, np.asarray(kept, np.int32), np.asarray(rows, np.int32),
            np.concatenate(pts) if pts else np.zeros((0, 3)), np.asarray(fits, np.float64).reshape(-1, 40, 3))


def record_post(out, tag, ref, maps32, cfg):
    """Both runs of the post-processing on one frame; asserts the conditions; returns the margins."""
    res = {}
    for name, dt in (("32", np.float32), ("64", np.float64)):
        res[name] = reference_post(ref, maps32.astype(dt), cfg)
    c32, c64 = res["32"], res["64"]
    assert np.array_equal(c32[0], c64[0]), f"{tag}: the two runs draw different canvases: change the seed"
    assert len(c32[2]) and c32[2].min() >= 4, f"{tag}: a lane with fewer than 4 rows: change the seed"
    nd = maps32.shape[1] - 3
    m = margins(maps32[0, 0], maps32[0, 1:1 + nd], cfg["conf"], cfg["emb_margin"])
    assert min(m) >= MARGIN, f"{tag}: a clustering decision within {MARGIN} of the gap {m}: change the seed"
    out[f"{tag}_canvas"], out[f"{tag}_lane_id"], out[f"{tag}_lane_rows"] = c32[0], c32[1], c32[2]
    out[f"{tag}_points32"], out[f"{tag}_points64"] = c32[3].astype(np.float64), c64[3]
    out[f"{tag}_fit32"], out[f"{tag}_fit64"] = c32[4], c64[4]
    out[f"{tag}_margins"] = np.asarray(m)
    return m


# ---- the head under the shim ---------------------------------------------------------------------------------------
def _namespace():
    import paddle_shim as ps

    p = ps.install(REF)
    nn = p.nn

    class Upsample(nn.Layer):
        def __init__(self, size=None, scale_factor=None, mode="nearest"):
            super().__init__()
            self._size, self._scale = size, scale_factor

        def forward(self, x):
            return torch.nn.functional.interpolate(x, size=None if self._size is None else tuple(self._size),
                                                   scale_factor=self._scale, mode="nearest")

    class Dropout2D(nn.Layer):
        def __init__(self, p=0.5):
            super().__init__()

        def forward(self, x):
            return x

    nn.Upsample, nn.Dropout2D = Upsample, Dropout2D
    nn.Sequential.sublayers = lambda self, include_self=False: list(self.modules())[0 if include_self else 1:]
    for loss in ("BCEWithLogitsLoss", "MSELoss", "BCELoss"):
        setattr(nn, loss, lambda *a, **k: None)
    import tempfile

    ns = dict(paddle=p, nn=nn, F=p.nn.functional, np=np, os=os, osp=os.path, tempfile=tempfile,
              naive_init_module=lambda m: m, init_weight=lambda m: None, manager=ps._Anything("manager"),
              resnet34=lambda pretrained=None: torch.nn.Sequential(), IoULoss=lambda *a, **k: None,
              NDPushPullLoss=lambda *a, **k: None)
    ps.exec_lines(MODEL, [(50, 108), (111, 140), (143, 180), (183, 231), (234, 279), (282, 299), (302, 345)], ns)
    return ps, ns


def build_reference_net(ns, s32, c64, bev, output_size):
    """down (composed as bev_lanedet.py:313-324 composes it), the two FCTransform_ and the lane head."""
    nn = ns["nn"]
    c32, h32, w32 = s32
    net = torch.nn.Module()
    net.down = ns["Residual"](module=nn.Sequential(nn.Conv2D(c32, c64, kernel_size=3, stride=2, padding=1),
                                                   nn.BatchNorm2D(c64), nn.ReLU(),
                                                   nn.Conv2D(c64, c64, kernel_size=3, stride=1, padding=1),
                                                   nn.BatchNorm2D(c64)),
                              downsample=nn.Conv2D(c32, c64, kernel_size=3, stride=2, padding=1))
    net.s32transformer = ns["FCTransform_"](s32, bev)
    net.s64transformer = ns["FCTransform_"]((c64, (h32 + 1) // 2, (w32 + 1) // 2), bev)
    net.lane_head = ns["LaneHeadResidualInstanceWithOffsetZ"](output_size, input_channel=2 * bev[0])
    return net


def head_state(shapes, seed, scales):
    """The seeded state of a head case from its key -> shape list (paddle_shim.fill_state's draw), with the final
    convolutions rescaled so that lanes come out: `scales` = (seg bias, emb weight factor)."""
    import paddle_shim as ps

    rng = np.random.default_rng(seed)
    state = {k: ps.synth_param(k, tuple(shapes[k]), rng) for k in sorted(shapes)}
    state["lane_head.head.ms_new.6.bias"] = (state["lane_head.head.ms_new.6.bias"] + np.float32(scales[0])).astype(np.float32)
    state["lane_head.head.me_new.6.weight"] = (state["lane_head.head.me_new.6.weight"] * np.float32(scales[1])).astype(np.float32)
    return state


def run_reference_net(net, x, dtype):
    net = net.to(dtype).eval()
    with torch.no_grad():
        s32 = torch.from_numpy(x).to(dtype)
        s64 = net.down(s32)
        bev = torch.cat([net.s64transformer(s64), net.s32transformer(s32)], 1)
        seg, emb, off, z = net.lane_head(bev)
        return torch.cat([seg, emb, torch.sigmoid(off), z], 1).numpy()


def main():
    ref = (_load_file("cluster"), _load_file("post_process"), os.path.join(APOLLO, "apollo_lane_metric.py"))
    out = {}
    for tag, (seed, H, W, nd, lanes) in POST_CASES.items():
        rng = np.random.default_rng(seed)
        maps = np.concatenate(ln.synthetic_lanes(rng, 1, H, W, nd, lanes=lanes), 1)
        cfg = dict(ln.CFG, max_x=H * 0.5 + 3.0)
        out[f"{tag}_maps"] = maps
        out[f"{tag}_cfg"] = np.asarray([cfg["conf"], cfg["emb_margin"], cfg["min_cluster_size"], cfg["max_x"],
                                        *cfg["meter_per_pixel"]], np.float64)
        print(tag, "margins", record_post(out, tag, ref, maps, cfg), "lanes", out[f"{tag}_lane_rows"])
    ps, ns = _namespace()
    full = ns["BEVLaneDet"](bev_shape=(200, 48), output_2d_shape=(144, 256), train=True)
    out["state_keys"] = np.asarray(sorted(full.state_dict()))
    del full
    for tag, (seed, B, s32, c64, bev, size) in HEAD_CASES.items():
        net = build_reference_net(ns, s32, c64, bev, size)
        shapes = {k: list(v.shape) for k, v in net.state_dict().items()}
        for trial in range(200):
            rng = np.random.default_rng(seed + 1000 * trial)
            x = rng.standard_normal((B, *s32)).astype(np.float32)
            scales = (rng.uniform(0.5, 1.5), rng.uniform(20.0, 60.0))
            state = head_state(shapes, seed + 1000 * trial, scales)
            net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
            maps32, maps64 = run_reference_net(net, x, torch.float32), run_reference_net(net, x, torch.float64)
            net = net.float()
            try:
                assert np.abs(maps32[:, 0] - np.float32(0.9)).min() >= 1e-2, "a seg logit at the threshold"
                assert np.abs(maps64[:, 0] - 0.9).min() >= 1e-2, "a seg logit at the threshold"
                trial_out = {}
                for b in range(B):
                    record_post(trial_out, f"{tag}_f{b}", ref, maps32[b:b + 1], HEAD_POST)
                    c64r = reference_post(ref, maps64[b:b + 1], HEAD_POST)
                    assert np.array_equal(c64r[0], trial_out[f"{tag}_f{b}_canvas"]), "the fp64 maps draw another canvas"
                    trial_out[f"{tag}_f{b}_points64"], trial_out[f"{tag}_f{b}_fit64"] = c64r[3], c64r[4]
            except AssertionError as e:
                print(tag, "trial", trial, "refused:", str(e)[:100])
                continue
            out.update(trial_out)
            out[f"{tag}_x"], out[f"{tag}_maps32"], out[f"{tag}_maps64"] = x, maps32, maps64
            out[f"{tag}_seed"] = np.asarray([seed + 1000 * trial], np.int64)
            out[f"{tag}_scales"] = np.asarray(scales, np.float64)
            out[f"{tag}_keys"] = np.asarray(sorted(shapes))
            out[f"{tag}_shapes"] = np.asarray([",".join(str(s) for s in shapes[k]) for k in sorted(shapes)])
            print(tag, "trial", trial, "lanes", [out[f"{tag}_f{b}_lane_rows"] for b in range(B)])
            break
        else:
            raise AssertionError(f"{tag}: no seed meets the conditions")
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
