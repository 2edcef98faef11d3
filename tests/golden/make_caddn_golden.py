"""Golden vectors for CaDDN's frustum-to-voxel and map-to-BEV stage from the reference's own Python, executed through
tests/golden/paddle_shim.py at small seeded shapes:

    FrustumGridGenerator                        models/detection/caddn/f2v/frustum_grid_generator.py
    Sampler, FrustumToVoxel                     f2v/sampler.py, f2v/frustum_to_voxel.py
    FFE.create_frustum_features                 ffe/ffe.py:75-97
    the flatten + map_to_bev of CADDN.test_forward   caddn.py:114-122 (ConvBNReLU: models/layers/layer_libs.py:316-339)
    bin_depths, create_meshgrid3d / normalize_coords, transform_points_3d / project_to_image
                                                utils/depth.py, utils/grid.py:21-67, utils/transform.py

    python tests/golden/make_caddn_golden.py     # needs the reference checkout; writes python_caddn.npz

What the shim lacks is supplied here: the 5-D grid_sample (torch's), paddle.shape / isfinite / flip / log, a linspace
that takes 0-dim tensors, full(fill_value=), Tensor.flatten(start_axis, stop_axis) and Conv2D._in_channels.

One departure is forced.  transform_points_3d (utils/transform.py:141-147) reshapes the [B, X, Y, Z, 3] grid to
[B * X * Y, Z, 3] and TILES the B transformations X * Y times, which pairs row n of the points with transformation
n % B and not n // (X * Y): with B > 1 and calibrations that differ, a frame's voxels are transformed with the other
frames' matrices in turn (asserted below; CaDDN's own code calls kornia's transform_points, which broadcasts per
frame).  With equal calibrations, or B = 1, the tiling is invisible.  The golden vectors therefore run the reference
ONE FRAME AT A TIME -- lidar_to_cam[b : b + 1], cam_to_img[b : b + 1], that frame's features -- with the whole batch's
image_shape, which the reference only reduces to its maximum: the per-frame semantics the device ops have (a frame's
result does not depend on its place in the batch).

Cases (smallest shapes at which the kernels can still go wrong):
  a  pc_range [2, -4.8, -2, 11.6, 4.8, 1.2], voxel 0.4 (24 x 24 x 8), LID with 12 bins, C = C_out = 16, image 48 x 160,
     feature map 12 x 40, B = 2 with two calibrations (one slightly rotated) and two image_shape rows neither of which
     is the maximum
  b  an 11 x 9 x 3 grid whose x_min is behind the camera, UD with 80 bins, C = C_out = 64, a 5 x 7 feature map, B = 1
  c  SID with 10 bins, C = 32, C_out = 48, Z = 25, B = 3, a 5 x 4 grid in (x, y); the middle frame's calibration puts
     every voxel outside the image
The feature maps and logits come from seeded generators (inputs(tag), also what the tests call), the map_to_bev weights
from paddle_shim.fill_state (state(g, tag)); only the calibrations and the reference's outputs are stored.

Stored per case: the reference's fp32 grid, voxel_features and spatial_features; for each the bound the tests read --
4 x the largest error of the reference's own fp32 result against the SAME Python run in fp64 from the same fp32 inputs
and weights, one fp32 ulp of the largest output magnitude as a floor (make_roi_head_golden.bound) -- and, for the grid,
the mask of components whose fp64 value is within rounding of not being finite (domain_edge; the -2 of the fp32 and
of the fp64 run are asserted to sit on the same components elsewhere).

Asserted here (check_conditions, which tests/test_caddn_cpu.py runs again on the committed file): in every frame but
the planted one the share of voxels with a non-zero reference sample is in [0.25, 0.9]; every case has voxels with
exactly one, two and four in-range (y, x) corners; the LID / SID cases have NaN-replaced coordinates; no homogeneous
|w| lies within a factor of 10 of 1e-8 (the one discontinuous branch).
"""
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import caddn_numpy as cn  # noqa: E402
import make_roi_head_golden as mkr  # noqa: E402
import paddle_shim as ps  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "python_caddn.npz")
TAGS = ("a", "b", "c")
F32 = np.float32

CASES = {
    "a": dict(pc_range=[2.0, -4.8, -2.0, 11.6, 4.8, 1.2], voxel_size=[0.4, 0.4, 0.4],
              disc_cfg={"mode": "LID", "num_bins": 12, "depth_min": 2.5, "depth_max": 12.0},
              C=16, C_out=16, h=12, w=40, image_shape=[[48, 156], [46, 160]], planted=()),
    "b": dict(pc_range=[-1.6, -3.6, -1.8, 7.2, 3.6, 0.6], voxel_size=[0.8, 0.8, 0.8],
              disc_cfg={"mode": "UD", "num_bins": 80, "depth_min": 0.5, "depth_max": 7.5},
              C=64, C_out=64, h=5, w=7, image_shape=[[20, 28]], planted=()),
    "c": dict(pc_range=[-2.4, -2.0, -3.0, 5.6, 2.0, 1.0], voxel_size=[1.6, 1.0, 0.16],
              disc_cfg={"mode": "SID", "num_bins": 10, "depth_min": 0.5, "depth_max": 6.5},
              C=32, C_out=48, h=6, w=8, image_shape=[[24, 30], [22, 32], [24, 31]], planted=(1,)),
}


def grid_size(tag):
    return cn.grid_size(CASES[tag]["pc_range"], CASES[tag]["voxel_size"])


def _rot(yaw, pitch):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    return rz @ ry


def calib(tag):
    """(lidar_to_cam [B, 4, 4], cam_to_img [B, 3, 4]) float32: KITTI's axes (x_cam = -y, y_cam = -z, z_cam = x), its
    small translations, a pinhole with KITTI's field of view scaled to the case's image."""
    c = CASES[tag]
    axes = np.array([[0.0, -1, 0], [0, 0, -1], [1, 0, 0]])
    l2c, c2i = [], []
    for b, (H, W) in enumerate(c["image_shape"]):
        Hm, Wm = np.max(c["image_shape"], 0)
        r = _rot(0.03, -0.02) if b == 1 and tag == "a" else (_rot(-0.02, 0.01) if b == 2 else np.eye(3))
        m = np.eye(4)
        m[:3, :3] = axes @ r
        m[:3, 3] = (-0.004 + 0.01 * b, -0.076, -0.27)
        f = 0.58 * Wm * (1.0 + 0.02 * b)
        p = np.array([[f, 0, 0.49 * Wm, 0.036 * f], [0, f, 0.46 * Hm, 0.0003 * f], [0, 0, 1, 0.0027]])
        if b in c["planted"]:
            p[0, 2] = 40.0 * Wm  # the principal point far off the image: every voxel projects outside
        l2c.append(m)
        c2i.append(p)
    return np.asarray(l2c, F32), np.asarray(c2i, F32)


def inputs(tag):
    """(image_features [B, C, h, w], depth_logits [B, D + 1, h, w]) float32 from the case's seed."""
    c = CASES[tag]
    rng = np.random.default_rng(900 + ord(tag))
    B, D = len(c["image_shape"]), c["disc_cfg"]["num_bins"]
    feats = rng.standard_normal((B, c["C"], c["h"], c["w"])).astype(F32)
    logits = (1.5 * rng.standard_normal((B, D + 1, c["h"], c["w"]))).astype(F32)
    return feats, logits


def map_to_bev_cfg(tag):
    c = CASES[tag]
    return {"in_channels": c["C"] * grid_size(tag)[2], "out_channels": c["C_out"], "kernel_size": 1, "stride": 1,
            "bias_attr": False, "padding": 0}


def f2v_cfg(tag):
    c = CASES[tag]
    return {"pc_range": c["pc_range"], "voxel_size": c["voxel_size"],
            "sample_cfg": {"mode": "bilinear", "padding_mode": "zeros"}}


def _t(x):
    return x.as_subclass(torch.Tensor) if isinstance(x, torch.Tensor) else torch.as_tensor(x)


def build_reference():
    """The reference's classes, executed from its files."""
    p = ps.install(REF)
    wrap = ps._wrap
    TF = torch.nn.functional
    p.shape = lambda x: [int(s) for s in x.shape]
    p.isfinite = lambda x: wrap(torch.isfinite(_t(x)))
    p.flip = lambda x, axis: wrap(torch.flip(_t(x), [int(a) for a in axis]))
    p.log = lambda x: wrap(torch.log(_t(x)))
    p.linspace = lambda a, b, n, dtype=None: wrap(torch.linspace(float(a), float(b), int(n),
                                                                   dtype=ps._dt(dtype) or torch.float32))
    p.full = lambda shape, fill_value, dtype="float32": wrap(torch.full(tuple(int(s) for s in shape), fill_value,
                                                                         dtype=ps._dt(dtype)))
    p.nn.functional.grid_sample = lambda x, grid, mode="bilinear", padding_mode="zeros", align_corners=True: wrap(
        TF.grid_sample(_t(x), _t(grid), mode=mode, padding_mode=padding_mode, align_corners=align_corners))
    ps.Tensor.flatten = lambda self, start_axis=0, stop_axis=-1: wrap(torch.flatten(_t(self), start_axis, stop_axis))
    for sub in ("models/detection/caddn", "models/detection/caddn/f2v"):
        ps._pkg("paddle3d." + sub.replace("/", "."), os.path.join(REF, "paddle3d", sub))
    grid_utils = ps.exec_lines(os.path.join(REF, "paddle3d/utils/grid.py"), [(21, 67)], dict(paddle=p, np=np))
    gm = sys.modules["paddle3d.utils.grid"] = type(sys)("paddle3d.utils.grid")  # the file's imports need PIL
    gm.create_meshgrid3d, gm.normalize_coords = grid_utils["create_meshgrid3d"], grid_utils["normalize_coords"]
    f2v = ps.load("paddle3d.models.detection.caddn.f2v.frustum_to_voxel")
    ffe = ps.exec_lines(os.path.join(REF, "paddle3d/models/detection/caddn/ffe/ffe.py"), [(75, 97)],
                        dict(paddle=p, F=p.nn.functional))
    libs = ps.exec_lines(os.path.join(REF, "paddle3d/models/layers/layer_libs.py"), [(316, 339)], dict(nn=p.nn))
    return p, f2v.FrustumToVoxel, ffe["create_frustum_features"], libs["ConvBNReLU"]


def flatten_map_to_bev(p, map_to_bev, voxel_features):
    """caddn.py:114-122 on a dict with voxel_features."""
    me = type("Me", (), {})()
    me.map_to_bev = map_to_bev
    ns = dict(paddle=p, self=me, data={"voxel_features": voxel_features})
    ps.exec_lines(os.path.join(REF, "paddle3d/models/detection/caddn/caddn.py"), [(114, 122)], ns)
    return ns["data"]["spatial_features"]


def run_frames(p, F2V, frustum_features, map_to_bev, tag, l2c, c2i, feats, logits, double):
    """(grid, voxel_features, spatial_features, homogeneous w's) of the reference, one frame at a time (see above)."""
    c = CASES[tag]
    cast = (lambda a: ps.tensor(np.asarray(a, F32)).double()) if double else (lambda a: ps.tensor(np.asarray(a, F32)))
    f2v = F2V(voxel_size=np.asarray(c["voxel_size"]), pc_range=c["pc_range"], sample_cfg=f2v_cfg(tag)["sample_cfg"],
              disc_cfg=dict(c["disc_cfg"]))
    conv = copy.deepcopy(map_to_bev)
    if double:
        g = f2v.grid_generator
        g.voxel_grid, g.grid_to_lidar = g.voxel_grid.double(), g.grid_to_lidar.double()
        conv = conv.double()
    shape = ps.tensor(np.asarray(c["image_shape"], np.int32))
    grids, voxels, bevs = [], [], []
    with torch.no_grad():
        for b in range(len(l2c)):
            frustum = frustum_features(None, image_features=cast(feats[b:b + 1]), depth_logits=cast(logits[b:b + 1]))
            bd = {"frustum_features": frustum, "trans_lidar_to_cam": cast(l2c[b:b + 1]),
                  "trans_cam_to_img": cast(c2i[b:b + 1]), "image_shape": shape}
            grids.append(_t(f2v.grid_generator(lidar_to_cam=bd["trans_lidar_to_cam"], cam_to_img=bd["trans_cam_to_img"],
                                               image_shape=shape)).numpy())
            bd = f2v(bd)
            voxels.append(_t(bd["voxel_features"]).contiguous().numpy())
            bevs.append(_t(flatten_map_to_bev(p, conv, bd["voxel_features"])).numpy())
    return np.concatenate(grids), np.concatenate(voxels), np.concatenate(bevs)


def homogeneous_w(tag, l2c, c2i):
    """The two homogeneous w's of every voxel in float64: after the 4x4 product and after the projection."""
    c = CASES[tag]
    X, Y, Z = grid_size(tag)
    vs, mn = np.asarray(c["voxel_size"], F32).astype(np.float64), np.asarray(c["pc_range"][:3], F32).astype(np.float64)
    ii = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij"), -1) + 0.5
    pts = np.concatenate([ii * vs + mn, np.ones(ii.shape[:-1] + (1,))], -1)
    cam = np.einsum("bij,xyzj->bxyzi", l2c.astype(np.float64), pts)
    w1 = cam[..., 3]
    camp = np.concatenate([cam[..., :3] / w1[..., None], np.ones_like(w1)[..., None]], -1)
    return w1, np.einsum("bij,bxyzj->bxyzi", c2i.astype(np.float64), camp)[..., 2]


def domain_edge(tag, l2c, c2i):
    """[B, X, Y, Z] bool: voxels whose fp64 bin index is within rounding of not being finite -- the argument of LID's
    sqrt (1 + 8 (depth - depth_min) / bin_size) or of SID's log (1 + depth) within 1e-3 of 0, three orders above what
    fp32 rounding moves it by at these depths."""
    d = CASES[tag]["disc_cfg"]
    depth = homogeneous_w(tag, l2c, c2i)[1] - c2i.astype(np.float64)[:, 2, 3][:, None, None, None]
    if d["mode"] == "UD":
        return np.zeros(depth.shape, bool)
    if d["mode"] == "LID":
        bin_size = 2 * (d["depth_max"] - d["depth_min"]) / (d["num_bins"] * (1 + d["num_bins"]))
        return np.abs(1 + 8 * (depth - d["depth_min"]) / bin_size) < 1e-3
    return np.abs(1 + depth) < 1e-3


def corner_counts(tag, grid):
    """In-range (y, x) corners per voxel [B, X, Y, Z] of a normalised grid (any z)."""
    c = CASES[tag]
    g = np.asarray(grid, np.float64)
    fx, fy = ((g[..., 0] + 1) * c["w"] - 1) / 2, ((g[..., 1] + 1) * c["h"] - 1) / 2
    x0, y0 = np.floor(fx), np.floor(fy)
    nx = ((x0 >= 0) & (x0 <= c["w"] - 1)).astype(int) + ((x0 + 1 >= 0) & (x0 + 1 <= c["w"] - 1))
    ny = ((y0 >= 0) & (y0 <= c["h"] - 1)).astype(int) + ((y0 + 1 >= 0) & (y0 + 1 <= c["h"] - 1))
    return nx * ny


def check_conditions(g, tag):
    """The maker's conditions on a case of the file; returns what it measured."""
    c = CASES[tag]
    l2c, c2i = g[f"{tag}_lidar_to_cam"], g[f"{tag}_cam_to_img"]
    assert np.array_equal(l2c, calib(tag)[0]) and np.array_equal(c2i, calib(tag)[1])
    voxel = g[f"{tag}_voxel_features"]  # [B, C, Z, Y, X]
    share = [(np.abs(voxel[b]).max(0) > 0).mean() for b in range(len(voxel))]
    for b, s in enumerate(share):
        if b in c["planted"]:
            assert s == 0.0 and not np.ptp(g[f"{tag}_spatial_features"][b], axis=(1, 2)).any(), (tag, b, s)
        else:
            assert 0.25 <= s <= 0.9, (tag, b, s)
    counts = corner_counts(tag, g[f"{tag}_grid"])
    seen = {int(k): int((counts == k).sum()) for k in (1, 2, 4)}
    assert all(seen.values()), (tag, seen)
    replaced = int((g[f"{tag}_grid"] == -2).sum())
    if c["disc_cfg"]["mode"] != "UD":
        assert int(g[f"{tag}_nan_coords"]) > 0 and replaced >= int(g[f"{tag}_nan_coords"]), tag
    w1, w2 = homogeneous_w(tag, l2c, c2i)
    for w in (w1, w2):
        a = np.abs(w)
        assert not ((a > 1e-9) & (a < 1e-7)).any(), tag
    return dict(share=[round(float(s), 3) for s in share], corners=seen, replaced=replaced,
                min_w=float(min(np.abs(w1).min(), np.abs(w2).min())))


def main():
    p, F2V, frustum_features, ConvBNReLU = build_reference()
    out = {}
    for tag in TAGS:
        c = CASES[tag]
        l2c, c2i = calib(tag)
        feats, logits = inputs(tag)
        cfg = map_to_bev_cfg(tag)
        conv = ConvBNReLU(**cfg)
        conv._conv._in_channels = cfg["in_channels"]
        conv.eval()
        out[f"{tag}_state_shapes"] = np.asarray(json.dumps(ps.fill_state(conv, 300 + ord(tag))))
        r32 = run_frames(p, F2V, frustum_features, conv, tag, l2c, c2i, feats, logits, False)
        r64 = run_frames(p, F2V, frustum_features, conv, tag, l2c, c2i, feats, logits, True)
        assert all(a.dtype == np.float32 for a in r32) and all(a.dtype == np.float64 for a in r64)
        out[f"{tag}_lidar_to_cam"], out[f"{tag}_cam_to_img"] = l2c, c2i
        out[f"{tag}_image_shape"] = np.asarray(c["image_shape"], np.int32)
        for name, a32, a64 in zip(("grid", "voxel_features", "spatial_features"), r32, r64):
            out[f"{tag}_{name}"] = a32
            if name == "grid":  # -2 where either is: compare the finite coordinates
                both = (a32 != -2) & (a64 != -2)
                bound, err = mkr.bound(np.where(both, a32, 0), np.where(both, a64, 0))
                unsure = np.zeros(a32.shape, bool)
                unsure[..., 2] = domain_edge(tag, l2c, c2i)
                assert not (((a32 == -2) != (a64 == -2)) & ~unsure).any(), tag
                out[f"{tag}_grid_unsure"] = unsure
            else:
                bound, err = mkr.bound(a32, a64)
            out[f"{tag}_{name}_bound"], out[f"{tag}_{name}_ref_err"] = bound, err
        # NaN-replaced coordinates: the reference's own count before the replacement (-2 cannot arise otherwise)
        out[f"{tag}_nan_coords"] = np.int64((r32[0] == -2).sum())
        if len(l2c) > 1:  # the batched call, for the record of the departure
            f2v = F2V(voxel_size=np.asarray(c["voxel_size"]), pc_range=c["pc_range"],
                      sample_cfg=f2v_cfg(tag)["sample_cfg"], disc_cfg=dict(c["disc_cfg"]))
            shape = ps.tensor(np.asarray(c["image_shape"], np.int32))
            with torch.no_grad():
                batched = _t(f2v.grid_generator(lidar_to_cam=ps.tensor(l2c), cam_to_img=ps.tensor(c2i),
                                                image_shape=shape)).numpy()
                same = _t(f2v.grid_generator(lidar_to_cam=ps.tensor(np.repeat(l2c[:1], len(l2c), 0)),
                                             cam_to_img=ps.tensor(np.repeat(c2i[:1], len(l2c), 0)),
                                             image_shape=shape)).numpy()
            assert not np.allclose(batched, r32[0], atol=1e-3), "the tiled transformations: expected to differ"
            assert np.allclose(same[0], r32[0][0], atol=1e-5) and np.allclose(same[1], r32[0][0], atol=1e-5)
        g = {k: np.asarray(v) for k, v in out.items()}
        print(tag, "grid", grid_size(tag), check_conditions(g, tag),
              {k: float(out[f"{tag}_{k}_bound"]) for k in ("grid", "voxel_features", "spatial_features")},
              "unsure", int(out[f"{tag}_grid_unsure"].sum()))
    np.savez_compressed(OUT, **{k: np.asarray(v) for k, v in out.items()})
    print(os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 1_000_000


def load(path=OUT):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def state(g, tag):
    """map_to_bev's Paddle-named state dict, regenerated from the stored keys and shapes (fill_state's rule)."""
    shapes = json.loads(str(g[f"{tag}_state_shapes"]))
    rng = np.random.default_rng(300 + ord(tag))
    return {key: ps.synth_param(key, tuple(shapes[key]), rng) for key in sorted(shapes)}


if __name__ == "__main__":
    main()
