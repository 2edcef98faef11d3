"""Golden vectors for the first stage of Voxel R-CNN / PV-RCNN from the reference's own Python, executed through
tests/golden/paddle_shim.py:

    AnchorGenerator                             models/heads/dense_heads/target_assigner/anchor_generator.py:15-108
    AnchorHeadSingle.__init__ .. forward        models/heads/dense_heads/anchor_head.py:37-204
    ResidualCoder.decode_paddle                 utils/box_coder.py:22-100

    python tests/golden/make_two_stage_golden.py     # needs the reference checkout; writes python_two_stage.npz

Anchors, values in full: the Voxel R-CNN car configuration (1 class, 2 anchors per location) and the PV-RCNN
configuration (3 classes, 6 per location) of configs/voxel_rcnn/voxel_rcnn_005voxel_kitti_car.yml and
configs/pv_rcnn/pv_rcnn_005voxel_kitti.yml on feature maps (nx, ny) = 1x1, 4x5, 3x3, 16x16 over a range that grows with
the map, and one align_center case with two sizes, three rotations and two bottom heights on a 5 x 3 map.  A 1x1 map
without align_center has an infinite stride in the reference (a numpy quotient by zero) and no anchors: recorded as
that.  Anchors at full size: the SHA-256 of the float32 bytes of the head's `anchors` on the KITTI map (200 x 176).

Head forward, B = 2, weights from paddle_shim.fill_state (only their shapes are stored, synth_param reproduces them),
each in float32 and in float64 on the same float32 inputs, weights and anchors:
  a  1 class / 2 anchors, C = 16, map 4 x 5 (H x W)
  b  3 classes / 6 anchors, C = 32, map 3 x 3
  c  3 classes / 6 anchors, C = 256, map 2 x 2

Asserted here, so that direction labels and the period of a rotation are comparable exactly (a condition on the
inputs, checked with the reference alone; the seed is stepped until it holds): for every anchor the two direction
logits differ by more than 64 x the reference's own float32 error of the logits (float32 against float64 result,
maximum over the case), and the argument of limit_period's floor stays off an integer by more than 64 x its own
float32 error.
"""
import copy
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import paddle_shim as ps  # noqa: E402

REF = "/root/reference"
HEADS = os.path.join(REF, "paddle3d/models/heads/dense_heads")
OUT = os.path.join(HERE, "python_two_stage.npz")

VOXEL = [0.05, 0.05, 0.1]
STRIDE = 8


def _anchor_cfg(name, size, height, **kw):
    return dict({"class_name": name, "anchor_sizes": [size], "anchor_rotations": [0, 1.57],
                 "anchor_bottom_heights": [height], "align_center": False, "feature_map_stride": STRIDE}, **kw)


CAR_CFG = [_anchor_cfg("Car", [3.9, 1.6, 1.56], -1.78, matched_threshold=0.6, unmatched_threshold=0.45)]
KITTI3_CFG = [CAR_CFG[0],
              _anchor_cfg("Pedestrian", [0.8, 0.6, 1.73], -0.6, matched_threshold=0.5, unmatched_threshold=0.35),
              _anchor_cfg("Cyclist", [1.76, 0.6, 1.73], -0.6, matched_threshold=0.5, unmatched_threshold=0.35)]
ALIGN_CFG = [{"class_name": "Car", "anchor_sizes": [[3.9, 1.6, 1.56], [4.2, 1.7, 1.6]],
              "anchor_rotations": [0, 0.785, 1.57], "anchor_bottom_heights": [-1.78, -1.0], "align_center": True,
              "feature_map_stride": STRIDE}]
CONFIGS = {"car": CAR_CFG, "kitti3": KITTI3_CFG}
CLASS_NAMES = {"car": ["Car"], "kitti3": ["Car", "Pedestrian", "Cyclist"]}
MODEL_CFG = {"use_direction_classifier": True, "dir_offset": 0.78539, "dir_limit_offset": 0.0}
KITTI_RANGE = [0, -40, -3, 70.4, 40, 1]
MAPS = [(1, 1), (4, 5), (3, 3), (16, 16)]  # (nx, ny)
ALIGN_MAP = (5, 3)
# tag -> (configuration, input channels, H, W)
HEAD_CASES = {"a": ("car", 16, 4, 5), "b": ("kitti3", 32, 3, 3), "c": ("kitti3", 256, 2, 2)}


def map_range(nx, ny):
    """The point cloud range whose head map is nx x ny cells: x from 0, y centred, z as KITTI's."""
    cell = VOXEL[0] * STRIDE
    return [0.0, -ny * cell / 2, -3.0, nx * cell, ny * cell / 2, 1.0]


def _t(x):
    return x.as_subclass(torch.Tensor) if isinstance(x, torch.Tensor) else torch.as_tensor(x)


def build_reference():
    """The reference's AnchorGenerator and AnchorHeadSingle, executed from its files."""
    p = ps.install(REF)
    p.shape = lambda x: list(x.shape)
    unsqueeze = ps.Tensor.unsqueeze  # the generator passes the axis as a one-element list
    ps.Tensor.unsqueeze = lambda self, axis: unsqueeze(self, axis[0] if isinstance(axis, (list, tuple)) else axis)
    p.log = lambda x: ps._wrap(torch.log(_t(x)))
    p.normal = lambda mean=0.0, std=1.0, shape=None: ps._wrap(torch.zeros(tuple(shape)))  # the weights are seeded
    torch.nn.Parameter.set_value = lambda self, value: None  # init_weight's draws: the weights are seeded afterwards
    gen = ps.exec_lines(os.path.join(HEADS, "target_assigner/anchor_generator.py"), [(15, 108)], {})["AnchorGenerator"]
    coder = ps.exec_lines(os.path.join(REF, "paddle3d/utils/box_coder.py"), [(22, 100)], dict(paddle=p))["ResidualCoder"]
    nothing = lambda *a, **k: None  # noqa: E731  (training-only collaborators)
    ns = dict(np=np, paddle=p, nn=p.nn, F=p.nn.functional, ResidualCoder=coder, AnchorGenerator=gen,
              AxisAlignedTargetAssigner=nothing, WeightedSmoothL1Loss=nothing, SigmoidFocalClassificationLoss=nothing,
              WeightedCrossEntropyLoss=nothing, reset_parameters=nothing)
    head = ps.exec_lines(os.path.join(HEADS, "anchor_head.py"), [(37, 204)], ns)["AnchorHeadSingle"]
    return p, gen, head


def make_head(Head, cfg_name, channels, pcr):
    return Head(model_cfg=dict(MODEL_CFG), input_channels=channels, class_names=CLASS_NAMES[cfg_name],
                voxel_size=VOXEL, point_cloud_range=pcr, anchor_target_cfg={}, predict_boxes_when_training=True,
                anchor_generator_cfg=copy.deepcopy(CONFIGS[cfg_name]), num_dir_bins=2,
                loss_weights={"code_weights": [1.0] * 7})


def run_head(p, head, x):
    """-> (cls [B, A, K], box [B, A, 7], dir logits [B, A, bins], the argument of limit_period's floor [B, A])."""
    seen = []
    floor = p.floor
    p.floor = lambda v: (seen.append(_t(v).clone()), floor(v))[1]
    try:
        with torch.no_grad():
            bd = head({"spatial_features_2d": ps._wrap(x), "batch_size": int(x.shape[0])})
    finally:
        p.floor = floor
    assert bd["cls_preds_normalized"] is False and len(seen) == 1
    B = int(x.shape[0])
    dirs = _t(head.forward_ret_dict["dir_cls_preds"]).reshape(B, -1, head.num_dir_bins)
    return (_t(bd["batch_cls_preds"]).numpy(), _t(bd["batch_box_preds"]).numpy(), dirs.numpy(), seen[0].numpy())


def bound(ref32, ref64):
    err = float(np.abs(ref32.astype(np.float64) - ref64).max())
    ulp = float(np.spacing(np.float32(np.abs(ref64).max())))
    return np.float64(max(4.0 * err, ulp)), np.float64(err)


def head_case(p, Head, tag, seed):
    """One case at one seed, or None where the margins do not hold."""
    cfg_name, C, H, W = HEAD_CASES[tag]
    head = make_head(Head, cfg_name, C, map_range(W, H))
    head.eval()
    shapes = ps.fill_state(head, seed)
    x = torch.from_numpy(np.random.default_rng(seed).standard_normal((2, C, H, W)).astype(np.float32))
    cls32, box32, dir32, q32 = run_head(p, head, x)
    head64 = make_head(Head, cfg_name, C, map_range(W, H))
    head64.load_state_dict(head.state_dict())
    head64.eval().double()
    head64.anchors = ps._wrap(_t(head.anchors).double())
    cls64, box64, dir64, q64 = run_head(p, head64, x.double())
    assert box64.dtype == np.float64 and q64.dtype == np.float64 and cls32.dtype == np.float32
    dir_err = float(np.abs(dir32.astype(np.float64) - dir64).max())
    q_err = float(np.abs(q32.astype(np.float64) - q64).max())
    gap = float(np.abs(dir64[..., 0] - dir64[..., 1]).min())
    off = float(np.abs(q64 - np.round(q64)).min())
    if not (gap > 64 * dir_err and off > 64 * q_err):
        return None
    assert np.array_equal(dir32.argmax(-1), dir64.argmax(-1)) and np.array_equal(np.floor(q32), np.floor(q64))
    out = {"seed": np.int64(seed), "state_shapes": np.asarray(json.dumps(shapes)), "x": x.numpy(),
           "anchors": _t(head.anchors).numpy(), "cls": cls32, "box": box32, "cls64": cls64, "box64": box64,
           "dir_labels": dir64.argmax(-1).astype(np.int64), "floor": np.floor(q64).astype(np.int64),
           "dir_gap": np.float64(gap), "dir_err": np.float64(dir_err), "floor_off": np.float64(off),
           "floor_err": np.float64(q_err)}
    out["cls_bound"], out["cls_ref_err"] = bound(cls32, cls64)
    out["box_bound"], out["box_ref_err"] = bound(box32, box64)
    return out


def main():
    p, Gen, Head = build_reference()
    out = {}
    for name, cfg in CONFIGS.items():
        for nx, ny in MAPS:
            pcr = np.asarray(map_range(nx, ny))
            with np.errstate(divide="ignore"):
                anchors, per_loc = Gen(anchor_range=pcr, anchor_generator_config=copy.deepcopy(cfg)).generate_anchors(
                    [np.array([nx, ny], np.int64)] * len(cfg))
            for k, a in enumerate(anchors):
                out[f"anchors_{name}_{nx}x{ny}_{k}"] = _t(a).numpy()
            out[f"anchors_{name}_{nx}x{ny}_per_location"] = np.asarray(per_loc, np.int64)
            print(name, (nx, ny), [tuple(a.shape) for a in anchors], per_loc)
        head = make_head(Head, name, 16, KITTI_RANGE)
        a = _t(head.anchors).numpy()
        assert a.dtype == np.float32 and a.shape[:3] == (1, 200, 176)
        out[f"anchors_{name}_kitti_sha256"] = np.asarray(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())
        out[f"anchors_{name}_kitti_shape"] = np.asarray(a.shape, np.int64)
    nx, ny = ALIGN_MAP
    anchors, per_loc = Gen(anchor_range=np.asarray(map_range(nx, ny)),
                           anchor_generator_config=copy.deepcopy(ALIGN_CFG)).generate_anchors([np.array([nx, ny], np.int64)])
    out["anchors_align_0"], out["anchors_align_per_location"] = _t(anchors[0]).numpy(), np.asarray(per_loc, np.int64)
    print("align", tuple(anchors[0].shape), per_loc)

    for tag in HEAD_CASES:
        seed = 70 + ord(tag)
        case = head_case(p, Head, tag, seed)
        while case is None:
            seed += 100
            case = head_case(p, Head, tag, seed)
        out.update({f"{tag}_{k}": v for k, v in case.items()})
        print(tag, "seed", seed, "A", case["cls"].shape[1], "dir gap", float(case["dir_gap"]), "err",
              float(case["dir_err"]), "floor off", float(case["floor_off"]), "err", float(case["floor_err"]),
              "bounds", {k: float(v) for k, v in case.items() if k.endswith("_bound")})

    np.savez_compressed(OUT, **{k: np.asarray(v) for k, v in out.items()})
    print(os.path.getsize(OUT), "bytes")


def load(path=OUT):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def state(g, tag):
    """The recorded head's Paddle-named state dict, regenerated from the stored keys and shapes (fill_state's rule)."""
    shapes = json.loads(str(g[f"{tag}_state_shapes"]))
    rng = np.random.default_rng(int(g[f"{tag}_seed"]))
    return {k: ps.synth_param(k, tuple(shapes[k]), rng) for k in sorted(shapes)}


if __name__ == "__main__":
    main()
