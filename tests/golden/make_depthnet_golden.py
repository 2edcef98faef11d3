"""Golden vectors for BEVDepth's depth network and view transformer, from the reference's own Python: ASPP, SELayer,
Mlp, DepthNet.forward, LSSViewTransformerBEVDepth.get_mlp_input and .forward of
paddle3d/models/transformers/bevdet_transformer.py, executed through tests/golden/paddle_shim.py at small seeded shapes,
in float32 and in float64.

    python tests/golden/make_depthnet_golden.py     # needs the reference checkout; writes python_depthnet.npz

What the reference tree does not hold is installed on the shim at run time, from its definition:
  * paddle.vision.models.resnet.BasicBlock, from its formula: relu(bn2(conv2(relu(bn1(conv1(x))))) + x) with two 3 x 3
    convolutions without bias and no downsample (all DepthNet uses);
  * the layers the shim has no body for: nn.Sigmoid, nn.Dropout (the identity in eval mode), nn.AdaptiveAvgPool2D and
    F.interpolate, each torch's operator of the same definition;
  * the bev_pool_v2 custom op: bev_pool_v2_pyop is replaced by an index_add of depth[ranks_depth] * feat[ranks_feat] into
    the cells ranks_bev, in the dtype of its inputs (the reference's wrapper casts to float32, which would make the
    float64 run a float32 one).
What the reference itself pins is everything else: the modules' structure and state-dict keys, the order of the 27 MLP
inputs, the split into depth and context channels, the softmax axis, the layouts handed to the pooling.

The geometry (frustum, get_lidar_coor, voxel_pooling_prepare_v2) runs in float32 in both runs, so both pool the same
points into the same cells; the calibration is paddle3d_amd.synth.camera_rig's.

Every result is stored as the float64 run with make_bevformer_golden.bound (4 x the difference of the float32 and the
float64 run, one fp32 ulp of the largest magnitude as floor).  Inputs and parameters are regenerated from seeds
(inputs(tag), state(tag, shapes)); the file holds results, bounds and each module's key -> shape list.  `r50_keys` is the
key -> shape list of the reference's view transformer at the arguments of configs/bevdet/bevdet4d_r50_depth_nuscenes.yml.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from make_bevformer_golden import bound  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "python_depthnet.npz")
F32 = np.float32

# ASPP(inplanes, mid_channels): a (no dilation above 6 reaches), b (12 reaches one row), c (18 reaches)
ASPPS = {"aspp_a": dict(seed=41, N=2, cin=16, cmid=16, H=7, W=9),
         "aspp_b": dict(seed=42, N=1, cin=32, cmid=16, H=13, W=19),
         "aspp_c": dict(seed=43, N=1, cin=16, cmid=32, H=19, W=37)}
SES = {"se": dict(seed=44, N=2, C=16, H=5, W=7)}
MLPS = {"mlp": dict(seed=45, M=4, hidden=16, out=16)}
# DepthNet(in_channels, mid_channels, context_channels, depth_channels)
NETS = {"dn": dict(seed=46, N=3, cin=32, mid=16, ctx=8, D=10, H=7, W=9)}
# LSSViewTransformerBEVDepth: 3 cameras of 64 x 176 at stride 16 (4 x 11 maps), 15 depth bins, a 32 x 32 grid
VTS = {"vt": dict(seed=47, B=1, N=3, cin=16, cout=16, input_size=(64, 176), downsample=16,
                  grid=dict(x=[-51.2, 51.2, 3.2], y=[-51.2, 51.2, 3.2], z=[-5, 3, 8], depth=[1.0, 60.0, 4.0]))}
R50 = dict(grid_config=dict(x=[-51.2, 51.2, 0.8], y=[-51.2, 51.2, 0.8], z=[-5, 3, 8], depth=[1.0, 60.0, 0.5]),
           input_size=[256, 704], in_channels=512, out_channels=80, depthnet_cfg=dict(use_dcn=False), downsample=16)
TAGS = (*ASPPS, *SES, *MLPS, *NETS, *VTS)


def _cfg(tag):
    for group in (ASPPS, SES, MLPS, NETS, VTS):
        if tag in group:
            return group[tag]
    raise KeyError(tag)


def rig(tag):
    from paddle3d_amd import synth

    c = VTS[tag]
    return synth.camera_rig(c["seed"], n_cam=c["N"], input_size=c["input_size"], batch=c["B"])


def inputs(tag):
    """The case's input arrays (float32), in the order of the module's forward."""
    c = _cfg(tag)
    rng = np.random.default_rng(c["seed"])
    if tag in ASPPS:
        return (rng.standard_normal((c["N"], c["cin"], c["H"], c["W"])).astype(F32),)
    if tag in SES:
        return (rng.standard_normal((c["N"], c["C"], c["H"], c["W"])).astype(F32),
                rng.standard_normal((c["N"], c["C"], 1, 1)).astype(F32))
    if tag in MLPS:
        return (rng.standard_normal((c["M"], 27)).astype(F32),)
    if tag in NETS:
        return (rng.standard_normal((c["N"], c["cin"], c["H"], c["W"])).astype(F32),
                rng.standard_normal((1, c["N"], 27)).astype(F32))
    h, w = (s // c["downsample"] for s in c["input_size"])
    return (rng.standard_normal((c["B"], c["N"], c["cin"], h, w)).astype(F32),)


def state(tag, shapes):
    """Parameters under the reference's keys for {key: shape} (paddle_shim.fill_state's draw)."""
    import paddle_shim as ps

    rng = np.random.default_rng(_cfg(tag)["seed"] + 100)
    return {k: ps.synth_param(k, tuple(shapes[k]), rng) for k in sorted(shapes)}


def load():
    return dict(np.load(OUT))


def key_shapes(g, tag):
    return json.loads(str(g[f"{tag}_keys"]))


# ---- the reference run (needs the reference checkout) ---------------------------------------------------------------


def _install():
    import paddle_shim as ps
    import torch.nn.functional as TF

    p = ps.install(REF)
    nn = p.nn
    plain = lambda t: t.as_subclass(torch.Tensor) if isinstance(t, torch.Tensor) else t  # noqa: E731

    class Sigmoid(nn.Layer):
        def forward(self, x):
            return torch.sigmoid(x)

    class Dropout(nn.Layer):
        def __init__(self, p=0.5):
            super().__init__()

        def forward(self, x):
            if self.training:
                raise RuntimeError("eval mode only")
            return x

    class BasicBlock(nn.Layer):
        """The stand-in (see the module docstring)."""

        def __init__(self, inplanes, planes, stride=1, downsample=None):
            super().__init__()
            assert stride == 1 and downsample is None
            self.conv1 = nn.Conv2D(inplanes, planes, 3, padding=1, stride=stride, bias_attr=False)
            self.bn1 = nn.BatchNorm2D(planes)
            self.relu = nn.ReLU()
            self.conv2 = nn.Conv2D(planes, planes, 3, padding=1, bias_attr=False)
            self.bn2 = nn.BatchNorm2D(planes)

        def forward(self, x):
            out = self.relu(self.bn1(self.conv1(x)))
            out = self.bn2(self.conv2(out))
            return self.relu(out + x)

    nn.Sigmoid, nn.Dropout, nn.AdaptiveAvgPool2D = Sigmoid, Dropout, torch.nn.AdaptiveAvgPool2d
    nn.functional.interpolate = lambda x, size=None, mode="nearest", align_corners=False: ps._wrap(
        TF.interpolate(plain(x), size=tuple(size), mode=mode, align_corners=align_corners))
    sys.modules["paddle.vision.models.resnet"].BasicBlock = BasicBlock
    bt = ps.load("paddle3d.models.transformers.bevdet_transformer")

    def bev_pool_v2_pyop(depth, feat, ranks_depth, ranks_feat, ranks_bev, bev_feat_shape, interval_starts,
                         interval_lengths):
        depth, feat = plain(depth), plain(feat)
        c = feat.shape[-1]
        out = torch.zeros((int(np.prod(bev_feat_shape[:-1])), c), dtype=feat.dtype)
        vals = depth.reshape(-1)[plain(ranks_depth).long()][:, None] * feat.reshape(-1, c)[plain(ranks_feat).long()]
        out.index_add_(0, plain(ranks_bev).long(), vals)
        return ps._wrap(out.reshape(tuple(bev_feat_shape)).permute(0, 3, 1, 2))

    bt.bev_pool_v2_pyop = bev_pool_v2_pyop
    return ps, bt


def _build(bt, tag):
    c = _cfg(tag)
    if tag in ASPPS:
        return bt.ASPP(c["cin"], c["cmid"])
    if tag in SES:
        return bt.SELayer(c["C"])
    if tag in MLPS:
        return bt.Mlp(27, c["hidden"], c["out"])
    if tag in NETS:
        return bt.DepthNet(c["cin"], c["mid"], c["ctx"], c["D"])
    return bt.LSSViewTransformerBEVDepth(grid_config=c["grid"], input_size=c["input_size"], downsample=c["downsample"],
                                         in_channels=c["cin"], out_channels=c["cout"], depthnet_cfg=dict(use_dcn=False))


def _run(ps, bt, tag, dt):
    m = _build(bt, tag)
    shapes = {k: list(v.shape) for k, v in m.state_dict().items()}
    st = state(tag, shapes)
    with torch.no_grad():
        for k, v in m.state_dict().items():
            v.copy_(torch.from_numpy(st[k]))
    m = m.to(dt).eval()
    T = lambda a: ps._wrap(torch.from_numpy(np.ascontiguousarray(a)))  # noqa: E731
    xs = [T(a).to(dt) for a in inputs(tag)]
    out = {}
    with torch.no_grad():
        if tag in VTS:
            cams = {k: T(v) for k, v in rig(tag).items()}  # float32 in both runs: the same points in the same cells
            geo = [cams[k] for k in ("rots", "trans", "cam2imgs", "post_rots", "post_trans", "bda")]
            mlp = m.get_mlp_input(*geo)
            out["mlp_input"] = mlp.numpy()
            bev, depth = m([xs[0], *geo, mlp.to(dt)])
            out["y"], out["depth"] = bev.numpy(), depth.numpy()
        else:
            out["y"] = m(*xs).numpy()
    return out, shapes


def main():
    ps, bt = _install()
    out = {}
    for tag in TAGS:
        (r32, shapes), (r64, _) = _run(ps, bt, tag, torch.float32), _run(ps, bt, tag, torch.float64)
        for name in r64:
            if name == "mlp_input":
                assert np.array_equal(r32[name], r64[name])  # float32 in both runs
                out[f"{tag}_{name}"] = r32[name]
                continue
            b, err = bound(r32[name], r64[name])
            out[f"{tag}_{name}"], out[f"{tag}_{name}_bound"], out[f"{tag}_{name}_ref_err"] = r64[name], b, err
            print(f"{tag:7s} {name:6s} {str(r64[name].shape):18s} |.| max {np.abs(r64[name]).max():.3g} nonzero "
                  f"{np.count_nonzero(r64[name]) / r64[name].size:.2f} ref err {err:.3e} bound {b:.3e}")
        out[f"{tag}_keys"] = np.asarray(json.dumps(shapes))
    r50 = bt.LSSViewTransformerBEVDepth(**R50)
    out["r50_keys"] = np.asarray(json.dumps({k: list(v.shape) for k, v in r50.state_dict().items()}))
    print("r50", len(r50.state_dict()), "keys, D =", r50.D)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
