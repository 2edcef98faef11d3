"""Golden vectors for the modulated deformable convolution and the MMResNet blocks built on it, from the reference's
own Python: DeformableConvV2.forward, Bottleneck.forward (caffe style, with dcn, eval-mode norm) and a two-block
ResLayer of paddle3d/models/backbones/mm_resnet.py, executed through tests/golden/paddle_shim.py at small seeded shapes,
in float32 and in float64.

    python tests/golden/make_dcn_golden.py     # needs the reference checkout; writes python_dcn.npz

Paddle's own DCN kernel (paddle.vision.ops.DeformConv2D) is not part of the reference tree.  The maker installs a
stand-in for it on the shim's `paddle.vision` object at run time: F.grid_sample(align_corners=True, padding_mode="zeros",
mode="bilinear") at the taps' pixel coordinates, times the mask, times the weight -- an independent formulation of the
same definition (a corner outside the image counts as zero), the precedent make_ms_deform_attn_golden.py set for
ms_deform_attn.  What the reference itself pins is everything around the op: the split of conv_offset's 27 channels into
18 offsets and 9 mask logits, the sigmoid, the paddings of conv_offset and conv_dcn, the layouts and the state-dict keys.
tests/golden/dcn_numpy.py is a second formulation (gathers); tests/test_dcn_cpu.py holds its float64 form to the
stand-in's float64 run to 1e-12.

Every result is stored as the float64 run with make_bevformer_golden.bound (4 x the difference of the float32 and the
float64 run, one fp32 ulp of the largest magnitude as floor).  Inputs and parameters are regenerated from seeds
(inputs(tag), state(tag, shapes)); the file holds results, bounds, conv_offset's float64 output and each module's
key -> shape list.

Cases: a (N = 2, 16 -> 16, 5 x 7), b (32 -> 48, 9 x 17) and b2 (the same sizes with stride 2 on a second input), c
(offsets of several pixels; taps 0, 4 and 8 pinned to exact integer and half-integer offsets so that samples land outside
the image, on the -1 and H borders and exactly on integers), d (the reference's initial state: conv_offset zero, every
mask 0.5), e (dilation 2); the bottlenecks ba (planes 16) and bb (planes 32) and the stage s (two blocks, stride 2).
`r50_keys` is the key -> shape list of the reference's MMResNet as the two CAPE ResNet-50 configs build it.
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from make_bevformer_golden import bound  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "python_dcn.npz")
F32 = np.float32

# DeformableConvV2 alone (with conv_dcn's bias, the class's default)
CASES = {
    "a": dict(seed=11, N=2, cin=16, cout=16, H=5, W=7, stride=1, dilation=1, offset_scale=1.0),
    "b": dict(seed=12, N=1, cin=32, cout=48, H=9, W=17, stride=1, dilation=1, offset_scale=1.5),
    "b2": dict(seed=13, N=1, cin=32, cout=48, H=9, W=17, stride=2, dilation=1, offset_scale=1.5),
    "c": dict(seed=14, N=1, cin=16, cout=32, H=6, W=9, stride=1, dilation=1, offset_scale=6.0, pinned=True),
    "d": dict(seed=15, N=1, cin=16, cout=16, H=5, W=7, stride=1, dilation=1, offset_scale=0.0, initial=True),
    "e": dict(seed=16, N=1, cin=16, cout=16, H=8, W=9, stride=1, dilation=2, offset_scale=1.0),
}
# Bottleneck(inplanes = 4 planes, planes, style="caffe", dcn=DCN): no downsample
BLOCKS = {"ba": dict(seed=21, N=2, planes=16, H=5, W=7, offset_scale=1.0),
          "bb": dict(seed=22, N=1, planes=32, H=9, W=17, offset_scale=1.5)}
# ResLayer(Bottleneck, inplanes, planes, 2 blocks, stride 2, style="caffe", dcn=DCN): the first block has the downsample
STAGE = {"s": dict(seed=31, N=1, inplanes=32, planes=16, H=10, W=14, offset_scale=1.0)}
DCN = dict(type_name="DeformConv2D", deformable_groups=1)
# case c: (tap, dy, dx) whose conv_offset rows are zero weights and these exact biases
PINNED = ((0, 0.0, 0.0), (4, 0.5, -0.5), (8, 3.0, 2.0))


def _cfg(tag):
    return CASES.get(tag) or BLOCKS.get(tag) or STAGE[tag]


def in_channels(tag):
    c = _cfg(tag)
    return c["cin"] if tag in CASES else (4 * c["planes"] if tag in BLOCKS else c["inplanes"])


def inputs(tag):
    c = _cfg(tag)
    rng = np.random.default_rng(c["seed"])
    return rng.standard_normal((c["N"], in_channels(tag), c["H"], c["W"])).astype(F32)


def state(tag, shapes):
    """Parameters under the reference's keys for {key: shape}."""
    c = _cfg(tag)
    rng = np.random.default_rng(c["seed"] + 100)
    st = {}
    for k in sorted(shapes):
        s = tuple(shapes[k])
        if k.endswith("_variance"):
            st[k] = rng.uniform(0.5, 1.5, s).astype(F32)
        elif k.endswith("_mean"):
            st[k] = rng.normal(0, 0.1, s).astype(F32)
        elif k.endswith("conv_offset.weight"):
            st[k] = (rng.normal(0, 1, s) * c["offset_scale"] / np.sqrt(np.prod(s[1:]))).astype(F32)
        elif k.endswith("conv_offset.bias"):
            st[k] = (rng.normal(0, 0.5, s) * min(c["offset_scale"], 1.0)).astype(F32)
        elif k.endswith("bias"):
            st[k] = rng.normal(0, 0.1, s).astype(F32)
        elif len(s) == 1:
            st[k] = rng.uniform(0.5, 1.5, s).astype(F32)
        else:
            st[k] = (rng.normal(0, 1, s) / np.sqrt(np.prod(s[1:]))).astype(F32)
    if c.get("pinned"):
        for tap, dy, dx in PINNED:
            st["conv_offset.weight"][2 * tap:2 * tap + 2] = 0
            st["conv_offset.bias"][2 * tap:2 * tap + 2] = (dy, dx)
    return st


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
    p.split = lambda x, num_or_sections, axis=0: [ps._wrap(t) for t in torch.split(plain(x), num_or_sections, dim=axis)]
    nn.MaxPool2D = torch.nn.MaxPool2d

    class DeformConv2D(nn.Layer):
        """The stand-in (see the module docstring): grid_sample in pixel coordinates with zeros padding."""

        def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, deformable_groups=1,
                     groups=1, weight_attr=None, bias_attr=None):
            super().__init__()
            assert deformable_groups == 1 and groups == 1
            k = kernel_size
            self.weight = torch.nn.Parameter(torch.zeros(out_channels, in_channels, k, k))
            self.bias = None if bias_attr is False else torch.nn.Parameter(torch.zeros(out_channels))
            self._k, self._s, self._p, self._d = k, stride, padding, dilation

        def forward(self, x, offset, mask=None):
            x, offset = plain(x), plain(offset)
            N, C, H, W = x.shape
            k, s, p, d = self._k, self._s, self._p, self._d
            Ho, Wo = (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1
            assert tuple(offset.shape) == (N, 2 * k * k, Ho, Wo)
            ys = (torch.arange(Ho, dtype=x.dtype) * s - p)[None, :, None]
            xs = (torch.arange(Wo, dtype=x.dtype) * s - p)[None, None, :]
            cols = []
            for tap in range(k * k):
                ky, kx = divmod(tap, k)
                h = ys + ky * d + offset[:, 2 * tap]
                w = xs + kx * d + offset[:, 2 * tap + 1]
                grid = torch.stack([2 * w / (W - 1) - 1, 2 * h / (H - 1) - 1], -1)  # (x, y), align_corners=True
                v = TF.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
                cols.append(v if mask is None else v * plain(mask)[:, tap:tap + 1])
            cols = torch.stack(cols, 2).reshape(N, C * k * k, Ho * Wo)
            y = torch.matmul(self.weight.reshape(self.weight.shape[0], -1), cols).reshape(N, -1, Ho, Wo)
            return y if self.bias is None else y + self.bias[None, :, None, None]

    vision = sys.modules["paddle.vision"]
    vision.ops = types.SimpleNamespace(DeformConv2D=DeformConv2D)
    p.vision = vision
    return ps, ps.load("paddle3d.models.backbones.mm_resnet")


def _build(mod, tag):
    if tag in CASES:
        c = CASES[tag]
        return mod.DeformableConvV2(c["cin"], c["cout"], 3, stride=c["stride"], padding=c["dilation"],
                                    dilation=c["dilation"])
    if tag in BLOCKS:
        c = BLOCKS[tag]
        return mod.Bottleneck(4 * c["planes"], c["planes"], style="caffe", dcn=DCN)
    c = STAGE[tag]
    return mod.ResLayer(block=mod.Bottleneck, inplanes=c["inplanes"], planes=c["planes"], num_blocks=2, stride=2,
                        style="caffe", dcn=DCN)


def _run(ps, mod, tag, dt):
    m = _build(mod, tag)
    shapes = {k: list(v.shape) for k, v in m.state_dict().items()}
    st = state(tag, shapes)
    with torch.no_grad():
        for k, v in m.state_dict().items():
            v.copy_(torch.from_numpy(st[k]))
    m = m.to(dt).eval()
    x = ps._wrap(torch.from_numpy(inputs(tag)).to(dt))
    out = {}
    with torch.no_grad():
        out["y"] = m(x).as_subclass(torch.Tensor).numpy()
        if tag in CASES:
            out["offset_mask"] = m.conv_offset(x).as_subclass(torch.Tensor).numpy()
    return out, shapes


def main():
    ps, mod = _install()
    out = {}
    for tag in (*CASES, *BLOCKS, *STAGE):
        (r32, shapes), (r64, _) = _run(ps, mod, tag, torch.float32), _run(ps, mod, tag, torch.float64)
        b, err = bound(r32["y"], r64["y"])
        out[f"{tag}_y"], out[f"{tag}_y_bound"], out[f"{tag}_y_ref_err"] = r64["y"], b, err
        out[f"{tag}_keys"] = np.asarray(json.dumps(shapes))
        line = f"{tag:3s} y {str(r64['y'].shape):18s} |y| max {np.abs(r64['y']).max():.3g} ref err {err:.3e} bound {b:.3e}"
        if tag in CASES:
            om, c = r64["offset_mask"], CASES[tag]
            out[f"{tag}_offset_mask"] = om
            # where the samples of the float64 run land: outside, on a border, on an integer
            Ho, Wo = om.shape[2:]
            ho = np.arange(Ho)[None, :, None] * c["stride"] - c["dilation"]
            wo = np.arange(Wo)[None, None, :] * c["stride"] - c["dilation"]
            h = np.stack([ho + (k // 3) * c["dilation"] + om[:, 2 * k] for k in range(9)], 1)
            w = np.stack([wo + (k % 3) * c["dilation"] + om[:, 2 * k + 1] for k in range(9)], 1)
            outside = (h <= -1) | (w <= -1) | (h >= c["H"]) | (w >= c["W"])
            on_border = (h == -1) | (h == c["H"]) | (w == -1) | (w == c["W"])
            integer = (h == np.floor(h)) & (w == np.floor(w)) & ~outside
            line += (f"  offsets |max| {np.abs(om[:, :18]).max():.2f}, outside {outside.mean():.3f}, on -1 / H "
                     f"{int(on_border.sum())}, on integers {int(integer.sum())}")
            if c.get("pinned"):
                assert outside.any() and on_border.any() and integer.any(), tag
            if c.get("initial"):
                assert not om.any(), tag
        print(line)
    # the key -> shape list of the two CAPE configs' backbone (no forward: the names a checkpoint has to be loaded under)
    mod.MMResNet.init_learning_rate = lambda self, lr_factor: None  # Paddle's per-parameter optimize_attr
    r50 = mod.MMResNet(depth=50, num_stages=4, out_indices=[2, 3], frozen_stages=-1,
                       norm_cfg=dict(type_name="BatchNorm2D", requires_grad=False), norm_eval=True, style="caffe", dcn=DCN,
                       stage_with_dcn=[False, False, True, True])
    out["r50_keys"] = np.asarray(json.dumps({k: list(v.shape) for k, v in r50.state_dict().items()}))
    print("r50", len(r50.state_dict()), "keys")
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
