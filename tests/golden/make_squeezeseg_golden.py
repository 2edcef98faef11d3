"""Golden results for SqueezeSegV3 from the reference's own Python: paddle3d/models/backbones/sac.py and
models/segmentation/squeezesegv3/squeezesegv3.py imported through tests/golden/paddle_shim.py, and the reader's
LoadSemanticKITTIRange.__call__ (transforms/reader.py:271-275, 287-366) and functional.normalize (transforms/
functional.py:42-46) executed from the reference checkout's text at run time.  No reference text is copied here.

    python tests/golden/make_squeezeseg_golden.py        # needs the reference checkout; writes python_squeezeseg.npz

What the shim lacks for these files is added here, for the run only: F.unfold, F.interpolate (bilinear,
align_corners=True), nn.LeakyReLU, nn.Dropout2D (identity at inference), paddle.argmax.

Every case runs twice from the same float32 inputs and seeded state dicts: as written (float32) and with the shim's
float32 and torch's default dtype mapped to float64.  The file holds the float64 results and, per result,
make_bevformer_golden.bound: 4 x the largest difference between the two runs, one float32 ulp of the largest magnitude as
the floor.  Inputs and weights are regenerated from seeds (`inputs`, `state`); the file holds results, bounds and the
reference's state-dict key names only.

Cases
  b32   one SACISKBlock, C = 32, N = 2, H = 5, W = 19:  `y` (the 1x1 layer's relu) and `out` (the block's feature)
  b64   one SACISKBlock, C = 64, N = 1, H = 3, W = 33, likewise
  net   SACRangeNet21 + SqueezeSegV3.export_forward, N = 2, in_channels = 5, H = 8, W = 32 (the three width halvings end
        at 8 x 4): `stage0` (the first encoder stage with its downsample), `feat` (the decoder's last map), `logits`,
        `pred`, and `labels`: the prediction at seeded per-point pixels, as SqueezeSegV3.forward gathers them
  scan0, scan1   the reader and the normalisation on two synthetic scans of 1500 and 700 points at H = 8, W = 64 (set
        on the instance): `image`, `proj_x`, `proj_y`, `proj_idx`, `proj_mask`

Discrete results are the reference's alone; `main` asserts, and the seeds are chosen so that it holds: every pixel's
top-two logit gap exceeds twice the logits' bound and both runs give the same argmax; no point's float64 pixel
coordinate lies within `scan_margin` of an integer (4 x the largest float32-to-float64 difference of the reference's
proj_x / proj_y before the floor); no two points of a pixel have equal depth; the two runs give the same pixels,
proj_idx and proj_mask."""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_bevformer_golden import bound  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "python_squeezeseg.npz")
READER_PY = "paddle3d/transforms/reader.py"
FUNCTIONAL_PY = "paddle3d/transforms/functional.py"

BLOCKS = {"b32": dict(C=32, N=2, H=5, W=19, seed=41), "b64": dict(C=64, N=1, H=3, W=33, seed=42)}
NET = dict(N=2, in_channels=5, H=8, W=32, classes=20, seed=43, points=(300, 200))
SCANS = {"scan0": dict(n=1500, seed=51), "scan1": dict(n=700, seed=52)}
SCAN_H, SCAN_W = 8, 64
MEAN = (12.12, 10.88, 0.23, -1.04, 0.21)  # configs/_base_/semantickitti.yml: range, x, y, z, remission
STD = (12.32, 11.47, 6.91, 0.86, 0.16)
TAGS = tuple(BLOCKS) + ("net",)
RESULTS = {"b32": ("y", "out"), "b64": ("y", "out"), "net": ("stage0", "feat", "logits")}


def load():
    return dict(np.load(OUT))


def build(tag, fused=True, **kw):
    """Our module for the case: a SACISKBlock, or SqueezeSegV3 on a SACRangeNet21."""
    from paddle3d_amd import squeezesegv3 as sq

    if tag in BLOCKS:
        return sq.SACISKBlock(BLOCKS[tag]["C"], fused=fused, **kw).eval()
    return sq.SqueezeSegV3(sq.SACRangeNet21(in_channels=NET["in_channels"], fused=fused, **kw), None, NET["classes"]).eval()


def ref_key(k):
    return k.replace(".running_mean", "._mean").replace(".running_var", "._variance")


def spec(tag):
    """{the reference's key: shape} of the case's state dict (our module's entries under the reference's names; the test
    of the key lists holds them equal to what the reference reports, recorded in the file)."""
    return {ref_key(k): tuple(v.shape) for k, v in build(tag).state_dict().items() if not k.endswith("num_batches_tracked")}


def state(tag):
    """The seeded state dict: convolution weights N(0, 1 / fan_in), biases N(0, 0.1), BatchNorm scales U(0.5, 1.5),
    running means N(0, 0.5) and variances U(0.3, 2.5) (non-trivial running statistics in every case)."""
    rng = np.random.default_rng((BLOCKS[tag] if tag in BLOCKS else NET)["seed"] + 1000)
    st = {}
    for k, shape in sorted(spec(tag).items()):
        if k.endswith("_variance"):
            v = rng.uniform(0.3, 2.5, shape)
        elif k.endswith("_mean"):
            v = rng.normal(0, 0.5, shape)
        elif k.endswith("bias"):
            v = rng.normal(0, 0.1, shape)
        elif len(shape) == 1:
            v = rng.uniform(0.5, 1.5, shape)
        else:
            fan = float(np.prod(shape[1:])) if "_deconv" not in k else float(shape[0] * shape[2] * shape[3]) / 2.0
            v = rng.normal(0, 1, shape) / np.sqrt(fan)
        st[k] = v.astype(np.float32)
    return st


def inputs(tag):
    if tag in BLOCKS:
        c = BLOCKS[tag]
        rng = np.random.default_rng(c["seed"])
        return dict(xyz=rng.standard_normal((c["N"], 3, c["H"], c["W"])).astype(np.float32),
                    feature=rng.standard_normal((c["N"], c["C"], c["H"], c["W"])).astype(np.float32))
    rng = np.random.default_rng(NET["seed"])
    n = sum(NET["points"])
    offsets = np.concatenate([[0], np.cumsum(NET["points"])]).astype(np.int32)
    proj_y = rng.integers(0, NET["H"], n).astype(np.int32)
    proj_x = rng.integers(0, NET["W"], n).astype(np.int32)
    return dict(image=rng.standard_normal((NET["N"], NET["in_channels"], NET["H"], NET["W"])).astype(np.float32),
                proj_y=proj_y, proj_x=proj_x, offsets=offsets)


def scan(n, seed):
    """A synthetic scan [n, 4] float32: ranges 2 .. 60 m, every azimuth, pitches from just outside the sensor's field
    of view (those clamp to the first and last row) to inside it, remissions in [0, 1)."""
    rng = np.random.default_rng(seed)
    r = rng.uniform(2, 60, n)
    yaw = rng.uniform(-np.pi, np.pi, n)
    pitch = np.deg2rad(rng.uniform(-25.5, 3.5, n))
    pts = np.stack([r * np.cos(pitch) * np.cos(yaw), r * np.cos(pitch) * np.sin(yaw), r * np.sin(pitch),
                    rng.uniform(0, 1, n)], 1)
    return pts.astype(np.float32)


def scans():
    """(points [2200, 4], offsets [3]) of the two golden scans, concatenated."""
    parts = [scan(SCANS[t]["n"], SCANS[t]["seed"]) for t in SCANS]
    return np.concatenate(parts), np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)


def check_discrete(g):
    """The conditions under which no discrete result can depend on rounding; returns what it saw."""
    lg, lb = g["net_logits"], float(g["net_logits_bound"])
    top = np.sort(lg, axis=1)[:, ::-1]
    gap = float((top[:, 0] - top[:, 1]).min())
    assert gap > 2 * lb, ("a pixel's top-two logit gap within twice the bound", gap, lb)
    assert np.array_equal(lg.argmax(1), g["net_pred"])
    margin = float(g["scan_margin"])
    seen = dict(gap=gap, logits_bound=lb, scan_margin=margin)
    for t in SCANS:
        for k, size in (("fx", SCAN_W), ("fy", SCAN_H)):
            f = g[f"{t}_{k}"]
            inside = (f > 0) & (f < size)  # beyond the image the clamp decides, and it is margins away from deciding
            d = float(np.abs(f - np.round(f))[inside].min())
            assert d > margin, (t, k, "a pixel coordinate within the margin of an integer", d, margin)
            seen[f"{t}_{k}"] = d
        pts = scan(SCANS[t]["n"], SCANS[t]["seed"])
        depth = np.linalg.norm(pts[:, :3], 2, axis=1)
        pix = g[f"{t}_proj_y"].astype(np.int64) * SCAN_W + g[f"{t}_proj_x"]
        key = np.stack([pix, depth.view(np.uint32).astype(np.int64)], 1)
        assert len(np.unique(key, axis=0)) == len(key), (t, "two points of a pixel have equal depth")
    return seen


# ---- the reference run (needs the reference checkout) ---------------------------------------------------------------


def _install(dt):
    import paddle_shim as ps
    import torch.nn.functional as TF

    p = ps.install(REF)
    import paddle.nn as nn
    import paddle.nn.functional as F

    ps._DT["float32"] = dt
    p.float32 = dt
    plain = lambda t: t.as_subclass(torch.Tensor) if isinstance(t, torch.Tensor) else t  # noqa: E731
    F.unfold = lambda x, kernel_sizes, strides=1, paddings=0, dilations=1: ps._wrap(
        TF.unfold(plain(x), kernel_sizes, dilations, paddings, strides))
    F.interpolate = lambda x, size=None, mode="nearest", align_corners=False, **k: ps._wrap(
        TF.interpolate(plain(x), size=tuple(int(s) for s in size), mode=mode, align_corners=align_corners))
    p.argmax = lambda x, axis=None: ps._wrap(torch.argmax(plain(x), dim=axis))

    class LeakyReLU(nn.Layer):
        def __init__(self, negative_slope=0.01):
            super().__init__()
            self._slope = negative_slope

        def forward(self, x):
            return TF.leaky_relu(x, self._slope)

    class Dropout2D(nn.Layer):  # inference
        def __init__(self, p=0.5):
            super().__init__()

        def forward(self, x):
            return x

    nn.LeakyReLU, nn.Dropout2D = LeakyReLU, Dropout2D
    root = os.path.join(REF, "paddle3d", "models", "segmentation")
    ps._pkg("paddle3d.models.segmentation", root)
    ps._pkg("paddle3d.models.segmentation.squeezesegv3", os.path.join(root, "squeezesegv3"))
    sys.modules["paddle3d.models.base"] = ps._AnyAttr("paddle3d.models.base")
    return ps, p


def _load_state(module, st, dt):
    own = module.state_dict()
    assert sorted(own) == sorted(st), sorted(set(own) ^ set(st))[:5]
    with torch.no_grad():
        for k, v in own.items():
            assert tuple(v.shape) == st[k].shape, (k, tuple(v.shape), st[k].shape)
            v.copy_(torch.from_numpy(st[k]))
    return module.to(dt).eval()


def _models(dt):
    saved = torch.get_default_dtype()
    ps, p = _install(dt)
    torch.set_default_dtype(dt)
    try:
        sac = ps.load("paddle3d.models.backbones.sac")
        seg = ps.load("paddle3d.models.segmentation.squeezesegv3.squeezesegv3")
        T = lambda a: ps._wrap(torch.from_numpy(np.ascontiguousarray(a)).to(dt))  # noqa: E731
        res, keys = {}, {}
        for tag in BLOCKS:
            block = sac.SACISKBlock(BLOCKS[tag]["C"])
            keys[tag] = sorted(block.state_dict())
            _load_state(block, state(tag), dt)
            tap = {}
            block.position_mlp[1].register_forward_hook(lambda m, i, o, tap=tap: tap.update(y=o.detach()))
            inp = inputs(tag)
            with torch.no_grad():
                _, out = block(T(inp["xyz"]), T(inp["feature"]))
            res[f"{tag}_y"], res[f"{tag}_out"] = tap["y"].numpy(), out.numpy()
        # pretrained: the stubbed checkpoint loader does nothing, and the initialisers are not run
        model = seg.SqueezeSegV3(sac.SACRangeNet21(in_channels=NET["in_channels"], pretrained="seeded"), None,
                                 NET["classes"], pretrained="seeded")
        keys["net"] = sorted(model.state_dict())
        _load_state(model, state("net"), dt)
        tap = {}
        enc = model.backbone.encoder
        enc.encoder_stages[0].register_forward_hook(lambda m, i, o: tap.update(stage0=o[1].detach()))
        model.heads[-1].register_forward_hook(lambda m, i, o: tap.update(feat=i[0].detach(), logits=o.detach()))
        inp = inputs("net")
        with torch.no_grad():
            pred = model.export_forward(T(inp["image"]))
        for k in ("stage0", "feat", "logits"):
            res[f"net_{k}"] = tap[k].numpy()
        res["net_pred"] = pred.numpy()
        off = inp["offsets"]
        res["net_labels"] = np.concatenate([  # SqueezeSegV3.forward: pred[proj_y, proj_x] per frame
            pred[b][torch.from_numpy(inp["proj_y"][off[b]:off[b + 1]].astype(np.int64)),
                    torch.from_numpy(inp["proj_x"][off[b]:off[b + 1]].astype(np.int64))].numpy()
            for b in range(NET["N"])])
        return res, keys
    finally:
        ps._DT["float32"] = torch.float32
        torch.set_default_dtype(saved)


class _Numpy:
    """numpy for the reader's text, with two changes: fromfile hands the scan back in the run's dtype, and floor
    records its argument (the pixel coordinates before the floor)."""

    def __init__(self, dt):
        self._dt, self.floors = dt, []

    def __getattr__(self, name):
        return getattr(np, name)

    def fromfile(self, path, dtype=None):
        return np.fromfile(path, dtype=dtype).astype(self._dt)

    def floor(self, x):
        self.floors.append(np.array(x, np.float64))
        return np.floor(x)


def _reader(dt):
    import paddle_shim as ps

    res = {}
    for tag, c in SCANS.items():
        npx = _Numpy(dt)
        me = types.SimpleNamespace()
        ns = dict(np=npx, self=me, Sample=None, logger=None)
        ps.exec_lines(os.path.join(REF, READER_PY), [(273, 275)], ns)  # the inclinations, as the constructor sets them
        me.proj_H, me.proj_W = SCAN_H, SCAN_W
        ps.exec_lines(os.path.join(REF, READER_PY), [(287, 366)], ns)  # __call__ up to the meta entries
        fn = ps.exec_lines(os.path.join(REF, FUNCTIONAL_PY), [(42, 46)], dict(np=np, Tuple=tuple))  # normalize
        with tempfile.NamedTemporaryFile(suffix=".bin") as f:
            scan(c["n"], c["seed"]).tofile(f.name)
            sample = types.SimpleNamespace(path=f.name, meta={}, labels=None, data=None)
            ns["__call__"](me, sample)
        fx, fy = npx.floors
        res[f"{tag}_raw"] = np.array(sample.data)
        mean, std = np.array(MEAN)[:, None, None], np.array(STD)[:, None, None]  # NormalizeRangeImage.__init__'s arrays
        res[f"{tag}_image"] = fn["normalize"](np.array(sample.data), mean, std)
        res[f"{tag}_proj_x"], res[f"{tag}_proj_y"] = sample.meta["proj_x"], sample.meta["proj_y"]
        res[f"{tag}_proj_mask"] = sample.meta["proj_mask"] > 0
        res[f"{tag}_fx"], res[f"{tag}_fy"] = fx, fy
    return res


def _proj_idx(tag, g):
    """proj_idx is a local of the reader; it is what its mask and its range image determine: the point whose depth the
    pixel holds (depths in a pixel are distinct)."""
    pts = scan(SCANS[tag]["n"], SCANS[tag]["seed"])
    depth = np.linalg.norm(pts[:, :3], 2, axis=1)
    idx = np.full((SCAN_H, SCAN_W), -1, np.int32)
    rng_img = g[f"{tag}_raw"][0]
    for i in range(len(pts)):
        y, x = g[f"{tag}_proj_y"][i], g[f"{tag}_proj_x"][i]
        if rng_img[y, x] == depth[i]:
            idx[y, x] = i
    return idx


def main():
    out = {}
    (m32, keys), (m64, _) = _models(torch.float32), _models(torch.float64)
    for tag in TAGS:
        for k in RESULTS[tag]:
            a, b = m32[f"{tag}_{k}"], m64[f"{tag}_{k}"]
            assert a.dtype == np.float32 and b.dtype == np.float64
            out[f"{tag}_{k}"] = b
            out[f"{tag}_{k}_bound"], out[f"{tag}_{k}_ref_err"] = bound(a, b)
            print(f"{tag} {k} {b.shape}: |max| {np.abs(b).max():.3f}, the reference's own error "
                  f"{float(out[f'{tag}_{k}_ref_err']):.3e}, bound {float(out[f'{tag}_{k}_bound']):.3e}")
        out[f"{tag}_state_keys"] = np.array(keys[tag])
    for k in ("pred", "labels"):
        assert np.array_equal(m32[f"net_{k}"], m64[f"net_{k}"]), (k, "the two runs predict differently")
        out[f"net_{k}"] = m64[f"net_{k}"]
    assert len(np.unique(out["net_pred"])) > 3, "the prediction uses few classes"
    r32, r64 = _reader(np.float32), _reader(np.float64)
    margin = 0.0
    for tag in SCANS:
        for k in ("proj_x", "proj_y", "proj_mask"):
            assert np.array_equal(r32[f"{tag}_{k}"], r64[f"{tag}_{k}"]), (tag, k, "the two runs project differently")
            out[f"{tag}_{k}"] = r64[f"{tag}_{k}"]
        assert r32[f"{tag}_fx"].dtype == np.float64 and r32[f"{tag}_image"].dtype == np.float32
        for k in ("fx", "fy"):
            margin = max(margin, 4.0 * float(np.abs(r32[f"{tag}_{k}"] - r64[f"{tag}_{k}"]).max()))
            out[f"{tag}_{k}"] = r64[f"{tag}_{k}"]
        out[f"{tag}_image"] = r64[f"{tag}_image"]
        out[f"{tag}_image_bound"], out[f"{tag}_image_ref_err"] = bound(r32[f"{tag}_image"], r64[f"{tag}_image"].astype(np.float64))
        out[f"{tag}_raw"] = r32[f"{tag}_raw"]
        i32, i64 = _proj_idx(tag, r32), _proj_idx(tag, dict(r64, **{f"{tag}_raw": r32[f"{tag}_raw"]}))
        assert np.array_equal(i32, i64) and np.array_equal(i32 > 0, out[f"{tag}_proj_mask"]), (tag, "proj_idx")
        out[f"{tag}_proj_idx"] = i32
        print(f"{tag}: {int((i32 >= 0).sum())} of {i32.size} pixels taken, image bound {float(out[f'{tag}_image_bound']):.3e}")
    out["scan_margin"] = np.float64(margin)
    print(check_discrete(out))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
