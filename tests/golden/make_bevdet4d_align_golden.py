"""Golden vectors for BEVDet4D's temporal alignment from the reference's own Python: BEVDet4D.shift_feature
(paddle3d/models/detection/bevdet/bevdet4d.py:90-159), executed through tests/golden/paddle_shim.py.

    python tests/golden/make_bevdet4d_align_golden.py     # needs /root/reference; writes python_bevdet4d_align.npz

The method is executed from its line range (the module's imports drag in the whole framework) on a SimpleNamespace
whose img_view_transformer carries BEVDet4D's grid_interval / grid_lower_bound.  The shim gains Tensor.index_select
with `axis=` and F.grid_sample (torch's, CPU); the grid the method passes to grid_sample is recorded next to the
output, at a fixed seeded sample of bevdet4d_align_numpy.GOLDEN_PIXELS pixels per case (golden_pixels; the file stays
small).  Inputs are rebuilt from seeds (bevdet4d_align_numpy.golden_case) and not stored.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as TF

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import bevdet4d_align_numpy as ba  # noqa: E402
import paddle_shim as ps  # noqa: E402

REF = "/root/reference"
BEVDET4D = os.path.join(REF, "paddle3d/models/detection/bevdet/bevdet4d.py")


def _extend_shim(F, seen):
    """What shift_feature calls and the shim lacks (added here, paddle_shim.py stays as it is)."""
    W = ps._wrap

    def index_select(self, index, axis=0):
        return W(torch.index_select(self.as_subclass(torch.Tensor), axis, index.as_subclass(torch.Tensor).long()))

    def grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True):
        seen.append(grid.as_subclass(torch.Tensor).clone())
        return W(TF.grid_sample(x.as_subclass(torch.Tensor), grid.as_subclass(torch.Tensor), mode=mode,
                                padding_mode=padding_mode, align_corners=align_corners))

    ps.Tensor.index_select = index_select
    F.grid_sample = grid_sample


def main():
    p = ps.install(REF)
    import paddle.nn.functional as F

    seen = []
    _extend_shim(F, seen)
    ns = ps.exec_lines(BEVDET4D, [(90, 159)], dict(paddle=p, F=F, np=np))
    vt = types.SimpleNamespace(grid_interval=[float(v) for v in ba.GRID_INTERVAL] + [8.0],
                               grid_lower_bound=[float(v) for v in ba.GRID_LOWER] + [-5.0])
    self = types.SimpleNamespace(img_view_transformer=vt)
    T = ps.tensor
    out = {}
    for i in range(len(ba.GOLDEN_CASES)):
        c = ba.golden_case(i)
        seen.clear()
        with torch.no_grad():
            y = ns["shift_feature"](self, T(c["input"]), [T(t) for t in c["trans"]], [T(r) for r in c["rots"]],
                                    T(c["bda"]), None if c["bda_adj"] is None else T(c["bda_adj"]))
        assert len(seen) == 1
        g = seen[0].numpy().astype(np.float32)
        inside = float(((np.abs(g[..., 0]) <= 1) & (np.abs(g[..., 1]) <= 1)).mean())
        o, g = ba.at_pixels(y.numpy().astype(np.float32), g, ba.golden_pixels(i))
        out[f"grid_{i}"], out[f"out_{i}"] = np.ascontiguousarray(g), np.ascontiguousarray(o)
        print(f"case {i} {c['name']}: grid in [-1, 1]^2 for {inside:.3f} of the pixels")
    np.savez_compressed(os.path.join(HERE, "python_bevdet4d_align.npz"), **out)


if __name__ == "__main__":
    main()
