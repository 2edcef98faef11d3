"""CaDDN's entry points (the rows of paddle3d_amd._lib.ENTRY_POINTS that name this module) under guarded
allocations: tests/guarded.py's Protocol.  Each scenario builds seeded inputs and returns `(inputs, call)`; it runs plain,
guarded with fill 0x00 and guarded with fill 0xFF (tests/guarded.py), and the test asserts: no guard band damaged (no
store outside an output or a workspace), every input bit-equal to its clone, every specified output bit-equal across
the three runs (nothing depends on what a buffer held before) and not trivial.  The workspaces are outputs here: the
`raw` scenario calls the C ABI with workspaces of its own and returns their carved regions (softmax probabilities,
pixel-major features, the repacked weight; the bytes between the 256-byte aligned regions are never written and are
left out).  The model scenario constructs the module inside the run, so its tensors are allocated under the guard too.

The last test asserts that the scenarios reach every one of them."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from guarded import Protocol  # noqa: E402

import caddn_numpy as cn  # noqa: E402
import make_caddn_golden as mk  # noqa: E402
import test_caddn_cpu as cpu  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32

P = Protocol("test_memory_safety_caddn_gpu", "memory-safety-caddn", DEV)
scenario = P.scenario


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _case(g, tag):
    args = cpu.case_args(g, tag)
    names = ("image_features", "depth_logits", "lidar_to_cam", "cam_to_img", "image_shape")
    return {f"{tag}_{n}": _t(a) for n, a in zip(names, args[:5])}, args[5:]


@scenario
def ops():
    """The three ops at every golden case (odd grids, a tile with 20 of 64 columns, C and C_out of 16, 32, 48, 64) and
    frustum_to_voxel at a channel count that is no multiple of four; every output is written whole."""
    from paddle3d_amd.ops import caddn

    g = mk.load()
    inputs, rest = {}, {}
    for tag in mk.TAGS:
        dev, rest[tag] = _case(g, tag)
        inputs.update(dev)
        for n, a in zip(("weight", "scale", "shift"), cn.fold_bn(mk.state(g, tag))):
            inputs[f"{tag}_{n}"] = _t(a)
    inputs["odd_features"] = _t(np.random.default_rng(4).standard_normal((1, 7, 5, 7)).astype(F32))

    def call():
        outs = {}
        for tag in mk.TAGS:
            a = [inputs[f"{tag}_{n}"] for n in ("image_features", "depth_logits", "lidar_to_cam", "cam_to_img",
                                                "image_shape")]
            outs[f"{tag}_grid"] = caddn.frustum_grid(*a[2:], *rest[tag])
            outs[f"{tag}_voxel"] = caddn.frustum_to_voxel(*a, *rest[tag])
            outs[f"{tag}_bev"] = caddn.frustum_to_bev(*a, *rest[tag], *[inputs[f"{tag}_{n}"] for n in
                                                                        ("weight", "scale", "shift")])
        b = [inputs[f"b_{n}"] for n in ("depth_logits", "lidar_to_cam", "cam_to_img", "image_shape")]
        outs["odd_voxel"] = caddn.frustum_to_voxel(inputs["odd_features"], *b, *rest["b"])
        return outs

    return inputs, call


@scenario
def raw():
    """The C ABI with workspaces of the caller: their carved regions are outputs."""
    from paddle3d_amd import _lib
    from paddle3d_amd.ops._common import host_f32, ptr, stream_ptr
    from paddle3d_amd.ops.caddn import DISC_MODES

    g, tag = mk.load(), "c"
    c = mk.CASES[tag]
    inputs, (grid, pc_min, voxel_size, disc) = _case(g, tag)
    for n, a in zip(("weight", "scale", "shift"), cn.fold_bn(mk.state(g, tag))):
        inputs[n] = _t(a)
    B, C, CO, h, w, D = len(c["image_shape"]), c["C"], c["C_out"], c["h"], c["w"], disc["num_bins"]
    X, Y, Z = grid
    up = lambda n: (n + 255) // 256 * 256  # noqa: E731

    def call():
        L = _lib.lib()
        a = [ptr(inputs[f"{tag}_{n}"]) for n in ("image_features", "depth_logits", "lidar_to_cam", "cam_to_img",
                                                 "image_shape")]
        geo = (X, Y, Z, ptr(host_f32(pc_min, 3)), ptr(host_f32(voxel_size, 3)), DISC_MODES[disc["mode"]],
               float(disc["depth_min"]), float(disc["depth_max"]))
        s = stream_ptr(DEV)
        n_prob, n_feat, n_w = B * h * w * D * 4, B * h * w * C * 4, Z * C * CO * 4
        nv, nb = int(L.pd3_frustum_to_voxel_workspace(B, C, D, h, w)), int(L.pd3_frustum_to_bev_workspace(B, C, D, h, w, Z, CO))
        assert nv == up(n_prob) + up(n_feat) and nb == nv + up(n_w)
        wv = torch.empty(nv, dtype=torch.uint8, device=DEV)
        wb = torch.empty(nb, dtype=torch.uint8, device=DEV)
        voxel = torch.empty((B, C, Z, Y, X), dtype=torch.float32, device=DEV)
        bev = torch.empty((B, CO, Y, X), dtype=torch.float32, device=DEV)
        assert L.pd3_frustum_to_voxel(*a, B, C, D, h, w, *geo, ptr(voxel), ptr(wv), nv, s) == 0
        assert L.pd3_frustum_to_voxel(*a, B, C, D, h, w, *geo, ptr(voxel), ptr(wv), nv - 1, s) == -2
        assert L.pd3_frustum_to_bev(*a, B, C, D, h, w, *geo, ptr(inputs["weight"]), ptr(inputs["scale"]),
                                    ptr(inputs["shift"]), CO, ptr(bev), ptr(wb), nb, s) == 0
        f32 = lambda t, lo, n: t[lo:lo + n].view(torch.float32)  # noqa: E731
        return dict(voxel=voxel, bev=bev, voxel_probs=f32(wv, 0, n_prob), voxel_rows=f32(wv, up(n_prob), n_feat),
                    bev_probs=f32(wb, 0, n_prob), bev_rows=f32(wb, up(n_prob), n_feat), bev_weight=f32(wb, nv, n_w))

    return inputs, call


@scenario
def model():
    """FrustumToBEV fused and unfused and the unfused reference route, built inside the run."""
    from paddle3d_amd import caddn
    from paddle3d_amd.checkpoint import load_paddle_state_dict

    g, tag = mk.load(), "a"
    inputs, _ = _case(g, tag)

    def call():
        outs = {}
        for fused in (True, False):
            m = caddn.FrustumToBEV(mk.f2v_cfg(tag), mk.CASES[tag]["disc_cfg"], mk.map_to_bev_cfg(tag), fused=fused)
            load_paddle_state_dict(m, {f"map_to_bev.{k}": v for k, v in mk.state(g, tag).items()})
            m = m.eval().to(DEV)
            bd = {"trans_lidar_to_cam": inputs[f"{tag}_lidar_to_cam"], "trans_cam_to_img": inputs[f"{tag}_cam_to_img"],
                  "image_shape": inputs[f"{tag}_image_shape"]}
            with torch.no_grad():
                outs[f"bev_{fused}"] = m(inputs[f"{tag}_image_features"], inputs[f"{tag}_depth_logits"], bd)
                if not fused:
                    outs["grid"] = m.f2v.grid_generator(bd["trans_lidar_to_cam"], bd["trans_cam_to_img"], bd["image_shape"])
        return outs

    return inputs, call


@pytest.mark.parametrize("name", list(P.scenarios))
def test_scenario(name):
    P.check_scenario(name)


def test_every_launching_entry_point_is_exercised():
    """Runs last; scenarios that did not run in this process are run here in their plain form."""
    from paddle3d_amd import _lib

    P.check_complete(_lib.symbols("test_memory_safety_caddn_gpu"), 5)
