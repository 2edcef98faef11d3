"""CAPE's entry points (paddle3d_amd._lib.CAPE_ENTRY_POINTS, whose rows name this module) under guarded allocations:
tests/guarded.py's Protocol.  Each scenario builds seeded inputs and returns `(inputs, call)`; it runs plain, guarded with
fill 0x00 and guarded with fill 0xFF, and the test asserts: no guard band damaged (no store outside an output), every
input bit-equal to its clone, every output bit-equal across the three runs (nothing depends on what a buffer held before
-- the padding keys of a camera's last tile and the padded query rows included, since they end in the output) and not
trivial.  The kernels take no workspace.  The model scenario constructs the layers inside the run, so their tensors are
allocated under the guard too.

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

import make_cape_golden as mk  # noqa: E402
import test_cape_cpu as cpu  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32

P = Protocol("test_memory_safety_cape_gpu", "memory-safety-cape", DEV)
scenario = P.scenario


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# (N, K, Q, d, heads, B): one key; a camera border inside a wave's walk with a second query block of one row; 250 keys (a
# last tile of 10) at the largest head
CVA_SHAPES = ((1, 1, 1, 16, 1, 1), (3, 17, 17, 32, 3, 2), (5, 33, 15, 128, 1, 1), (2, 250, 37, 64, 2, 1))
# (B, N, Q, F): without views and with, one element, a row count past a workgroup, the largest F
POS_SHAPES = ((1, 0, 1, 2), (2, 0, 300, 96), (2, 3, 37, 8), (1, 2, 5, 128))


@scenario
def ops():
    """Both ops at the border shapes of tests/test_cape_gpu.py, with and without a mask, and at the golden case b."""
    from paddle3d_amd.ops import cape

    rng = np.random.default_rng(29)
    f = lambda *s: _t(rng.standard_normal(s).astype(F32))  # noqa: E731
    inputs = {}
    for i, (N, K, Q, d, heads, B) in enumerate(CVA_SHAPES):
        E = heads * d
        inputs.update({f"qa{i}": f(B, Q, E), f"qg{i}": f(B, N, Q, E), f"ka{i}": f(B, N, K, E), f"kg{i}": f(B, N, K, E),
                       f"v{i}": f(B, N, K, E), f"sa{i}": _t(rng.uniform(-0.3, 0.3, heads).astype(F32)),
                       f"sg{i}": _t(rng.uniform(-0.3, 0.3, heads).astype(F32))})
        m = rng.random((B, N, K)) < 0.4
        m[:, 0, 0] = False
        inputs[f"m{i}"] = _t(m)
    for i, (B, N, Q, F) in enumerate(POS_SHAPES):
        inputs[f"p{i}"] = _t(rng.random((B, Q, 3)).astype(F32))
        if N:
            inputs[f"R{i}"], inputs[f"t{i}"] = f(B, N, 3, 3), f(B, N, 3)
    g = mk.load()
    inputs.update(zip(("b_qa", "b_qg", "b_ka", "b_kg", "b_v", "b_sa", "b_sg", "b_m"), (_t(a) for a in cpu.ca_rows(g, "b"))))

    def call():
        x, outs = inputs, {}
        for i, (N, K, Q, d, heads, B) in enumerate(CVA_SHAPES):
            rows = tuple(x[f"{n}{i}"] for n in ("qa", "qg", "ka", "kg", "v", "sa", "sg"))
            outs[f"cva{i}"] = cape.cross_view_attention(*rows, heads)
            outs[f"cva{i}_masked"] = cape.cross_view_attention(*rows, heads, x[f"m{i}"])
        outs["b_cva"] = cape.cross_view_attention(*(x[n] for n in ("b_qa", "b_qg", "b_ka", "b_kg", "b_v", "b_sa", "b_sg")),
                                                  mk.CASES["b"]["heads"], x["b_m"])
        for i, (B, N, Q, F) in enumerate(POS_SHAPES):
            outs[f"pos{i}"] = cape.posemb3d(x[f"p{i}"], F, bound=mk.BOUND, rot=x.get(f"R{i}"), trans=x.get(f"t{i}"))
        outs["pos_plain"] = cape.posemb3d(x["p1"], 8)
        return outs

    return inputs, call


@scenario
def model():
    """The layer of case b with and without its conditional MLP, the embeddings and the 2-layer transformer with time
    (position_embeding through pd3_petr_coords3d) and the head with its decode, forced and unfused, built inside the run."""
    from paddle3d_amd import cape

    g = mk.load()
    i = cpu.tensors("b", DEV)
    ti = {k: torch.from_numpy(v).to(DEV) for k, v in mk.tr_inputs("b").items()}

    hargs = cpu.head_args("b", DEV)

    def call():
        outs = {}
        for fused in ("force", False):
            for name in ("cva", "cva0"):
                layer = cpu.build(g, "b", name, fused).to(DEV)
                with torch.no_grad():
                    outs[f"{name}_{fused}"] = layer(i["x"], i["bev_embed"], i["lidar_obj_pe"], i["feature"], i["camera_pe"],
                                                    i["mask"], i["img_embed"], i["bev_embed"], None)
            outs[f"pe_{fused}"] = cape.world_posemb3d(i["ref_points"], mk.BOUND, i["R"], i["t"], 8, fused=fused)
            outs[f"pe0_{fused}"] = cape.pos2posemb3d(i["ref_points"], mk.POS_FEATS, fused=fused)
            tr = cpu.build_transformer(g, "b", fused).to(DEV)
            with torch.no_grad():
                ego = cape.curlidar2prevlidar(ti["ext_cur"].T, ti["ext_prev"].T)
                outs[f"tr_{fused}"] = tr(ti["feature"], ti["mask"], ti["I_inv"], ti["R_inv"], ti["t"], mk.TR["image"],
                                         ego_matrix=ego)[0]
                head = cpu.build_head(g, "b", fused).to(DEV)
                preds = head(*hargs)
                det = head.get_bboxes(preds)
            outs.update({f"hcls_{fused}": preds["all_cls_scores"], f"hbox_{fused}": preds["all_bbox_preds"]})
            outs.update({f"{k}_{fused}": v for k, v in zip(("boxes", "scores", "labels", "count"), det)})
        return outs

    return dict(i, hfeat=hargs[0][0], hintr=hargs[1], hext=hargs[2], **{"tr_" + k: v for k, v in ti.items()}), call


@pytest.mark.parametrize("name", list(P.scenarios))
def test_scenario(name):
    P.check_scenario(name)


def test_every_launching_entry_point_is_exercised():
    """Runs last; scenarios that did not run in this process are run here in their plain form."""
    from paddle3d_amd import _lib

    P.check_complete(_lib.symbols("test_memory_safety_cape_gpu"), 2)
