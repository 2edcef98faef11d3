"""The reload test of tests/test_derived_cpu.py through the packed paths: a module runs once (its weights are packed
for the kernel), takes a twin's parameters through `load_state_dict` and runs again; the second result is the twin's
own, bit for bit, and not the first one.  Shapes: the smallest the modules' own tests use."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from test_derived_cpu import randomise, same, tensors  # noqa: E402

from paddle3d_amd.derived import invalidate_derived  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def reload_is_seen(make, run, what=""):
    """make(seed) -> a module on the device with seeded parameters; run(module) -> its outputs (tensors, nested)."""
    m, twin = make(1), make(2)
    for mod in (m, twin):
        assert not mod.training
    with torch.no_grad():
        first = [t.clone() for t in tensors(run(m))]
        m.load_state_dict(twin.state_dict())
        got = [t.clone() for t in tensors(run(m))]
        want = tensors(run(twin))
    assert first and same(got, want), f"{what}: stale derived weights after load_state_dict"
    assert not same(first, got), f"{what}: the twin computes what the module computed before"
    return m


# ---- SMOKE --------------------------------------------------------------------------------------------------------------
def test_smoke_stacked_winograd_weight():
    from paddle3d_amd import smoke as S
    from paddle3d_amd.ops import conv

    cin, c, h, w = 8, 32, 5, 7  # the smallest predictor of test_smoke_gpu: 8 -> 2 x 32 on a 5 x 7 map
    assert conv.winograd43_supported(cin, 2 * c, h, w)
    x = torch.randn(1, cin, h, w, generator=torch.Generator().manual_seed(0)).to(DEV)

    def make(seed):
        return randomise(S.SMOKEPredictor(num_classes=3, num_channels=c, in_channels=cin, conv_kernel="winograd43"),
                         seed).to(DEV).eval()

    reload_is_seen(make, lambda m: m(x), "SMOKEPredictor")


# ---- DD3D ---------------------------------------------------------------------------------------------------------------
def test_dd3d_tower_convolutions(monkeypatch):
    from paddle3d_amd import dd3d as D
    from paddle3d_amd.ops import conv

    shapes, strides, C = ((12, 40), (5, 7)), (8, 16), 32  # test_winograd_towers_on_request
    gen = torch.Generator().manual_seed(0)
    feats = [torch.randn(2, C, h, w, generator=gen).to(DEV) for h, w in shapes]

    def make(seed):
        return randomise(D.FCOS2DHead(list(strides), [C] * 2, num_classes=3, norm="FrozenBN", num_cls_convs=2,
                                      num_box_convs=2, conv_kernel="winograd43"), seed).to(DEV).eval()

    head = reload_is_seen(make, lambda m: m.towers(feats), "FCOS2DHead towers")
    # after invalidate_derived every tower convolution packs again, once (not once per level)
    packs = []
    pack = conv.pack_winograd43_weight
    monkeypatch.setattr(conv, "pack_winograd43_weight", lambda *a, **k: packs.append(1) or pack(*a, **k))
    with torch.no_grad():
        before = [t.clone() for t in tensors(head.towers(feats))]
        assert not packs
        invalidate_derived(head)
        after = tensors(head.towers(feats))
        assert len(packs) == sum(isinstance(m, D._TowerConv) for m in head.modules()) == 4
        head.towers(feats)
    assert len(packs) == 4 and same(before, after)


def _dd3d_randomise(model, seed):
    """Convolutions at He scale, biases of a tenth, every Scale / Offset within a quarter of its initial value."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.dim() == 4:
                p.copy_(torch.randn(p.shape, generator=gen) * math.sqrt(2.0 / (9 * p.shape[1])))
            elif ".scales_" in name or ".offsets_" in name:
                p.mul_(float(torch.rand((), generator=gen)) * 0.5 + 0.75)
            else:
                p.copy_(torch.randn(p.shape, generator=gen) * 0.1)
    return model


def test_dd3d_lazy_predictor_arrays():
    from paddle3d_amd import dd3d as D
    import test_dd3d_gpu as gpu
    from test_memory_safety_dd3d_gpu import POINTS

    shapes, strides, C, nc, _, _, B, cfg = POINTS[0]
    L = len(shapes)
    gen = torch.Generator().manual_seed(0)
    feats = [torch.randn(B, C, h, w, generator=gen).to(DEV) for h, w in shapes]
    K = torch.from_numpy(gpu.sweep_camera(B)).to(DEV)

    def make(seed):
        head2 = D.FCOS2DHead(list(strides), [C] * L, num_classes=nc, num_cls_convs=2, num_box_convs=2, norm="FrozenBN")
        inf2 = D.FCOS2DInference(pre_nms_thresh=cfg["pre_nms_thresh"], pre_nms_topk=cfg["pre_nms_topk"],
                                 post_nms_topk=cfg["post_nms_topk"], nms_thresh=cfg["nms_thresh"], num_classes=nc)
        head3 = D.FCOS3DHead(list(strides), [C] * L, num_classes=nc, num_convs=2, norm="FrozenBN")
        inf3 = D.FCOS3DInference(num_classes=nc)
        model = D.DD3D(None, "none", None, head2, inf2, head3, inf3, do_nms=True, num_classes=nc,
                       input_strides=strides)
        return _dd3d_randomise(model, seed).to(DEV).eval()

    def run(m):
        assert m.device_supported(feats)
        rows, counts = m.head_padded(feats, K, fused="lazy")
        assert int(counts.sum()) > 0
        return rows, counts

    reload_is_seen(make, run, "DD3D.packed")


# ---- SqueezeSegV3 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["InvertedResidual", "DecoderStage"])
def test_squeezeseg_conv3x3_layers(which):
    from paddle3d_amd import squeezesegv3 as sq

    C, h, w = 32, 4, 8  # 32 -> 32 is in DEFAULT_CONV3X3: the F(2x2, 3x3) Winograd kernel
    assert sq.conv3x3_kernel_for("auto", C, C, h, w, DEV) == "winograd"
    x = torch.randn(1, C, h, w, generator=torch.Generator().manual_seed(0)).to(DEV)

    def make(seed):
        m = sq.InvertedResidual([C, C]) if which == "InvertedResidual" else sq.DecoderStage(C, C, upsample=False)
        return randomise(m, seed).to(DEV).eval()

    reload_is_seen(make, lambda m: m(x), which)


def test_squeezeseg_sac_block():
    from paddle3d_amd import squeezesegv3 as sq

    C, h, w = 32, 4, 9
    gen = torch.Generator().manual_seed(0)
    xyz, feature = torch.randn(1, 3, h, w, generator=gen).to(DEV), torch.randn(1, C, h, w, generator=gen).to(DEV)

    def make(seed):
        return randomise(sq.SACISKBlock(C), seed).to(DEV).eval()

    def run(m):
        assert m.takes_kernel(feature)
        return m(xyz, feature)[1]

    reload_is_seen(make, run, "SACISKBlock")


# ---- IA-SSD -------------------------------------------------------------------------------------------------------------
def test_iassd_fused_scale():
    from paddle3d_amd import iassd

    key = min(iassd.MEASURED_FASTER)  # (16, 16, 32, 16)
    gen = torch.Generator().manual_seed(0)
    xyz, feats = (torch.rand(2, 100, 3, generator=gen) * 4).to(DEV), torch.randn(2, 2, 100, generator=gen).to(DEV)

    def make(seed):
        m = iassd.SAModuleMSG_WithSampling(npoint=16, sample_range=-1, sample_type="D-FPS", radii=[0.9], nsamples=[key[3]],
                                           mlps=[[2, *key[:3]]], aggregation_mlp=[32], confidence_mlp=[16], num_classes=3,
                                           fused="force")
        return randomise(m, seed).to(DEV).eval()

    def run(m):
        assert m.scale_is_fused(0, 100)
        return m(xyz, feats)[1:]

    reload_is_seen(make, run, "SAModuleMSG_WithSampling")


# ---- sparse convolutions ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", ["f16", "bf16x3"])
def test_sparse_packed_weight(pipe):
    from paddle3d_amd import sparse as S
    from paddle3d_amd.ops import sparse_conv3d as sp
    from test_sparse_conv_gpu import _random_sparse

    cin, cout = (16, 32) if pipe == "f16" else (16, 64)
    assert sp.f16_supported(cin, cout, 27) if pipe == "f16" else (sp.SPLIT_BF16 and sp.bf16x3_pays(cin, cout, 27))
    shape, batch = (4, 16, 16), 1
    coords, feats = _random_sparse(np.random.default_rng(0), batch, shape, 300, cin)
    coords, feats = torch.from_numpy(coords).to(DEV), torch.from_numpy(feats).to(DEV)

    def make(seed):
        return randomise(S.SubmConv3D(cin, cout, 3, key="k"), seed).to(DEV).eval()

    def run(m):
        return m(S.SparseConvTensor(feats, coords, shape, batch, amp=(pipe == "f16"))).features.float()

    reload_is_seen(make, run, f"SubmConv3D {pipe}")
