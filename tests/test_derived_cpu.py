"""paddle3d_amd/derived.py on the CPU: the one rule for every derived weight (kept with the signature of the tensors it
was built from, rebuilt when that differs, `invalidate_derived` after a `.data` write), first on a two-layer Sequential,
then through every derivation of the package that is plain torch: after `load_state_dict` with a twin's parameters the
derived value is the twin's, not the one built before the load."""
import os
import sys

import pytest
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from paddle3d_amd import derived as dv  # noqa: E402
from paddle3d_amd.derived import derived, invalidate_derived, slots  # noqa: E402


def randomise(module, seed):
    """Seeded values for every parameter and every BatchNorm statistic (the constructors leave mean 0, variance 1)."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.3)
        for m in module.modules():
            if isinstance(m, nn.modules.batchnorm._BatchNorm):
                m.weight.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
                m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.3)
                m.running_var.copy_(torch.rand(m.num_features, generator=gen) * 1.5 + 0.5)
    return module


def tensors(value):
    """The tensors of a derived value (nested tuples / lists / dicts; everything else is dropped), in order."""
    if isinstance(value, torch.Tensor):
        return [value]
    if isinstance(value, dict):
        value = list(value.values())
    if isinstance(value, (tuple, list)):
        return [t for v in value for t in tensors(v)]
    return []


def same(a, b):
    a, b = tensors(a), tensors(b)
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


# ---- derived() itself ---------------------------------------------------------------------------------------------------
class Counter:
    def __init__(self, net):
        self.net, self.calls, self.grad = net, 0, None

    def __call__(self):
        self.calls += 1
        self.grad = torch.is_grad_enabled()
        return self.net[0].weight.detach() * 2


def two_layers():
    return nn.Sequential(nn.Linear(3, 4), nn.Linear(4, 2))


def test_builds_once_and_again_after_a_write_a_load_or_another_key():
    net = two_layers()
    build = Counter(net)
    first = derived(net, "w", build)
    assert derived(net, "w", build) is first and build.calls == 1
    with torch.no_grad():
        net[1].bias.mul_(2.0)
    second = derived(net, "w", build)
    assert second is not first and build.calls == 2 and derived(net, "w", build) is second
    net.load_state_dict(randomise(two_layers(), 1).state_dict())
    third = derived(net, "w", build)
    assert build.calls == 3 and torch.equal(third, net[0].weight * 2) and not torch.equal(third, second)
    assert derived(net, "w", build, key="cpu") is not third and build.calls == 4
    assert derived(net, "w", build, key="cpu") is derived(net, "w", build, key="cpu") and build.calls == 4
    derived(net, "w", build)  # the key changed back: one value per slot
    assert build.calls == 5
    derived(net, "other", build)  # another slot of the same owner: its own value, the first one stays
    assert build.calls == 6 and set(slots(net)) == {"w", "other"}
    derived(net, "w", build)
    assert build.calls == 6


def test_sources_narrow_what_is_watched():
    net = two_layers()
    build = Counter(net)
    derived(net, "w", build, sources=net[0])
    with torch.no_grad():
        net[1].weight.mul_(2.0)
    derived(net, "w", build, sources=net[0])
    assert build.calls == 1
    with torch.no_grad():
        net[0].bias.add_(1.0)
    derived(net, "w", build, sources=net[0])
    assert build.calls == 2
    # a tensor, None and nested iterables are sources too
    derived(net, "t", build, sources=(net[0].weight, None, [net[1].bias]))
    with torch.no_grad():
        net[0].bias.add_(1.0)
    derived(net, "t", build, sources=(net[0].weight, None, [net[1].bias]))
    assert build.calls == 3
    with torch.no_grad():
        net[1].bias.add_(1.0)
    derived(net, "t", build, sources=(net[0].weight, None, [net[1].bias]))
    assert build.calls == 4
    assert dv.signature(None) == () and len(dv.signature(net)) == 4 and len(dv.signature([net[0], net[1].bias])) == 3


def test_a_data_write_waits_for_invalidate_derived():
    net = two_layers()
    build = Counter(net)
    first = derived(net, "w", build)
    net[0].weight.data.mul_(3.0)
    assert derived(net, "w", build) is first and build.calls == 1  # stale: the documented limit
    assert invalidate_derived(net) is net and not slots(net)
    assert torch.equal(derived(net, "w", build), net[0].weight * 2) and build.calls == 2


def test_build_runs_without_grad_and_the_slots_are_not_state():
    net = two_layers()
    keys = list(net.state_dict())
    build = Counter(net)
    with torch.enable_grad():
        value = derived(net, "w", build)
    assert build.grad is False and not value.requires_grad
    derived(net[1], "w", build)
    assert list(net.state_dict()) == keys and len(list(net.parameters())) == 4 and not list(net.buffers())
    assert len(list(net.modules())) == 3
    dv.drop(net[1])
    assert not slots(net[1]) and slots(net)  # drop: the owner alone


def test_train_drops_the_slots_of_an_inference_cache_module():
    class Layer(dv.InferenceCache, nn.Linear):
        pass

    m = Layer(2, 2).eval()
    derived(m, "w", lambda: m.weight.detach().clone())
    assert slots(m)
    m.train()
    assert not slots(m)
    with pytest.raises(RuntimeError, match="eval"):
        m._require_eval()
    m.eval()._require_eval()
    derived(m, "w", lambda: m.weight.detach().clone())
    assert m.invalidate() is m and not slots(m)


# ---- the package's pure-torch derivations: a reload is seen ---------------------------------------------------------
def _pfn():
    from paddle3d_amd import centerpoint as cpm

    m = cpm.PillarFeatureNet(4, (8, 16), voxel_size=(0.2, 0.2, 4), point_cloud_range=(0, -4, -3, 8, 4, 1))
    return m, m._weights


def _sparse_bn():
    from paddle3d_amd import sparse

    m = nn.BatchNorm1d(8, eps=1e-3)
    return m, lambda: sparse._fold(m)


def _sa_module():
    from paddle3d_amd import iassd

    m = iassd.SAModuleMSG_WithSampling(npoint=8, sample_range=-1, sample_type="D-FPS", radii=[0.5, 1.0], nsamples=[16, 16],
                                       mlps=[[1, 16, 16, 32], [1, 16, 16, 16]], aggregation_mlp=[32], confidence_mlp=[16],
                                       num_classes=3)
    return m, m._fold


def _iassd_head():
    from paddle3d_amd import iassd

    coder = dict(use_mean_size=True, mean_size=[[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]])
    m = iassd.IASSD_Head(32, [16], [16], 3, {"box_coder_config": coder})
    return m, m._fold


def _conv_bn_layer():
    from paddle3d_amd import squeezesegv3 as sq

    m = sq.ConvBNLayer(4, 8, 3, padding=1)
    return m, m.folded


def _sac_block():
    from paddle3d_amd import squeezesegv3 as sq

    m = sq.SACISKBlock(24)  # 24 channels: the fused kernel refuses, nothing is packed, no library call
    return m, m._params


@pytest.mark.parametrize("make", [_pfn, _sparse_bn, _sa_module, _iassd_head, _conv_bn_layer, _sac_block],
                         ids=lambda f: f.__name__.strip("_"))
def test_a_reload_is_seen(make):
    (m, derive), (twin, derive_twin) = make(), make()
    randomise(m.eval(), 1)
    randomise(twin.eval(), 2)
    first = derive()
    assert derive() is first and tensors(first)
    kept = [t.clone() for t in tensors(first)]
    m.load_state_dict(twin.state_dict())
    second, want = derive(), derive_twin()
    assert same(second, want)
    assert not same(second, kept)


def test_pfn_rebuilds_on_every_call_in_training_mode():
    m, derive = _pfn()
    m.eval()
    assert all(a is b for a, b in zip(derive(), derive()))
    m.train()
    assert not any(a is b for a, b in zip(derive(), derive()))


# ---- invalidate_derived reaches every module ----------------------------------------------------------------------------
def _models():
    from paddle3d_amd import centerpoint as cpm
    from paddle3d_amd import iassd, pointpillars, two_stage
    from paddle3d_amd import squeezesegv3 as sq
    import test_dd3d_cpu
    import test_smoke_cpu

    yield "centerpoint_pillars", cpm.centerpoint_pillars_nuscenes(max_num_voxels=(100, 100))
    yield "centerpoint_voxels", cpm.centerpoint_voxels_kitti(max_num_voxels=(100, 100))
    yield "pointpillars", pointpillars.pointpillars_kitti_car(max_num_voxels=(100, 100))
    yield "voxel_rcnn", two_stage.voxel_rcnn_005voxel_kitti_car()
    yield "iassd", iassd.iassd_kitti()
    yield "squeezesegv3", sq.SqueezeSegV3(sq.SACRangeNet(5, 21))
    yield "smoke", test_smoke_cpu.build_model("gn32")
    yield "dd3d", test_dd3d_cpu.build_model("v2_l5")


def test_invalidate_derived_leaves_no_slot_below_a_model():
    for name, model in _models():
        mods = list(model.modules())
        for m in mods:  # a slot on every module, the ones this package does not define included
            derived(m, "sentinel", lambda: ("sentinel",))
        assert all(slots(m) for m in mods), name
        assert invalidate_derived(model) is model
        held = [type(m).__name__ for m in mods if slots(m)]
        assert not held, (name, held)
        assert not any(k.endswith(dv._SLOTS) or "sentinel" in k for k in model.state_dict()), name
