"""The statuses the hard_voxelize and PillarFeatureNet entry points answer a bad call with, and which one wins when two
things are wrong, through the C ABI (the way tests/voxel_lattice.py's run_raw calls it).  The order of the checks is part of
the contract: null pointers, numeric ranges, the grid and the path selector, then the workspace size (csrc/voxelize.hip);
ranges, the empty case, null pointers, then the supported shapes (csrc/pfn.hip).  No case gets as far as a launch.

The case: 2 frames of 64 points, D = 4, voxel size (0.5, 0.5, 8) over (0, 0, -3, 8, 8, 5), P = 4, V = 32."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
B, N, D, P, V = 2, 64, 4, 4, 32
VS, PR = (0.5, 0.5, 8.0), (0.0, 0.0, -3.0, 8.0, 8.0, 5.0)
KINDS = ["path", "index", "f64"]
POINTERS = {"path": ["pts", "voxels", "coords", "npv", "nv", "ws"],
            "index": ["pts", "span", "plist", "coords", "npv", "nv", "ws"],
            "f64": ["pts", "voxels", "coords", "npv", "nv", "ws"]}


def _ws_bytes(**kw):
    from paddle3d_amd.ops._common import host_f32, lib, ptr

    a = dict(batch=B, n=N, d=D, vs=VS, p=P, v=V)
    a.update(kw)
    return lib().pd3_hard_voxelize_workspace(a["batch"], a["n"], a["d"], ptr(host_f32(a["vs"], 3)), ptr(host_f32(PR, 6)),
                                             a["p"], a["v"])


@pytest.fixture(scope="module")
def bufs():
    """Device buffers of the full size of the case for every argument, so that a call which did go on would stay in bounds."""
    dev = torch.device("cuda")
    need = _ws_bytes()
    assert need > 1
    t = {"pts": torch.zeros(B, N, D, dtype=torch.float64, device=dev),
         "voxels": torch.zeros(B, V, P, D, dtype=torch.float64, device=dev),
         "coords": torch.zeros(B, V, 3, dtype=torch.int32, device=dev),
         "npv": torch.zeros(B, V, dtype=torch.int32, device=dev),
         "nv": torch.zeros(B, dtype=torch.int32, device=dev),
         "span": torch.zeros(B, V, 2, dtype=torch.int32, device=dev),
         "plist": torch.zeros(B * N + 4, dtype=torch.int32, device=dev),
         "ws": torch.zeros(need + 256, dtype=torch.uint8, device=dev)}
    return t, need


def vox(kind, bufs, null=None, ws_short=0, **kw):
    """The status of pd3_hard_voxelize_{path, index, f64} on the case with the named changes."""
    from paddle3d_amd.ops._common import host_f32, lib, ptr, stream_ptr

    t, need = bufs
    a = dict(batch=B, n=N, d=D, vs=VS, p=P, v=V, path=0)
    a.update(kw)
    g = lambda k: None if k == null else ptr(t[k])  # noqa: E731
    vs, pr = host_f32(a["vs"], 3), host_f32(PR, 6)
    head = [g("pts"), None, a["batch"], a["n"], a["d"], ptr(vs), ptr(pr), a["p"], a["v"]]
    tail = [g("coords"), g("npv"), g("nv"), None, g("ws"), need - ws_short, stream_ptr(t["ws"].device)]
    L = lib()
    if kind == "path":
        return L.pd3_hard_voxelize_path(*head, g("voxels"), *tail, a["path"])
    if kind == "index":
        return L.pd3_hard_voxelize_index(*head, g("span"), g("plist"), *tail)
    return L.pd3_hard_voxelize_f64(*head, g("voxels"), *tail)


@pytest.mark.parametrize("kind", KINDS)
def test_voxelize_null_pointers(kind, bufs):
    for name in POINTERS[kind]:
        assert vox(kind, bufs, null=name) == EINVAL, name


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("change", [dict(batch=0), dict(n=0), dict(n=1 << 31), dict(d=2), dict(p=0), dict(v=0),
                                    dict(vs=(0.5, 0.0, 8.0))], ids=lambda c: "-".join(c))
def test_voxelize_ranges(kind, change, bufs):
    assert vox(kind, bufs, **change) == EINVAL


@pytest.mark.parametrize("path", [-1, 18])
def test_voxelize_path_range(path, bufs):
    assert vox("path", bufs, path=path) == EINVAL


@pytest.mark.parametrize("kind", KINDS)
def test_voxelize_short_workspace(kind, bufs):
    assert vox(kind, bufs, ws_short=1) == EWORKSPACE


def test_voxelize_precedence(bufs):
    assert vox("path", bufs, path=18, ws_short=1) == EINVAL
    for kind in KINDS:
        assert vox(kind, bufs, null="coords", ws_short=1) == EINVAL, kind


def test_voxelize_workspace_of_bad_sizes():
    assert _ws_bytes(batch=0) == 0
    assert _ws_bytes(vs=(0.5, 0.0, 8.0)) == 0


# ---- PillarFeatureNet ---------------------------------------------------------------------------------------------------
M, MAXP = 32, 8  # pillars, points per pillar


@pytest.fixture(scope="module")
def pfn_bufs():
    dev = torch.device("cuda")
    f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)  # noqa: E731
    i = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)  # noqa: E731
    return {"voxels": f(M, MAXP, D), "num": i(M), "coors": i(M, 4), "w1": f(16, 68), "s1": f(68), "b1": f(68),
            "w2": f(2 * 68, 64), "s2": f(64), "b2": f(64), "out": f(M, 64), "pts": f(2, N, D), "span": i(M, 2),
            "plist": i(2 * N + 4)}


def pfn_path(t, m=M, center_dims=3, c1=32, c2=64, path=0, null=False):
    from paddle3d_amd.ops._common import lib, ptr, stream_ptr

    g = lambda k: None if null else ptr(t[k])  # noqa: E731
    return lib().pd3_pillar_feature_net_path(g("voxels"), g("num"), g("coors"), m, MAXP, D, center_dims, 0.5, 0.5, 8.0, 0.25,
                                             0.25, 1.0, g("w1"), g("s1"), g("b1"), c1, g("w2"), g("s2"), g("b2"), c2,
                                             g("out"), path, stream_ptr(t["out"].device))


def pfn_indexed(t, m=M, per_frame=M // 2, list_stride=N, n=N):
    from paddle3d_amd.ops._common import lib, ptr, stream_ptr

    g = lambda k: ptr(t[k])  # noqa: E731
    return lib().pd3_pillar_feature_net_indexed(g("pts"), n, g("span"), g("plist"), list_stride, g("coors"), m, per_frame, MAXP,
                                                D, 3, 0.5, 0.5, 8.0, 0.25, 0.25, 1.0, g("w1"), g("s1"), g("b1"), 32, g("w2"),
                                                g("s2"), g("b2"), 64, g("out"), stream_ptr(t["out"].device))


def test_pfn_path_statuses(pfn_bufs):
    assert pfn_path(pfn_bufs, path=3) == EINVAL
    assert pfn_path(pfn_bufs, center_dims=4) == EINVAL
    assert pfn_path(pfn_bufs, m=0, null=True) == 0  # the empty case wins over the null check
    assert pfn_path(pfn_bufs, c1=68) == EUNSUPPORTED
    assert pfn_path(pfn_bufs, c1=16, path=2) == EUNSUPPORTED  # a shape the packed form refuses


def test_pfn_indexed_statuses(pfn_bufs):
    chunk = 8  # kPkPillars: pillars per chunk of the packed kernel
    assert pfn_indexed(pfn_bufs, m=2 * (chunk + 1), per_frame=chunk + 1) == EUNSUPPORTED
    assert pfn_indexed(pfn_bufs, list_stride=0) == EINVAL
    assert pfn_indexed(pfn_bufs, m=0) == 0
    # a span's start (a position in the list row) travels in 24 bits: a list row that long, and a frame whose points such a
    # row could not name once each, are refused before anything is read
    assert pfn_indexed(pfn_bufs, n=1 << 24) == EUNSUPPORTED
    assert pfn_indexed(pfn_bufs, list_stride=1 << 24) == EUNSUPPORTED
    assert pfn_indexed(pfn_bufs, n=1 << 24, list_stride=0) == EINVAL  # ranges before shapes
    assert pfn_indexed(pfn_bufs) == 0  # the case itself is served (all spans empty: zeros out)
