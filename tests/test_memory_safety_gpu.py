"""Every device op under guarded allocations: no store outside an output or a workspace, no result that depends on what
a buffer held before, no write to an input (tests/guarded.py has the harness, tests/test_guarded_cpu.py its self-test).

A SCENARIO is a function that builds its inputs (seeded) and returns `(inputs, call)`; `call()` runs the library through
its Python wrappers and model classes (the four entry points without a wrapper through the ctypes handle, with outputs
from `torch.empty` like the wrappers') and returns the dict of SPECIFIED results.  Where include/paddle3d_amd.h defines
only part of a buffer, the scenario slices by the count the op itself returns and quotes the header line; a buffer the
header calls zero padded / fully written is returned whole.

Each scenario runs three times in one process -- plain, guarded with fill 0x00, guarded with fill 0xFF (fp NaN, int32
-1 = this code base's "no neighbour") -- and the test asserts: no guard band damaged; every specified output bit-equal
across the three runs (the two float-atomic gradients that are documented as order dependent compare under their own
test's tolerance, see TOLERANT); every input bit-equal to its clone; outputs not trivial.  Model scenarios construct
the model inside the run, so packed weights, plans and cached workspaces are allocated under the guard too.

The last test asserts that the scenarios reach every kernel-launching entry point of the C ABI.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from guarded import Protocol  # noqa: E402

from paddle3d_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32

# outputs compared under a tolerance instead of bit for bit: (scenario, output suffix) -> {dtype: relative bound (of
# max(|reference|, 1))}.  ms_deform_attn's grad_value is accumulated with float atomics ("may differ in the last bits from
# run to run", paddle3d_amd.h); the bounds are the ones tests/test_ms_deform_attn_gpu.py::
# test_edges_and_non_finite_locations holds it to against the restatement (`tol = 1e-4 if dtype == np.float32 else
# 1e-10`).  Every other float-atomic gradient here (gather / grouping) is fed small integers, whose fp32 sums are
# exact in any order, and compares bit for bit; assign_score_withk's backward has no atomics (its own test:
# test_backward_reproducible) and is exact as well.
TOLERANT = {("ms_deform_attn", "grad_value"): {torch.float32: 1e-4, torch.float64: 1e-10}}


def _probe_lds_atomic_order():
    """The self-check is probed once per process: keep its launch out of whichever scenario runs first."""
    from paddle3d_amd.ops import voxelize

    voxelize.lds_atomic_order_ok(DEV)


P = Protocol("test_memory_safety_gpu", "memory-safety", DEV, tolerant=TOLERANT, before_pass=_probe_lds_atomic_order,
             may_allocate_nothing={"selfcheck_lds_atomic_order"})
scenario = P.scenario


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _lib():
    from paddle3d_amd.ops._common import check, lib, ptr, stream_ptr

    return lib(), check, ptr, stream_ptr(DEV)


def _count(t):
    """The host value of a device count an op returned (the scenario slices by it)."""
    return [int(v) for v in t.reshape(-1).tolist()]


# ---------------------------------------------------------------------------------------------------------------------
# voxelization
def _vox_points(frames=3, n=20000, d=5, seed=3):
    pts = np.stack([synth.nuscenes_sweep(seed + i, n_points=n) for i in range(frames)])[:, :, :d].copy()
    lens = np.array([n, n * 2 // 3 + 1, 0][:frames], np.int32)  # ragged, the last frame empty
    return pts, lens


def _vox_paths(name, paths, vs, pr, p, v):
    """hard_voxelize_batch on every `path`.  The shapes are chosen so that EVERY listed form takes them: a forced form
    that answers PD3_EUNSUPPORTED here has fallen out of coverage and fails the scenario.  All five outputs whole: "zero
    padded" / "batch = -1 on padding rows"."""
    from paddle3d_amd._lib import Paddle3DAmdError
    from paddle3d_amd.ops import voxelize

    pts, lens = _vox_points()
    inputs = dict(points=_t(pts), num_points=_t(lens))

    def call():
        outs, ran = {}, []
        for path in paths:
            try:
                r = voxelize.hard_voxelize_batch(inputs["points"], list(vs), list(pr), p, v, inputs["num_points"],
                                                 with_batch_coors=True, path=path)
            except Paddle3DAmdError as e:
                assert "status -3" in str(e) and path >= 2, (path, e)
                continue
            ran.append(path)
            nv = _count(r[3])
            assert 0 < nv[0] < v and 0 < nv[1] < v and nv[2] == 0, nv  # counts below the capacity: padding rows exist
            for k, o in zip(("voxels", "coords", "npv", "nv", "coors4"), r):
                outs[f"{k}_path{path}"] = o
        print(f"[memory-safety]   {name}: paths run {ran}", flush=True)
        assert ran == list(paths), f"{name}: forms {sorted(set(paths) - set(ran))} refused this shape (PD3_EUNSUPPORTED)"
        outs["paths_run"] = torch.tensor(ran)
        outs["__trivial_ok__"] = {"paths_run"}
        return outs

    return inputs, call


@scenario
def hard_voxelize_pillar_paths():
    return _vox_paths("pillar", [0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 17], synth.NUSC_PILLAR, synth.NUSC_RANGE,
                      20, 24000)


@scenario
def hard_voxelize_3d_paths():
    return _vox_paths("3d", [0, 1, 14, 15, 16], synth.NUSC_VOXEL, synth.NUSC_VOXEL_RANGE, 10, 24000)


@scenario
def hard_voxelize_capped_single_frame():
    """[N, D] form with D = 4 and more voxels than max_voxels (the cap cuts), P = 7 (row not a multiple of 4 floats)."""
    from paddle3d_amd.ops import voxelize

    pts = synth.kitti_frame(5, n_points=9001)[:, :4].copy()
    inputs = dict(points=_t(pts))

    def call():
        outs = {}
        for path in (0, 1):
            vox, co, npv, nv = voxelize.hard_voxelize(inputs["points"], list(synth.KITTI_PILLAR), list(synth.KITTI_RANGE),
                                                      7, 1000, path=path)
            assert _count(nv) == [1000]
            outs.update({f"voxels{path}": vox, f"coords{path}": co, f"npv{path}": npv, f"nv{path}": nv})
        return outs

    return inputs, call


@scenario
def hard_voxelize_f64():
    from paddle3d_amd.ops import voxelize

    pts, lens = _vox_points(frames=3, n=6000)
    inputs = dict(points=_t(pts.astype(np.float64)), num_points=_t(lens))

    def call():
        r = voxelize.hard_voxelize_batch(inputs["points"], list(synth.NUSC_PILLAR), list(synth.NUSC_RANGE), 20, 8000,
                                         inputs["num_points"], with_batch_coors=True)
        assert r[0].dtype == torch.float64 and 0 < _count(r[3])[0] < 8000
        return dict(zip(("voxels", "coords", "npv", "nv", "coors4"), r))

    return inputs, call


@scenario
def hard_voxelize_abi_entry():
    """pd3_hard_voxelize itself (the wrappers call the _path form): direct ABI call, outputs from torch.empty."""
    pts, lens = _vox_points(frames=2, n=5000)
    inputs = dict(points=_t(pts), num_points=_t(lens))

    def call():
        from paddle3d_amd.ops._common import host_f32, workspace

        L, check, ptr, stream = _lib()
        b, n, d = pts.shape
        p, v = 20, 6000
        vs, pr = host_f32(synth.NUSC_PILLAR, 3), host_f32(synth.NUSC_RANGE, 6)
        voxels = torch.empty((b, v, p, d), dtype=torch.float32, device=DEV)
        coords = torch.empty((b, v, 3), dtype=torch.int32, device=DEV)
        npv = torch.empty((b, v), dtype=torch.int32, device=DEV)
        nv = torch.empty((b,), dtype=torch.int32, device=DEV)
        ws = workspace(L.pd3_hard_voxelize_workspace(b, n, d, ptr(vs), ptr(pr), p, v), DEV)
        check(L.pd3_hard_voxelize(ptr(inputs["points"]), ptr(inputs["num_points"]), b, n, d, ptr(vs), ptr(pr), p, v,
                                  ptr(voxels), ptr(coords), ptr(npv), ptr(nv), None, ptr(ws), ws.numel(), stream),
              "hard_voxelize")
        assert 0 < _count(nv)[0] < v
        return dict(voxels=voxels, coords=coords, npv=npv, nv=nv)

    return inputs, call


def _index_rows(span, plist, nv, n):
    """The entries of point_list the spans of the real voxels name, frame after frame (everything else in point_list
    is scratch: "voxel v of frame b holds the points point_list[b * max_points + start + 0 .. count - 1]")."""
    span, plist = span.cpu().numpy(), plist.cpu().numpy()
    rows = []
    for b, k in enumerate(nv):
        for st, cnt in span[b, :k]:
            rows.append(plist[b * n + st: b * n + st + cnt])
    return torch.from_numpy(np.concatenate(rows) if rows else np.zeros(0, np.int32))


@scenario
def hard_voxelize_index_and_pfn_indexed():
    """pd3_hard_voxelize_index + pd3_pillar_feature_net_indexed on a ragged batch with an empty frame.  coords, counts,
    num_voxels, coors and vox_span whole (padding rows: zeros, batch -1, span (0, 0)); point_list through the spans."""
    from paddle3d_amd.ops import voxel_encoder as ve
    from paddle3d_amd.ops import voxelize

    pts, lens = _vox_points()
    g = torch.Generator().manual_seed(11)
    w = dict(w1=torch.randn(10, 32, generator=g) * 0.3, s1=torch.randn(32, generator=g), b1=torch.randn(32, generator=g) * 0.1,
             w2=torch.randn(64, 64, generator=g) * 0.2, s2=torch.randn(64, generator=g), b2=torch.randn(64, generator=g) * 0.1)
    inputs = dict(points=_t(pts), num_points=_t(lens), **{k: v.to(DEV) for k, v in w.items()})

    def call():
        i = inputs
        vs, pr, v = list(synth.NUSC_PILLAR), list(synth.NUSC_RANGE), 24000
        got = voxelize.hard_voxelize_index_batch(i["points"], vs, pr, 20, v, i["num_points"])
        assert got is not None
        span, plist, coords, npv, nv, coors4 = got
        nvh = _count(nv)
        assert 0 < nvh[0] < v and nvh[2] == 0
        feats = ve.pillar_feature_net_indexed(i["points"], span, plist, coors4.view(-1, 4), 20, vs[0], vs[1],
                                              vs[0] / 2 + pr[0], vs[1] / 2 + pr[1], i["w1"], i["s1"], i["b1"], i["w2"],
                                              i["s2"], i["b2"])
        assert feats is not None
        return dict(span=span, listed=_index_rows(span, plist, nvh, pts.shape[1]), coords=coords, npv=npv, nv=nv,
                    coors4=coors4, pfn=feats)

    return inputs, call


@scenario
def dynamic_voxelize():
    from paddle3d_amd.ops import voxelize

    inputs = dict(points=_t(synth.nuscenes_sweep(9, n_points=10007)))

    def call():
        return dict(coors=voxelize.dynamic_voxelize(inputs["points"], list(synth.NUSC_VOXEL), list(synth.NUSC_VOXEL_RANGE)))

    return inputs, call


@scenario
def merge_sweeps():
    from paddle3d_amd.ops import sweeps

    rng = np.random.default_rng(4)
    frames = [rng.normal(0, 8, (n, 5)).astype(F32) for n in (1501, 700, 1, 333)]
    for f in frames[1:]:
        f[::7, :2] *= 0.01  # points inside sweep_remove_radius: dropped, so the count is below the row capacity
    mats = []
    for k in range(3):
        m = np.eye(4)
        m[:3, 3] = rng.normal(0, 1, 3)
        mats.append(m if k != 1 else None)
    inputs = {f"frame{k}": _t(f) for k, f in enumerate(frames)}

    def call():
        fr = [inputs[f"frame{k}"] for k in range(4)]
        out, n = sweeps.merge_sweeps(fr[0], fr[1:], mats, [0.05, 0.1, 0.15], return_count=True)
        k = _count(n)[0]
        assert 0 < k < out.shape[0]
        # "out [<= total points, ...] ... num_out [1]": rows past num_out are not part of the result
        return dict(points=out[:k], n=n)

    return inputs, call


# ---------------------------------------------------------------------------------------------------------------------
# voxel encoders, scatter
def _random_pillars(seed, m, p, d):
    rng = np.random.default_rng(seed)
    npv = rng.integers(0, p + 1, m).astype(np.int32)
    npv[:3] = [0, p, 1]
    vox = rng.normal(0, 5, (m, p, d)).astype(F32)
    vox[np.arange(p)[None, :] >= npv[:, None]] = 0
    co = np.stack([np.zeros(m), np.zeros(m), rng.integers(0, 512, m), rng.integers(0, 512, m)], 1).astype(np.int32)
    return vox, npv, co


def _pfn_weights(seed, d, c1, c2, extra=5):
    g = torch.Generator().manual_seed(seed)
    w = dict(w1=torch.randn(d + extra, c1, generator=g) * 0.3, s1=torch.randn(c1, generator=g),
             b1=torch.randn(c1, generator=g) * 0.1)
    if c2:
        w.update(w2=torch.randn(2 * c1, c2, generator=g) * 0.2, s2=torch.randn(c2, generator=g),
                 b2=torch.randn(c2, generator=g) * 0.1)
    return {k: v.to(DEV) for k, v in w.items()}


@scenario
def pillar_feature_net_forms():
    """All _PFN_FORMS of tests/test_scatter_pfn_gpu.py ((two layers, path)) at pillar counts that are not multiples of
    the packed form's chunk of 8, plus the HardVFE decoration (three centre dims) and the entry point without `path`."""
    from paddle3d_amd.ops import voxel_encoder as ve

    cases = [(20, 5, 1001), (32, 4, 3), (7, 4, 509)]
    inputs = {}
    for p, d, m in cases:
        vox, npv, co = _random_pillars(p * 10 + d, m, p, d)
        inputs.update({f"vox{p}": _t(vox), f"npv{p}": _t(npv), f"co{p}": _t(co)})
        inputs.update({f"two{p}_{k}": v for k, v in _pfn_weights(p, d, 32, 64).items()})
        inputs.update({f"one{p}_{k}": v for k, v in _pfn_weights(p + 1, d, 64, 0).items()})
        inputs.update({f"vfe{p}_{k}": v for k, v in _pfn_weights(p + 2, d, 64, 64, extra=6).items()})

    def call():
        L, check, ptr, stream = _lib()
        outs = {}
        i = inputs
        for p, d, m in cases:
            a = (i[f"vox{p}"], i[f"npv{p}"], i[f"co{p}"], 0.2, 0.2, -51.1, -51.1)
            for two, path in [(True, 0), (True, 1), (True, 2), (False, 0)]:
                w = {k.split("_", 1)[1]: v for k, v in i.items() if k.startswith(("two" if two else "one") + f"{p}_")}
                ws = [w["w1"], w["s1"], w["b1"]] + ([w["w2"], w["s2"], w["b2"]] if two else [])
                outs[f"pfn_p{p}_two{int(two)}_path{path}"] = ve.pillar_feature_net(*a, *ws, path=path)
            w = {k.split("_", 1)[1]: v for k, v in i.items() if k.startswith(f"vfe{p}_")}
            outs[f"vfe_p{p}"] = ve.hard_vfe(a[0], a[1], a[2], [0.2, 0.2, 8.0], list(synth.NUSC_RANGE), w["w1"], w["s1"],
                                            w["b1"], w["w2"], w["s2"], w["b2"])
            # pd3_pillar_feature_net (no path argument; the wrapper calls the _path form)
            w = {k.split("_", 1)[1]: v for k, v in i.items() if k.startswith(f"two{p}_")}
            out = torch.empty((m, 64), dtype=torch.float32, device=DEV)
            f = C.c_float
            check(L.pd3_pillar_feature_net(ptr(a[0]), ptr(a[1]), ptr(a[2]), m, p, d, 2, f(0.2), f(0.2), f(0.0), f(-51.1),
                                           f(-51.1), f(0.0), ptr(w["w1"]), ptr(w["s1"]), ptr(w["b1"]), 32, ptr(w["w2"]),
                                           ptr(w["s2"]), ptr(w["b2"]), 64, ptr(out), stream), "pillar_feature_net")
            outs[f"abi_p{p}"] = out
            outs[f"mean_p{p}"] = ve.voxel_mean(a[0], a[1])
        return outs

    return inputs, call


@scenario
def pointpillars_scatter_and_inverse_map():
    """Canvas "fully written (zero where no pillar)"; shapes (ny, nx, batch) = (40, 24, 1), (496, 432, 2), and an odd
    plane with a channel count that is not a multiple of 4; rows with a batch index outside [0, batch) are ignored."""
    from paddle3d_amd.ops import pointpillars_scatter as ps

    rng = np.random.default_rng(1)
    cases = [(40, 24, 1, 64, 300), (496, 432, 2, 64, 9000), (37, 41, 1, 7, 300)]
    inputs = {}
    for ny, nx, b, c, m in cases:
        cells = rng.choice(b * ny * nx, m, replace=False)
        c4 = np.stack([cells // (ny * nx), np.zeros(m), cells % (ny * nx) // nx, cells % nx], 1).astype(np.int32)
        c4[::50, 0] = -1
        inputs[f"f{ny}"] = _t(rng.normal(size=(m, c)).astype(F32))
        inputs[f"c{ny}"] = _t(c4)

    def call():
        outs = {}
        for ny, nx, b, c, m in cases:
            outs[f"canvas{ny}"] = ps.pointpillars_scatter(inputs[f"f{ny}"], inputs[f"c{ny}"], b, ny, nx)
            outs[f"inv{ny}"] = ps.inverse_map(inputs[f"c{ny}"], b, ny, nx)
        return outs

    return inputs, call


# ---------------------------------------------------------------------------------------------------------------------
# dense convolutions
def _conv_inputs(seed, n, cin, cout, h, w, wv=None, groups=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(n, cin, h, w)
    x[..., : (wv or w)] = torch.randn(n, cin, h, wv or w, generator=g)
    wt = torch.randn(cout, cin // groups, 3, 3, generator=g) / (9 * cin // groups) ** 0.5
    return x, wt, torch.randn(cout, generator=g)


@scenario
def conv3x3_fp32_family():
    """Direct, Winograd F(2,3), F(4,3) packed / ping-pong / pre-transformed, stride-2 direct and bf16x3 at maps that are
    not multiples of the kernels' tiles: (1, 8, 64, 6, 48), (3, 16, 128, 10, 36, wv = 34), (2, 64, 64, 9, 20)."""
    from paddle3d_amd.ops import conv

    cases = [(1, 8, 64, 6, 48, None), (3, 16, 128, 10, 36, 34), (2, 64, 64, 9, 20, None)]
    inputs = {}
    for k, (n, cin, cout, h, w, wv) in enumerate(cases):
        x, wt, b = _conv_inputs(k, n, cin, cout, h, w, wv)
        inputs.update({f"x{k}": x.to(DEV), f"w{k}": wt.to(DEV), f"b{k}": b.to(DEV)})

    def call():
        L, check, ptr, stream = _lib()
        outs = {}
        for k, (n, cin, cout, h, w, wv) in enumerate(cases):
            x, wt, b = inputs[f"x{k}"], inputs[f"w{k}"], inputs[f"b{k}"]
            outs[f"direct{k}"] = conv.conv3x3_bias_relu(x, conv.pack_conv3x3_weight(wt), b, cout, w_valid=wv)
            if h % 2 == 0:
                outs[f"direct_s2_{k}"] = conv.conv3x3_bias_relu(x, conv.pack_conv3x3_weight(wt), b, cout, stride=2,
                                                                w_valid=wv)
                if conv.conv3x3_s2_x3_supported(cin, cout, h, wv or w, n):
                    outs[f"s2_x3_{k}"] = conv.conv3x3_s2_x3_bias_relu(x, conv.pack_conv3x3_s2_x3_weight(wt), b, cout,
                                                                      w_valid=wv)
            if wv is None:
                outs[f"wino23_{k}"] = conv.conv3x3_winograd_bias_relu(x, conv.pack_winograd_weight(wt), b, cout)
            for tile in (32, 64):
                outs[f"wino43_t{tile}_{k}"] = conv.conv3x3_winograd43_bias_relu(
                    x, conv.pack_winograd43_weight(wt, tile), b, cout, w_valid=wv)
            ul = conv.pack_winograd43_lane_weight(wt)
            outs[f"wino43_pp_{k}"] = conv.conv3x3_winograd43_pp_bias_relu(x, ul, b, cout, w_valid=wv)
            if wv is None:  # the profiling entry: the same launch + cycle counters of one workgroup in dbg [8 waves][4]
                traced = torch.empty((n, cout, h, w), dtype=torch.float32, device=DEV)
                dbg = torch.empty((8, 4), dtype=torch.int64, device=DEV)  # cycle counts: guarded, not compared
                check(L.pd3_conv3x3_winograd43_pp_trace(ptr(x), ptr(ul), ptr(b), n, cin, cout, h, w, 1, ptr(traced), ptr(dbg),
                                                        stream), "conv3x3_winograd43_pp_trace")
                assert torch.equal(traced, outs[f"wino43_pp_{k}"])
                outs[f"wino43_trace_{k}"] = traced
            # (v_pre itself is an intermediate in the kernel's own tile order: the convolution that reads it is the output)
            v = conv.winograd43_input_transform(x, w_valid=wv)
            outs[f"wino43_ppv_{k}"] = conv.conv3x3_winograd43_ppv_bias_relu(v, x.shape, ul, b, cout, w_valid=wv)
        assert any(k.startswith("s2_x3_") for k in outs)
        return outs

    return inputs, call


@scenario
def conv_grouped_small():
    """The final SeparateHead convolutions: fp32 whole (pd3_grouped_conv3x3_small, direct ABI) and as a slice into a
    wider caller-owned map whose other groups must come back untouched.  The fp32 kernels take widths that are a
    multiple of 4 only ("requires cin_per_group % 4 == 0, w % 4 == 0": w = 33 answers PD3_EUNSUPPORTED before any launch,
    asserted below), so (n, groups, h) = (2, 4, 9) runs at w = 36 -- an odd height and neither a whole 8 x 128 tile;
    the width 33 of (2, 4, 9, 33) is what the fp16 forms run (conv_f16_family)."""
    from paddle3d_amd._lib import Paddle3DAmdError
    from paddle3d_amd.ops import conv

    n, groups, cg, co, h, w = 2, 4, 64, 4, 9, 36
    x, wt, b = _conv_inputs(7, n, groups * cg, groups * co, h, w, 33, groups=groups)
    inputs = dict(x=x.to(DEV), w=wt.to(DEV), b=b.to(DEV))

    def call():
        L, check, ptr, stream = _lib()
        wg = conv.pack_grouped_weight(inputs["w"], groups)
        whole = torch.empty((n, groups * co, h, w), dtype=torch.float32, device=DEV)
        check(L.pd3_grouped_conv3x3_small(ptr(inputs["x"]), ptr(wg), ptr(inputs["b"]), n, groups, cg, co, h, w, ptr(whole),
                                          stream), "grouped_conv3x3_small")
        wide = torch.full((n, (groups + 3) * co, h, w), 7.0, dtype=torch.float32, device=DEV)
        conv.grouped_conv3x3_small(inputs["x"], wg, inputs["b"], groups, out=wide, out_groups=groups + 3, out_group0=2)
        assert bool((wide[:, : 2 * co] == 7.0).all()) and bool((wide[:, (2 + groups) * co:] == 7.0).all())
        with pytest.raises(Paddle3DAmdError, match="status -3"):  # refused on the host: nothing is launched or written
            conv.grouped_conv3x3_small(inputs["x"][..., :33].contiguous(), wg, inputs["b"], groups)
        return dict(whole=whole, wide=wide, auto=conv.grouped_conv3x3_small(inputs["x"], wg, inputs["b"], groups))

    return inputs, call


@scenario
def conv_f16_family():
    """The AMP kernels: NCHW -> NHWC conversion with odd c, h, w; stride-1 fp16 in every out_mode, dual, stride-2 at
    (16, 128, 33, 45), grouped small on NHWC and on the group-major form."""
    from paddle3d_amd.ops import conv

    g = torch.Generator().manual_seed(3)
    inputs = dict(odd=torch.randn(2, 5, 7, 9, generator=g).to(DEV))
    cases = [(2, 16, 128, 33, 45), (1, 32, 64, 6, 50), (2, 64, 256, 9, 33)]
    for k, (n, cin, cout, h, w) in enumerate(cases):
        x, wt, b = _conv_inputs(20 + k, n, cin, cout, h, w)
        inputs.update({f"x{k}": x.to(DEV), f"w{k}": wt.to(DEV), f"b{k}": b.to(DEV)})
    _, wg, bg = _conv_inputs(30, 1, 256, 4 * 2, 3, 3, groups=4)
    inputs.update(wg=wg.to(DEV), bg=bg.to(DEV))

    def call():
        outs = dict(odd_nhwc=conv.to_f16_nhwc(inputs["odd"]))
        for k, (n, cin, cout, h, w) in enumerate(cases):
            assert conv.f16_supported(cin, cout, h, w)
            xh = conv.to_f16_nhwc(inputs[f"x{k}"])
            wt, b = inputs[f"w{k}"], inputs[f"b{k}"]
            outs[f"nhwc{k}"] = xh
            for tile in ((64, 128) if cout % 128 == 0 else (64,)):
                wp = conv.pack_conv3x3_f16_weight(wt, tile)
                outs[f"f16_t{tile}_{k}"] = conv.conv3x3_f16_bias_relu(xh, wp, b, cout)
                outs[f"f16_f32_t{tile}_{k}"] = conv.conv3x3_f16_bias_relu(xh, wp, b, cout, out_f32_nchw=True)
                outs[f"f16_gm_t{tile}_{k}"] = conv.conv3x3_f16_bias_relu(xh, wp, b, cout, group_major=True)
                oh, of = conv.conv3x3_f16_bias_relu_dual(xh, wp, b, cout)
                outs[f"dual_h_t{tile}_{k}"], outs[f"dual_f_t{tile}_{k}"] = oh, of
            if conv.s2_f16_supported(cin, cout):
                outs[f"s2_{k}"] = conv.conv3x3_s2_f16_bias_relu(xh, conv.pack_conv3x3_f16_weight(wt, 128), b, cout)
        # grouped small: the 256-channel first-stage output of the last case as 4 branches of 64 channels
        n, _, cout, h, w = cases[2]
        wgp = conv.pack_grouped_weight_f16(inputs["wg"], 4)
        wide = torch.full((n, 6 * 2, h, w), 7.0, dtype=torch.float32, device=DEV)
        conv.grouped_conv3x3_small_f16(outs["f16_t64_2"], wgp, inputs["bg"], 4, out=wide, out_groups=6, out_group0=1)
        assert bool((wide[:, :2] == 7.0).all()) and bool((wide[:, 10:] == 7.0).all())
        outs["grouped_nhwc_wide"] = wide
        outs["grouped_gm"] = conv.grouped_conv3x3_small_f16(outs["f16_gm_t64_2"], wgp, inputs["bg"], 4, group_major=True)
        assert "s2_0" in outs
        return outs

    return inputs, call


@scenario
def conv_patch_fpn_levels():
    """SecondFPN's patch convolutions, fp32-MFMA (modes 0 .. 3) and bf16x3 (modes 0 .. 2), each into a channel slice of a
    wider caller-owned map pre-filled with 7.0: the channels outside the slice come back unchanged."""
    from paddle3d_amd.ops import conv

    g = torch.Generator().manual_seed(8)

    def rnd(*s):
        return torch.randn(*s, generator=g)

    inputs = dict(x0=rnd(2, 16, 12, 64), w0=rnd(128, 16, 2, 2) / 8, b0=rnd(128),            # mode 0: Conv2D k2 s2
                  x1=rnd(2, 32, 6, 10), w1=rnd(128, 32, 1, 1) / 6, b1=rnd(128),             # mode 1: 1x1
                  x1b=rnd(2, 64, 6, 10), w1b=rnd(70, 64, 1, 1) / 8, b1b=rnd(70),            # mode 1, any cout
                  x2=torch.zeros(2, 32, 5, 12), w2=rnd(32, 64, 2, 2) / 6, b2=rnd(64),       # mode 2: deconv k2, wv = 10
                  x3=torch.zeros(2, 32, 5, 8), w3=rnd(32, 16, 4, 4) / 6, b3=rnd(16))        # mode 3: deconv k4, wv = 6
    inputs["x2"][..., :10] = rnd(2, 32, 5, 10)
    inputs["x3"][..., :6] = rnd(2, 32, 5, 6)
    inputs = {k: v.to(DEV) for k, v in inputs.items()}

    def call():
        outs = {}
        i = inputs

        def wide(cout, h, w):
            return torch.full((2, cout + 24, h, w), 7.0, dtype=torch.float32, device=DEV)

        def run(tag, fn, pack, x, wt, b, mode, tr, cout, out, wv=None):
            assert (conv.patch_x3_supported if "x3_" in tag else conv.patch_supported)(mode, x.shape[1], cout, x.shape[2],
                                                                                         x.shape[3]), tag
            fn(x, pack(wt, mode, tr), b, mode, cout, out, 16, relu=True, w_valid=wv)
            assert bool((out[:, :16] == 7.0).all()) and bool((out[:, 16 + cout:] == 7.0).all()), tag
            outs[tag] = out

        for kind, fn, pack in (("mfma", conv.patch_conv_bias_relu, conv.pack_patch_weight),
                               ("x3_", conv.patch_conv_x3_bias_relu, conv.pack_patch_weight_x3)):
            run(kind + "mode0", fn, pack, i["x0"], i["w0"], i["b0"], 0, False, 128, wide(128, 6, 32))
            run(kind + "mode1", fn, pack, i["x1"], i["w1"], i["b1"], 1, False, 128, wide(128, 6, 10))
            run(kind + "mode2", fn, pack, i["x2"], i["w2"], i["b2"], 2, True, 64, wide(64, 10, 20), wv=10)
        run("mfma_mode1_cout70", conv.patch_conv_bias_relu, conv.pack_patch_weight, i["x1b"], i["w1b"], i["b1b"], 1, False,
            70, wide(70, 6, 10))
        run("mfma_mode3", conv.patch_conv_bias_relu, conv.pack_patch_weight, i["x3"], i["w3"], i["b3"], 3, True, 16,
            wide(16, 20, 24), wv=6)
        return outs

    return inputs, call


@scenario
def scatter_conv_fused():
    """PointPillarsScatter fused into the stride-2 convolution: dense fp32 (out "columns >= nx / 2 written as zeros"),
    fp16, and the sparse form (rulebook -> tile order -> bf16x3 gather-GEMM -> rows_to_dense_fill)."""
    from paddle3d_amd.ops import conv
    from paddle3d_amd.ops import pointpillars_scatter as ps

    rng = np.random.default_rng(2)
    b, ny, nx, cin, cout, m = 2, 40, 24, 64, 64, 300
    cells = rng.choice(b * ny * nx, m, replace=False)
    c4 = np.stack([cells // (ny * nx), np.zeros(m), cells % (ny * nx) // nx, cells % nx], 1).astype(np.int32)
    _, wt, bias = _conv_inputs(5, 1, cin, cout, 3, 3)
    inputs = dict(f=_t(rng.normal(size=(m, cin)).astype(F32)), c=_t(c4), w=wt.to(DEV), b=bias.to(DEV))

    def call():
        i = inputs
        canvas = ps.SparseCanvas(i["f"], i["c"], b, ny, nx)
        assert conv.scatter_conv_supported(cin, cout, ny, nx, 2) and conv.scatter_conv_sparse_supported(cin, cout, ny, nx, 2)
        outs = dict(inv=canvas.inv, dense_canvas=canvas.dense(),
                    fp32=conv.scatter_conv3x3_bias_relu(canvas, conv.pack_conv3x3_weight(i["w"]), i["b"], cout))
        for tile in (64,):
            outs[f"f16_t{tile}"] = conv.scatter_conv3x3_s2_f16_bias_relu(canvas, conv.pack_conv3x3_f16_weight(i["w"], tile),
                                                                          i["b"], cout)
        outs["sparse"], _ = conv.scatter_conv3x3_sparse(canvas, i["w"], i["b"])
        return outs

    return inputs, call


# ---------------------------------------------------------------------------------------------------------------------
# sparse convolutions
def _random_sparse(rng, batch, shape, n, c):
    d, h, w = shape
    lin = rng.choice(batch * d * h * w, n, replace=False)
    bb, r = np.divmod(lin, d * h * w)
    z, r = np.divmod(r, h * w)
    y, x = np.divmod(r, w)
    return np.stack([bb, z, y, x], 1).astype(np.int32), rng.normal(size=(n, c)).astype(F32)


@scenario
def sparse_conv_indices_v1():
    """pd3_sparse_conv3d_indices (subm and strided; the wrapper slices out_coords / nbr by the n_out the op returns:
    "out_coords [out_cap, 4], nbr [out_cap, K] ..., n_out [1]") + the fp32 feature kernels, unordered (direct ABI:
    pd3_sparse_conv3d_features has no wrapper) and ordered, + to_dense ("fully written").  subm: n_out = n_in, and the
    rows of padding inputs are defined too ("out_coords = the input row, nbr = -1 throughout, features = the epilogue
    of an empty sum"): everything is returned whole."""
    from paddle3d_amd.ops import sparse_conv3d as sp

    rng = np.random.default_rng(6)
    coords, feats = _random_sparse(rng, 2, (9, 20, 24), 601, 16)
    coords[::40, 0] = -1  # padding rows are ignored
    g = torch.Generator().manual_seed(6)
    inputs = dict(coords=_t(coords), feats=_t(feats), w=(torch.randn(3, 3, 3, 16, 32, generator=g) * 0.1).to(DEV),
                  bias=torch.randn(32, generator=g).to(DEV), scale=torch.randn(32, generator=g).to(DEV),
                  shift=torch.randn(32, generator=g).to(DEV))

    def call():
        L, check, ptr, stream = _lib()
        i = inputs
        outs = {}
        for tag, kw in (("subm", dict(kernel_size=3, stride=1, padding=1, subm=True)),
                        ("down", dict(kernel_size=3, stride=2, padding=1, subm=False))):
            idx = sp.indices(i["coords"], 2, (9, 20, 24), **kw)
            assert idx.n_out > 0
            outs[f"{tag}_nbr"], outs[f"{tag}_coords"] = idx.nbr, idx.out_coords
            if tag == "subm":  # the padding rows: no neighbour at all, the input row as coordinates
                pad = i["coords"][:, 0] < 0
                assert int(pad.sum()) > 0 and idx.n_out == coords.shape[0]
                assert bool((idx.nbr[pad] == -1).all()) and torch.equal(idx.out_coords, i["coords"])
            res = torch.randn(idx.n_out, 32, generator=torch.Generator().manual_seed(1)).to(DEV)
            o = sp.features(i["feats"], idx, i["w"], i["bias"], i["scale"], i["shift"], res, relu=True)
            raw = torch.empty((idx.n_out, 32), dtype=torch.float32, device=DEV)
            check(L.pd3_sparse_conv3d_features(ptr(i["feats"]), ptr(idx.nbr), None, idx.n_out, 27, 16, 32, ptr(i["w"]),
                                               ptr(i["bias"]), None, None, None, 0, ptr(raw), stream),
                  "sparse_conv3d_features")
            if tag == "subm":  # an empty sum through the epilogue: bias alone for the unordered call (no scale / relu)
                assert torch.equal(raw[pad], i["bias"].expand(int(pad.sum()), 32))
            outs[f"{tag}_feats"], outs[f"{tag}_feats_unordered"] = o, raw
            if tag == "down":
                outs["dense"] = sp.to_dense(o, idx.out_coords, 2, idx.out_shape)
        return outs

    return inputs, call


@scenario
def sparse_conv_plan_with_capacity():
    """The no-sync plan (sort_coords, conv_outputs, rulebook, tile_order) with out_cap ABOVE n_out, then all four
    feature kernels (fp32 ordered, bf16x3, f16 -> f16, f16 -> f32) and to_dense at capacity.  Everything is sliced by
    the device count the plan returns (n_out_dev): rows between the count and the capacity are scratch -- except
    `order` ("-1 past the row count") and the dense map ("fully written"), which are returned whole."""
    from paddle3d_amd.ops import sparse_conv3d as sp

    rng = np.random.default_rng(7)
    shape = (9, 20, 24)
    coords, feats = _random_sparse(rng, 2, shape, 700, 32)
    coords[::33, 0] = -1
    g = torch.Generator().manual_seed(7)
    inputs = dict(coords=_t(coords), feats=_t(feats), w_subm=(torch.randn(3, 3, 3, 32, 64, generator=g) * 0.1).to(DEV),
                  w_down=(torch.randn(3, 3, 3, 64, 128, generator=g) * 0.1).to(DEV), bias=torch.randn(128, generator=g).to(DEV),
                  scale=torch.randn(128, generator=g).to(DEV), shift=torch.randn(128, generator=g).to(DEV))
    specs = [sp.ConvSpec((3, 3, 3), (1, 1, 1), (1, 1, 1), True, "a"), sp.ConvSpec((3, 3, 3), (2, 2, 2), (1, 1, 1), False)]

    def call():
        L, check, ptr, stream = _lib()
        i = inputs
        exact = sp.plan(i["coords"], 2, shape, specs)
        caps = [exact.counts[0] + 57, exact.counts[1] + 129]
        pl = sp.plan(i["coords"], 2, shape, specs, caps=caps)
        assert not bool(pl.overflow)
        n0 = _count(pl.n_in_dev)[0]
        assert n0 == exact.counts[0] < coords.shape[0]
        # "keys_sorted [n], order [n]": a permutation of ALL input rows (padding rows last), returned whole
        assert sorted(pl.order.tolist()) == list(range(coords.shape[0]))
        outs = dict(order=pl.order, overflow=pl.overflow.to(torch.int32), n0=pl.n_in_dev)
        outs["__trivial_ok__"] = {"overflow"}
        f0 = i["feats"][pl.order]  # rows of the first index set, as sparse._planned_input gathers them
        rows_in = f0
        for tag, idx, w, cin, cout in (("subm", pl.indices[0], i["w_subm"], 32, 64), ("down", pl.indices[1], i["w_down"], 64, 128)):
            k = _count(idx.n_out_dev)[0]
            assert 0 < k < idx.n_out, (tag, k, idx.n_out)  # the count is below the capacity: unspecified rows exist
            outs[f"{tag}_nbr"], outs[f"{tag}_n"] = idx.nbr[:k], idx.n_out_dev
            if idx.out_coords is not None:
                outs[f"{tag}_coords"] = idx.out_coords[:k]
            assert idx.order is not None
            outs[f"{tag}_tile_order"] = idx.order
            bias, scale, shift = i["bias"][:cout], i["scale"][:cout], i["shift"][:cout]
            f32 = sp.features(rows_in, idx, w, bias, scale, shift, None, relu=True)
            x3 = sp.features_bf16x3(rows_in, idx, sp.pack_weight_bf16x3(w), cin, cout, bias, scale, shift, None, True)
            wp = sp.pack_weight_f16(w)
            h16 = sp.features_f16(rows_in.half(), idx, wp, cin, cout, bias, scale, shift, None, True)
            h32 = sp.features_f16(rows_in.half(), idx, wp, cin, cout, bias, None, None, None, False, out_f32=True)
            raw = torch.empty((idx.n_out, cout), dtype=torch.float32, device=DEV)  # pd3_sparse_conv3d_features: no wrapper
            check(L.pd3_sparse_conv3d_features(ptr(rows_in), ptr(idx.nbr), ptr(idx.n_out_dev), idx.n_out, 27, cin, cout, ptr(w),
                                               ptr(bias), ptr(scale), ptr(shift), None, 1, ptr(raw), stream),
                  "sparse_conv3d_features")
            outs.update({f"{tag}_f32": f32[:k], f"{tag}_f32_unordered": raw[:k], f"{tag}_bf16x3": x3[:k], f"{tag}_f16": h16[:k],
                         f"{tag}_f16_f32": h32[:k]})
            rows_in = f32
        idx = pl.indices[1]
        outs["dense"] = sp.to_dense(rows_in, idx.out_coords, 2, idx.out_shape, n_dev=idx.n_out_dev)
        return outs

    return inputs, call


@scenario
def gather_gemm_f16_into_slice():
    """pd3_gather_gemm_f16 writing `cout` columns at out_off > 0 into a wider caller-owned matrix, as SecondFPN's AMP
    path does: `out` is allocated here under the guard, pre-filled, and returned whole -- the columns outside
    [out_off, out_off + cout) must come back unchanged.  Row counts that are not multiples of the 16-row block."""
    from paddle3d_amd.ops import sparse_conv3d as sp

    rng = np.random.default_rng(8)
    rows, n_in, k, cin, cout, ld, off = 1003, 517, 4, 32, 64, 192, 64
    nbr = rng.integers(-1, n_in, (rows, k)).astype(np.int32)
    g = torch.Generator().manual_seed(8)
    inputs = dict(feats=torch.randn(n_in, cin, generator=g).half().to(DEV), nbr=_t(nbr),
                  w=(torch.randn(1, 2, 2, cin, cout, generator=g) * 0.2).to(DEV), bias=torch.randn(cout, generator=g).to(DEV))

    def call():
        i = inputs
        wp = sp.pack_weight_f16(i["w"])
        outs = {}
        for tag, order in (("raster", None), ("tiled", sp.tile_order(i["nbr"]))):
            out = torch.empty((rows, ld), dtype=torch.float16, device=DEV)
            out.fill_(-3.0)
            sp.gather_gemm_f16(i["feats"], i["nbr"], wp, cin, cout, out, out_off=off, bias=i["bias"], relu=True, order=order)
            assert bool((out[:, :off] == -3.0).all()) and bool((out[:, off + cout:] == -3.0).all()), tag
            outs[tag] = out
        outs["order"] = sp.tile_order(i["nbr"])
        return outs

    return inputs, call


# ---------------------------------------------------------------------------------------------------------------------
# NMS, IoU, sort, post-processing
@scenario
def nms_and_iou():
    """n in {1, 64, 65, 129}.  keep: "first *num_to_keep entries valid" -> sliced by the returned count; IoU / overlap
    matrices whole."""
    from paddle3d_amd.ops import iou3d_nms

    inputs = {f"boxes{n}": _t(synth.nms_boxes(n, n=n, clusters=max(1, n // 6))[0]) for n in (64, 65, 129)}
    inputs["boxes1"] = inputs["boxes129"][5:6].clone()  # one box, which overlaps its own copy among the 129

    def call():
        outs = {"__trivial_ok__": {"bev_keep1", "normal_keep1"}}  # one box: keep = [0]
        for n in (1, 64, 65, 129):
            bx = inputs[f"boxes{n}"]
            for tag, fn in (("bev", iou3d_nms.nms_gpu_device), ("normal", iou3d_nms.nms_normal_gpu_device)):
                keep, num = fn(bx, 0.2)
                k = _count(num)[0]
                assert 0 < k <= n and (n < 64 or k < n)
                outs[f"{tag}_keep{n}"], outs[f"{tag}_num{n}"] = keep[:k], num
            other = inputs[f"boxes{129 if n == 1 else 65}"]
            outs[f"iou{n}"] = iou3d_nms.boxes_iou_bev_gpu(bx, other)
            outs[f"overlap{n}"] = iou3d_nms.boxes_overlap_bev_gpu(bx, other)
        outs["atan2f"] = iou3d_nms.libm_eval("atan2f", inputs["boxes129"][:, 0].contiguous(), inputs["boxes129"][:, 1].contiguous())
        outs["sinf"] = iou3d_nms.libm_eval("sinf", inputs["boxes65"][:, 6].contiguous())
        return outs

    return inputs, call


@scenario
def stable_argsort():
    from paddle3d_amd.ops import sort

    rng = np.random.default_rng(9)
    inputs = {}
    for n in (1, 63, 1000):
        inputs[f"scores{n}"] = _t(np.round(rng.random(n), 2).astype(F32))       # many equal keys
        inputs[f"ranks{n}"] = _t(rng.integers(0, 50, n).astype(np.int32))
    inputs["ranks64"] = _t(rng.integers(0, 1 << 30, 1000).astype(np.int64))

    def call():
        outs = {"__trivial_ok__": {"desc1", "asc1"}}  # one key: order = [0]
        for n in (1, 63, 1000):
            outs[f"desc{n}"] = sort.stable_argsort(inputs[f"scores{n}"], descending=True)
            outs[f"asc{n}"] = sort.stable_argsort(inputs[f"ranks{n}"], max_key=49)
        outs["asc_i64"] = sort.stable_argsort(inputs["ranks64"])
        return outs

    return inputs, call


def _cp_tasks(seed, h, w, batch=1):
    tasks = synth.center_head_outputs(seed, feat_h=h, feat_w=w, num_classes=(1, 2, 2), n_peaks=40)
    if batch > 1:
        more = [synth.center_head_outputs(seed + b, feat_h=h, feat_w=w, num_classes=(1, 2, 2), n_peaks=40)
                for b in range(1, batch)]
        tasks = [{k: np.concatenate([t[k]] + [m[j][k] for m in more]) for k in t} for j, t in enumerate(tasks)]
    return tasks


_CP = dict(voxel_size=[0.2, 0.2], point_cloud_range=[-51.2, -51.2], post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
           down_ratio=4, score_threshold=0.1, nms_iou_threshold=0.2)


@scenario
def centerpoint_postprocess_entry_points():
    """The three entry points, pre in {1, 65, 1025}.  out_count: "number of valid leading rows per frame ...; the rows
    behind it read zero" (all three forms: "none needs clearing by the caller"), so every output is returned whole.
    Maps 100 x 104 (not a multiple of anything) and, for the fused-head forms, two frames."""
    from paddle3d_amd.ops import centerpoint_postprocess as cp

    keys = ("hm", "reg", "height", "dim", "vel", "rot")
    plain = _cp_tasks(31, 100, 104)
    fused = _cp_tasks(41, 100, 104, batch=2)
    inputs = {f"p{j}_{k}": _t(t[k]) for j, t in enumerate(plain) for k in keys}
    # a fused CenterHead: every head a channel slice of ONE [B, C, H, W] map
    inputs["fused"] = _t(np.concatenate([t[k] for t in fused for k in keys], 1))
    offs = [0, 1, 3] * 3

    def call():
        outs = {}
        lists = {k: [inputs[f"p{j}_{k}"] for j in range(3)] for k in keys}
        views, c0 = {k: [] for k in keys}, 0
        for t in fused:
            for k in keys:
                views[k].append(inputs["fused"][:, c0:c0 + t[k].shape[1]])
                c0 += t[k].shape[1]
        for pre in (1, 65, 1025):
            args = (_CP["voxel_size"], _CP["point_cloud_range"], _CP["post_center_range"], offs, 4, 0.1, 0.2, pre, 83, True)
            b, s, l, n = cp.centerpoint_postprocess_device(*[lists[k] for k in keys], *args)
            k0 = _count(n)[0]
            # pre 1 and 65 leave the count below the 3 * 83 rows, so rows behind it exist; 1025 may fill them all
            assert 0 < k0 <= 3 * 83 and (pre == 1 or k0 > 3) and (k0 < b.shape[1] or pre == 1025)
            outs.update({f"plain{pre}_boxes": b, f"plain{pre}_scores": s, f"plain{pre}_labels": l, f"plain{pre}_n": n})
            for tag, kw in (("strided", {}), ("fullsort", dict(full_sort=True))):
                b, s, l, n = cp.centerpoint_postprocess_device(*[views[k] for k in keys], *args, allow_batch=True, **kw)
                assert all(0 < kf <= b.shape[1] and (kf < b.shape[1] or pre == 1025) for kf in _count(n))
                outs.update({f"{tag}{pre}_boxes": b, f"{tag}{pre}_scores": s, f"{tag}{pre}_labels": l, f"{tag}{pre}_n": n})
            b, s, l, n, r = cp.centerpoint_postprocess_device(*[views[k] for k in keys], *args, allow_batch=True, records=100)
            assert all(0 < kf <= b.shape[1] and (kf < b.shape[1] or pre == 1025) for kf in _count(n))
            outs.update({f"rec{pre}_boxes": b, f"rec{pre}_scores": s, f"rec{pre}_labels": l, f"rec{pre}_n": n,
                         f"rec{pre}_records": r})
        return outs

    return inputs, call


@scenario
def bevdet_postprocess_and_circle_nms():
    """out_count: "valid leading rows per frame ...; rows behind it read zero" -> all four outputs whole.  circle_nms:
    "keep [n] receives the kept indices in order, num_to_keep their number" -> sliced by the count; n in {1, 64, 65, 129}."""
    import bevdet_head_numpy as bh

    from paddle3d_amd import bevdet_head
    from paddle3d_amd.ops import bevdet_postprocess as bp

    heads = bh.golden_inputs()
    inputs = {f"t{j}_{k}": _t(v) for j, hd in enumerate(heads) for k, v in hd.items()}
    rng = np.random.default_rng(12)
    for n in (1, 64, 65, 129):
        inputs[f"dets{n}"] = _t(np.concatenate([rng.uniform(-10, 10, (n, 2)), rng.random((n, 1))], 1).astype(F32))

    def call():
        preds = [{k: inputs[f"t{j}_{k}"] for k in hd} for j, hd in enumerate(heads)]
        coder = bevdet_head.CenterPointBBoxCoder(**bh.GOLDEN_CODER)
        b, s, l, n = bevdet_head.get_bboxes_device(preds, bh.GOLDEN_TEST_CFG, coder, bh.GOLDEN_TASKS)
        assert all(0 < k < b.shape[1] for k in _count(n)), _count(n)
        outs = dict(boxes=b, scores=s, labels=l, n=n)
        outs["__trivial_ok__"] = {"keep1"}
        for m in (1, 64, 65, 129):
            keep, num = bp.circle_nms_device(inputs[f"dets{m}"], 4.0)
            k = _count(num)[0]
            assert 0 < k <= m and (m == 1 or k < m)
            outs[f"keep{m}"], outs[f"num{m}"] = keep[:k], num
        return outs

    return inputs, call


@scenario
def ssd_postprocess():
    """Golden case "b" of tests/golden/make_ssd_golden.py with nms_pre_max_size in {1, 65, 1025}, both selections.
    The operator writes a frame's first out_count rows (and the marker row 0 of an empty frame) and nothing else: the
    wrapper hands it zeroed outputs, which therefore come back whole with zeros behind the count."""
    import make_ssd_golden as G

    from paddle3d_amd.pointpillars import AnchorGenerator, SSDHead

    c = G.CASES["b"]
    sg = np.load(os.path.join(HERE, "golden", "python_ssd.npz"))
    gen0 = AnchorGenerator(2, c["pcr"], c["vs"], c["anchor_configs"], 1)
    cls, box, dirp = G.head_outputs("b", c, gen0.anchors.shape[0])
    fh, fw = gen0.feature_map_size
    apl = gen0.num_anchors_per_loc

    def group(p):
        bb, _, width = p.shape
        return p.reshape(bb, fh, fw, apl * width).transpose(0, 3, 1, 2)

    co = np.concatenate([sg["b_coords"], np.full((7, 4), -1, np.int32)]).astype(np.int32)
    inputs = dict(map=_t(np.concatenate([group(cls), group(box), group(dirp)], 1)), coors=_t(co))

    def call():
        outs = {}
        gen = AnchorGenerator(2, c["pcr"], c["vs"], c["anchor_configs"], 1).to(DEV)
        total = 0
        for pre in (1, 65, 1025):
            head = SSDHead(num_classes=c["num_classes"], feature_channels=c["channels"],
                           num_anchor_per_loc=2 * len(c["anchor_configs"]), **dict(c["head"], nms_pre_max_size=pre)).to(DEV).eval()
            for full in (False, True):
                b, s, l, n = head.post_process(inputs["map"], gen, inputs["coors"], device_only=True, full_sort=full)
                counts = _count(n)
                total += sum(counts)
                # the middle frame of the case is empty (marker row); pre 1 leaves every count below the 40 rows
                assert counts[1] == 0 and all(k <= b.shape[1] for k in counts) and (pre != 1 or 0 < counts[0] < b.shape[1])
                for f, k in enumerate(counts):  # zeros behind the count (behind the marker row of an empty frame)
                    assert not bool(b[f, max(k, 1):].any()) and not bool(s[f, max(k, 1):].any())
                outs.update({f"pre{pre}_{int(full)}_boxes": b, f"pre{pre}_{int(full)}_scores": s,
                             f"pre{pre}_{int(full)}_labels": l, f"pre{pre}_{int(full)}_n": n})
        assert total > 12
        # one frame of the case may be empty and a label may be class 0: the counts as a whole are checked above
        outs["__trivial_ok__"] = {k for k in outs if "labels" in k or k.endswith("_n")}
        return outs

    return inputs, call


# ---------------------------------------------------------------------------------------------------------------------
# BEV pooling, view transformers, temporal alignment
def _hand_intervals(lengths, n_depth, n_feat, n_cells, seed):
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, np.int32)
    total = int(lengths.sum())
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int32)
    cells = np.sort(rng.choice(n_cells, len(lengths), replace=False)).astype(np.int32)
    # a frustum point lands in one cell: ranks_depth never repeats (the backward STORES depth_grad[ranks_depth[i]])
    return dict(ranks_bev=np.repeat(cells, lengths).astype(np.int32), ranks_depth=rng.choice(n_depth, total, replace=False).astype(np.int32),
                ranks_feat=rng.integers(0, n_feat, total).astype(np.int32), interval_starts=starts, interval_lengths=lengths)


@scenario
def bev_pool_v2_hand_built_intervals():
    """Interval lengths that include 1, 15, 16, 17 and 31 (the 15-point clamped tail of csrc/bev_pool.hip), channel
    counts 80 and 3; out and both gradients "fully written (zero where no interval lands)"."""
    from paddle3d_amd.ops import bev_pool_v2 as bp

    lengths = [1, 15, 16, 17, 31, 2, 32, 33, 1, 1, 14, 64, 47, 3]
    assert {1, 15, 16, 17, 31} <= set(lengths)
    rng = np.random.default_rng(13)
    inputs = {}
    for c in (80, 3):
        idx = _hand_intervals(lengths, 2 * 7 * 4 * 5, 2 * 4 * 5, 11 * 13, c)
        inputs.update({f"{k}{c}": _t(v) for k, v in idx.items()})
        inputs[f"depth{c}"] = _t(rng.random((2, 7, 4, 5)).astype(F32))
        inputs[f"feat{c}"] = _t(rng.normal(size=(2, 4, 5, c)).astype(F32))
        inputs[f"grad{c}"] = _t(rng.normal(size=(1, 11, 13, c)).astype(F32))

    def call():
        outs = {}
        for c in (80, 3):
            i = {k[: -len(str(c))]: v for k, v in inputs.items() if k.endswith(str(c))}
            outs[f"out{c}"] = bp.bev_pool_v2(i["depth"], i["feat"], i["ranks_depth"], i["ranks_feat"], i["ranks_bev"],
                                             i["interval_lengths"], i["interval_starts"], (1, 11, 13, c))
            # the backward takes the index sets sorted by ranks_feat (BevPoolV2.backward does the re-sort)
            d = i["depth"].clone().requires_grad_(True)
            f = i["feat"].clone().requires_grad_(True)
            y = bp.BevPoolV2.apply(d, f, i["ranks_depth"], i["ranks_feat"], i["ranks_bev"], (1, 11, 13, c),
                                   i["interval_starts"], i["interval_lengths"])
            y.backward(i["grad"])
            outs[f"depth_grad{c}"], outs[f"feat_grad{c}"] = d.grad, f.grad
        return outs

    return inputs, call


@scenario
def view_transformers():
    """frustum_to_lidar (BEVDet rig, two frames) and voxel_pooling_prepare in its three modes ("first counts[0] /
    counts[1] valid": the wrapper slices by the counts the op returns), pooled through bev_pool_v2."""
    from paddle3d_amd import bevdet, bevfusion
    from paddle3d_amd.ops import bev_pool_v2 as bp

    rig = synth.camera_rig(2, n_cam=3, input_size=(64, 176), batch=2)
    depth, feat = synth.lss_camera_features(3, 6, 118, 4, 11, 24)
    inputs = {k: _t(v) for k, v in rig.items()}
    inputs.update(depth=_t(depth), feat=_t(feat))

    def call():
        i = inputs
        vt = bevdet.LSSViewTransformer(input_size=(64, 176), downsample=16)
        coor = vt.get_lidar_coor(i["rots"], i["trans"], i["cam2imgs"], i["post_rots"], i["post_trans"], i["bda"])
        assert vt.D == 118
        prep = vt.voxel_pooling_prepare_v2(coor)
        assert prep[0] is not None and 0 < prep[0].numel() < coor.numel() // 3  # kept points below the capacity
        outs = dict(coor=coor, **{f"m0_{k}": v for k, v in zip(("bev", "depth", "feat", "starts", "lengths"), prep)})
        outs["bev"] = vt.voxel_pooling_v2(coor, i["depth"], i["feat"].permute(0, 3, 1, 2).contiguous())
        dx, bx, nx = bevfusion.gen_dx_bx([-51.2, 51.2, 0.8], [-51.2, 51.2, 0.8], [-10.0, 10.0, 20.0])
        nx = [int(v) for v in nx]
        for split in (True, False):
            p = bp.lss_pooling_prepare(coor, dx, bx, nx, split=split)
            assert 0 < p[0].numel() < coor.numel() // 3
            outs.update({f"lss{int(split)}_{k}": v for k, v in zip(("cell", "depth", "feat", "starts", "lengths"), p)})
        outs["lss_fused"] = bp.lss_voxel_pooling_fused(coor, i["depth"], i["feat"], dx, bx, nx).contiguous()
        return outs

    return inputs, call


@scenario
def bevdet4d_align_mixed_layouts():
    """Current frame contiguous, adjacent frames alternately contiguous NCHW and the channels-last view
    voxel_pooling_v2 returns; with and without the current frame; the sampling grid returned."""
    import bevdet4d_align_numpy as ba

    from paddle3d_amd import bevdet4d

    rng = np.random.default_rng(14)
    B, Ch, H, W, nadj = 2, 5, 9, 13, 3
    rots, trans = ba.poses(rng, B, nadj)
    inputs = {f"rots{k}": _t(r) for k, r in enumerate(rots)}
    inputs.update({f"trans{k}": _t(t) for k, t in enumerate(trans)})
    inputs["bda"] = _t(np.broadcast_to(ba.bda_matrix(rot_deg=7.0, flip_x=True), (B, 3, 3)).copy())
    for k in range(nadj + 1):
        f = ba.features(rng, (B, Ch, H, W))
        inputs[f"feat{k}"] = _t(np.ascontiguousarray(np.transpose(f, (0, 2, 3, 1)))) if k % 2 else _t(f)

    def call():
        i = inputs
        feats = [i[f"feat{k}"].permute(0, 3, 1, 2) if k % 2 else i[f"feat{k}"] for k in range(nadj + 1)]
        r, t = [i[f"rots{k}"] for k in range(nadj + 1)], [i[f"trans{k}"] for k in range(nadj + 1)]
        out, grid = bevdet4d.align_concat(feats, r, t, i["bda"], return_grid=True)
        shifted = bevdet4d.shift_feature(feats[1], [t[0], t[1]], [r[0], r[1]], i["bda"])
        return dict(out=out, grid=grid, shifted=shifted)

    return inputs, call


@scenario
def ms_deform_attn():
    """C in {3, 16, 32}, the unaligned-value case (a contiguous view 4 bytes into its buffer), fp32 and fp64; forward
    exact; backward: grad_sampling_loc and grad_attn_weight exact ("bitwise reproducible"), grad_value (float atomics)
    under its own test's tolerance -- see TOLERANT."""
    import ms_deform_attn_numpy as md

    from paddle3d_amd.ops import ms_deform_attn as op

    inputs, cases = {}, []
    for C_, dtype in ((3, np.float32), (16, np.float32), (32, np.float32), (32, np.float64)):
        tag = f"c{C_}_{np.dtype(dtype).name}"
        value, loc, attn, sh, st = md.random_case(np.random.default_rng(C_), 2, 37, 2, C_, [[5, 11], [3, 6]], 3, dtype, -0.3, 1.3)
        inputs.update({f"{tag}_value": _t(value), f"{tag}_loc": _t(loc), f"{tag}_attn": _t(attn), f"{tag}_sh": _t(sh),
                       f"{tag}_st": _t(st)})
        inputs[f"{tag}_go"] = _t(np.random.default_rng(C_ + 1).standard_normal((2, 37, 2 * C_)).astype(dtype))
        cases.append(tag)
    v32 = inputs["c32_float32_value"]
    buf = torch.zeros(v32.numel() + 1, dtype=torch.float32, device=DEV)
    buf[1:].copy_(v32.reshape(-1))
    inputs["unaligned_buffer"] = buf

    def call():
        outs = {}
        for tag in cases:
            a = [inputs[f"{tag}_{k}"] for k in ("value", "loc", "attn", "sh", "st")]
            outs[f"{tag}_out"] = op.ms_deform_attn(*a, 64)
            gv, gl, ga = op.ms_deform_attn_backward(inputs[f"{tag}_go"], *a, 64)
            outs[f"{tag}_grad_value"], outs[f"{tag}_grad_loc"], outs[f"{tag}_grad_attn"] = gv, gl, ga
        a = [inputs[f"c32_float32_{k}"] for k in ("value", "loc", "attn", "sh", "st")]
        a[0] = inputs["unaligned_buffer"][1:].view(a[0].shape)
        assert a[0].data_ptr() % 16 == 4
        outs["unaligned_out"] = op.ms_deform_attn(*a, 64)
        return outs

    return inputs, call


# ---------------------------------------------------------------------------------------------------------------------
# point ops
def _cloud(rng, *shape):
    lo, hi = np.array([0, -40, -3], F32), np.array([70.4, 40, 1], F32)
    return (lo + rng.random(shape + (3,), dtype=F32) * (hi - lo)).astype(F32)


def _int_grad(rng, *shape):
    """Small integers: their fp32 sums are exact in any order, so a float-atomic gradient is one bit pattern."""
    return rng.integers(-8, 9, shape).astype(F32)


@scenario
def pointnet2_batch_ops():
    """FPS n in {1, 1023, 1025} on both tiers, gather / ball query / grouping with their gradients (integer-valued
    grad_out: exact under float atomics), points_in_boxes on the [:, :, 0:7] view of an [B, M, 8] tensor."""
    from paddle3d_amd.ops import pointnet2_ops as pn
    from paddle3d_amd.ops import roiaware_pool3d as roi

    rng = np.random.default_rng(15)
    inputs = {f"xyz{n}": _t(_cloud(rng, 2, n)) for n in (1, 1023, 1025)}
    n, m, s, c = 1025, 129, 9, 5
    inputs.update(feats=_t(rng.normal(size=(2, c, n)).astype(F32)), g_gather=_t(_int_grad(rng, 2, c, m)),
                  g_group=_t(_int_grad(rng, 2, c, m, s)))
    boxes = np.concatenate([_cloud(rng, 2, 33), rng.uniform(2, 12, (2, 33, 3)).astype(F32),
                            rng.uniform(-3, 3, (2, 33, 2)).astype(F32)], -1)
    inputs["boxes8"] = _t(boxes)

    def call():
        i = inputs
        outs = {"__trivial_ok__": {"fps1_t0", "fps1_t1", "fps1_t2"}}  # one point: every sample is index 0
        for k in (1, 1023, 1025):
            for tier in (0, 1, 2):
                outs[f"fps{k}_t{tier}"] = pn.farthest_point_sample(i[f"xyz{k}"], min(k, 65) if k > 1 else 3, tier)
        idx = pn.farthest_point_sample(i["xyz1025"], m)
        f = i["feats"].clone().requires_grad_(True)
        got = pn.gather_operation(f, idx)
        got.backward(i["g_gather"])
        outs["gather"], outs["gather_grad"] = got, f.grad
        new_xyz = pn.gather_operation(i["xyz1025"].transpose(1, 2).contiguous(), idx).transpose(1, 2).contiguous()
        ball = pn.ball_query_batch(new_xyz, i["xyz1025"], 6.0, s)
        f2 = i["feats"].clone().requires_grad_(True)
        grouped = pn.grouping_operation_batch(f2, ball)
        grouped.backward(i["g_group"])
        outs.update(ball=ball, grouped=grouped, grouped_grad=f2.grad)
        outs["in_boxes"] = roi.points_in_boxes_gpu(i["xyz1025"], i["boxes8"][:, :, 0:7])
        assert bool((outs["in_boxes"] >= 0).any()) and bool((outs["in_boxes"] < 0).any())
        return outs

    return inputs, call


@scenario
def pointnet2_stack_ops():
    from paddle3d_amd import pointnet2_stack as ps2
    from paddle3d_amd.ops import pointnet2_ops as pn

    rng = np.random.default_rng(16)
    cnt, qcnt = np.array([1025, 0, 700], np.int32), np.array([129, 0, 65], np.int32)  # a frame without points
    xyz = _cloud(rng, int(cnt.sum()))
    q = np.concatenate([xyz[rng.choice(1025, 129)], xyz[1025 + rng.choice(700, 65)]]) + F32(0.1)  # near their frame's points
    Z, Y, X = 5, 40, 36
    vs, lo = np.array([2.0, 2.0, 1.0], F32), np.array([0.0, -40.0, -3.0], F32)
    cells = np.unique(np.concatenate([np.repeat(np.arange(2), 900)[:, None],
                                      np.stack([rng.integers(0, Z, 1800), rng.integers(0, Y, 1800), rng.integers(0, X, 1800)], 1)],
                                     1), axis=0).astype(np.int32)
    vxyz = ((cells[:, [3, 2, 1]].astype(F32) + F32(0.5)) * vs + lo).astype(F32)
    vq = vxyz[rng.choice(len(vxyz), 203)] + rng.normal(0, 0.5, (203, 3)).astype(F32)
    vq_b = np.sort(rng.integers(0, 2, 203))[:, None]
    vcoords = np.concatenate([vq_b, np.floor((vq - lo) / vs).astype(np.int64)[:, [2, 1, 0]]], 1).astype(np.int32)
    inputs = dict(xyz=_t(xyz), cnt=_t(cnt), q=_t(q.astype(F32)), qcnt=_t(qcnt), feats=_t(rng.normal(size=(len(xyz), 7)).astype(F32)),
                  grad=_t(_int_grad(rng, len(q), 7, 6)), cells=_t(cells), vxyz=_t(vxyz), vq=_t(vq.astype(F32)), vcoords=_t(vcoords))

    def call():
        i = inputs
        idx = pn.ball_query_stack(i["q"], i["qcnt"], i["xyz"], i["cnt"], 4.0, 6)
        assert bool((idx[:, 0] >= 0).any())
        safe = idx.clamp(min=0)
        f = i["feats"].clone().requires_grad_(True)
        grouped = pn.grouping_operation_stack(f, i["cnt"], safe, i["qcnt"])
        grouped.backward(i["grad"])
        pinds = ps2.generate_voxel2pinds([2, Z, Y, X, 32], i["cells"])
        vidx = pn.voxel_query_wrapper(i["vq"], i["vxyz"], i["vcoords"], pinds, 3.0, 5, 1, 2, 2)
        assert bool((vidx[:, 0] >= 0).any())
        return dict(ball=idx, grouped=grouped, grouped_grad=f.grad, pinds=pinds, voxel_query=vidx)

    return inputs, call


@scenario
def assign_score_withk():
    """(B, N, K, M, O) = (2, 33, 5, 3, 17); forward and the three gradients, all "bitwise reproducible" (no atomics)."""
    from paddle3d_amd.ops import assign_score_withk as op

    rng = np.random.default_rng(17)
    B, N, K, M, O = 2, 33, 5, 3, 17
    x = rng.standard_normal((B, N, 3)).astype(F32)
    idx = np.argsort(((x[:, :, None] - x[:, None]) ** 2).sum(-1), -1, kind="stable")[..., :K].astype(np.int64)
    inputs = dict(scores=_t((rng.random((B, N, K, M), dtype=F32) + F32(0.5)).astype(F32)),
                  points=_t(rng.standard_normal((B, N, M, O)).astype(F32)), centers=_t(rng.standard_normal((B, N, M, O)).astype(F32)),
                  knn=_t(idx), grad=_t(rng.standard_normal((B, O, N)).astype(F32)))

    def call():
        i = inputs
        out = op.assign_score_withk(i["scores"], i["points"], i["centers"], i["knn"])
        gs, gp, gc = op.assign_score_withk_backward(i["grad"], i["scores"], i["points"], i["centers"], i["knn"])
        only = op.assign_score_withk_backward(i["grad"], i["scores"], i["points"], i["centers"], i["knn"],
                                              need=(False, True, False))
        return dict(out=out, grad_scores=gs, grad_points=gp, grad_centers=gc, grad_points_only=only[1])

    return inputs, call


# ---------------------------------------------------------------------------------------------------------------------
# whole models at the smallest configuration each accepts; constructed INSIDE the run
def _randomise_bn(model):
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)


def _centerpoint(factory, points, amp=False, **kw):
    inputs = dict(points=_t(points))

    def call():
        torch.manual_seed(0)
        model = factory(**kw)
        _randomise_bn(model)
        with torch.no_grad():
            for task in model.bbox_head.tasks:
                task.hm[-1].bias.fill_(-1.0)
        model = model.to(DEV).eval()
        if amp:
            model.set_amp(True)
        outs = {}
        for rep in range(2):  # the second forward runs on the cached plans, packed weights and workspaces
            dets = model.test_forward(inputs["points"])
            assert len(dets) == inputs["points"].shape[0]
            for f, d in enumerate(dets):
                assert d["scores"].shape[0] > 0
                outs.update({f"boxes{rep}_{f}": d["box3d_lidar"], f"scores{rep}_{f}": d["scores"],
                             f"labels{rep}_{f}": d["label_preds"]})
        outs["__trivial_ok__"] = {k for k in outs if k.startswith("labels")}  # class 0 alone is a legal result
        return outs

    return inputs, call


def _nusc_frames(seed, n):
    return np.stack([synth.nuscenes_sweep(seed + i, n_points=n) for i in range(2)])


@scenario
def model_centerpoint_pillars_fp32():
    from paddle3d_amd import centerpoint as cpm

    return _centerpoint(cpm.centerpoint_pillars_nuscenes, _nusc_frames(70, 40000), max_num_voxels=(24000, 24000))


@scenario
def model_centerpoint_pillars_amp():
    from paddle3d_amd import centerpoint as cpm

    return _centerpoint(cpm.centerpoint_pillars_nuscenes, _nusc_frames(72, 40000), amp=True, max_num_voxels=(24000, 24000))


@scenario
def model_centerpoint_voxels():
    from paddle3d_amd import centerpoint as cpm

    # the config's own range: 41 x 1440 x 1440 sparse grid, a 180-wide first stage and a 90-wide second one (rows at pitch 92)
    return _centerpoint(cpm.centerpoint_voxels_nuscenes, _nusc_frames(74, 40000), max_num_voxels=(30000, 30000))


@scenario
def model_pointpillars_kitti():
    from paddle3d_amd import pointpillars as ppm

    pts = np.stack([synth.kitti_frame(80 + i, n_points=12000) for i in range(2)])
    inputs = dict(points=_t(pts))

    def call():
        torch.manual_seed(0)
        model = ppm.pointpillars_kitti_car(max_num_voxels=(8000, 8000))
        _randomise_bn(model)
        model = model.to(DEV).eval()
        outs = {}
        for rep in range(2):
            b, s, l, n = model.test_forward(inputs["points"], device_only=True)
            for f, k in enumerate(_count(n)):
                k = max(k, 1)  # count 0: the marker row
                outs.update({f"boxes{rep}_{f}": b[f, :k], f"scores{rep}_{f}": s[f, :k], f"labels{rep}_{f}": l[f, :k]})
            outs[f"n{rep}"] = n
        outs["__trivial_ok__"] = {k for k in outs if k.startswith("labels")}  # one class: every label is 0
        return outs

    return inputs, call


@scenario
def selfcheck_lds_atomic_order():
    """The hardware self-check the voxelizer's path choice consults, made to run again (it is cached per process)."""
    from paddle3d_amd.ops import voxelize

    inputs = {}

    def call():
        voxelize.reset_lds_atomic_order_probe()
        ok = voxelize.lds_atomic_order_ok(DEV)
        return dict(ok=torch.tensor([int(ok)]))

    return inputs, call


@scenario
def selfcheck_block_topk():
    """The block top-K selection's probe: two sets, keys from global memory (form 0) and staged into LDS (form 1), with
    a left-out value and keys above 2^key_bits.  idx / key [sets][K] and cut [sets][2], all whole."""
    rng = np.random.default_rng(23)
    n, K, key_bits, leave_out = 4097, 129, 21, (1 << 21) - 1
    keys = rng.integers(0, 1 << 21, (2, n)).astype(np.uint32)
    keys[0, ::5] = leave_out
    keys[1, ::7] = 0xFFFFFFFF
    keys[1, 100:400] = 0                    # 300 keys tie for the first K = 129 places: the cut lies among them
    inputs = dict(keys=_t(keys.view(np.int32)))

    def call():
        lib, check, ptr, stream = _lib()
        outs = {}
        for form in (0, 1):
            idx = torch.empty((2, K), dtype=torch.int32, device=DEV)
            key = torch.empty((2, K), dtype=torch.int32, device=DEV)
            cut = torch.empty((2, 2), dtype=torch.int32, device=DEV)
            check(lib.pd3_selfcheck_block_topk(ptr(inputs["keys"]), 2, n, K, key_bits, form, leave_out, 0, ptr(idx),
                                               ptr(key), ptr(cut), stream), "selfcheck_block_topk")
            outs.update({f"idx{form}": idx, f"key{form}": key, f"cut{form}": cut})
        assert torch.equal(outs["idx0"], outs["idx1"])
        for form in (0, 1):                 # neither set refused (a refused set's words are all 0xFFFFFFFF)
            assert (outs[f"cut{form}"] != -1).any(dim=1).all() and (outs[f"idx{form}"] != -1).all()
        assert outs["cut0"][1].tolist() == [0, K]
        return outs

    return inputs, call


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.scenarios))
def test_scenario(name):
    P.check_scenario(name)


# host-only queries: they launch nothing
def _host_only(sym):
    return sym in ("pd3_version", "pd3_target_arch") or sym.endswith(("_workspace", "_entries", "_floats"))


# launching entry points no scenario has to reach, by name (at most two may ever be listed).  Empty: the hardware
# self-check and the profiling entry pd3_conv3x3_winograd43_pp_trace both have a scenario.
NOT_REQUIRED = set()


def test_every_launching_entry_point_is_exercised():
    """Runs last.  Scenarios that did not run in this process (the test selected alone, or with -k) are run here in
    their plain form under the launch ledger, so the assertion never depends on test selection."""
    from paddle3d_amd import _lib

    launching = [s for s in _lib.symbols("test_memory_safety_gpu") if not _host_only(s)]
    assert len(NOT_REQUIRED) <= 2 and NOT_REQUIRED <= set(launching)
    P.check_complete([s for s in launching if s not in NOT_REQUIRED])
