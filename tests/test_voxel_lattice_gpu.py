"""hard_voxelize's forms across cell, tile, group and cap borders (tests/voxel_lattice.py has the lattice, the restated plans
and the references; tests/test_voxel_lattice_cpu.py their own checks).

Every (case, form) pair is decided by the restated plan: where it refuses, the library must answer status -3 and nothing
else; where it accepts, voxels (as uint32), coords, counts and num_voxels of every frame must equal the oracle port on
that frame's own points, bit for bit.  A disagreement between the restated rule and the library in either direction is a
failure; nothing skips.  Every case runs on `auto`, on `sort` and on the forms its family names.

test_cells      fp32 points on and beside every cell boundary (+-6 ulps, fp32 and float64 boundaries), the single-cell z
                bounds, signed zeros / denormals / 1e-40 at zero minima, size * 2^20, 1e30, FLT_MAX, NaN, +-inf, on five
                grids and every form that takes them, every point alone in its cell so that none hides behind P; the same
                points through dynamic_voxelize against ref_cells.
test_points     N at 1, 63 .. 65, T - 1 .. T + 1, 2T, 2T + 1 for every route tile T, 64 and 65 tiles, ragged batches.
test_groups     one group at the register / hash-pass borders of the group kernels, in three layouts over the route tiles.
test_slots      cell multiplicities around P for P in {1, 2, 20, 254}; P = 255 refused by every fast form.
test_voxels     the voxel cap against the occupied cells, inside a tile and at its end; tiles that open 4095 .. T cells
                (kVwAssignCap) with V inside the direct-store range; pieces of 8 and 9 first points per thread (kHold).
test_grids      1 x 1 x 1 up to 16385 x 16384: the 2^20 / 2^22 / 2^28 borders, non-power-of-two extents.
test_rowq_bound max_voxels * rowq at 2^24 - 4097 (runs once, on the wave form) and 2^24 - 4096 (refused); the bound counts
                floats, not float4s, behind a voxels tensor at data_ptr() % 16 == 4.
test_rows       D = 3 .. 8 with P * D % 4 zero and non-zero; points and voxels at data_ptr() % 16 == 4.
test_batch      B in {1, 2, 3, 8, 9}, ragged, with the batched coors output on every form (frame0 of the two-stream form).
test_index      every index case through hard_voxelize_index_batch: None exactly where neither wave form takes the case.
"""
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_lattice as L  # noqa: E402

pytestmark = pytest.mark.gpu


def _device_error(e):
    """A HIP error is not a wrong result: nothing more may run on the device in this session."""
    pytest.exit(f"device error, stopping the session: {e}", returncode=3)


def _compare(oracle, case, out, coors=False):
    vox, co, npv, nv = out[:4]
    b, _ = L.sizes(case)
    for f in range(b):
        rv, rc, rn, rnv = L.port_reference(oracle, case, f)
        assert int(nv[f]) == rnv, ("num_voxels", f, int(nv[f]), rnv)
        np.testing.assert_array_equal(co[f], rc)
        np.testing.assert_array_equal(npv[f], rn)
        np.testing.assert_array_equal(np.ascontiguousarray(vox[f]).view(np.uint32), rv.view(np.uint32))
        if coors:
            c4 = out[4].reshape(b, case.V, 4)[f]
            assert (c4[:rnv, 0] == f).all() and (c4[rnv:, 0] == -1).all(), ("batch index", f)
            np.testing.assert_array_equal(c4[:, 1:], rc)


def _sweep(oracle, cases, coors=False, forms=None, label=""):
    """Every case on auto, sort and its forms.  Returns nothing; fails with the list of (case, form) pairs that differ."""
    failures, accepted, refused = [], 0, 0
    t0 = time.perf_counter()
    for case in cases:
        inputs = L.device_input(case)
        for form in ("auto", "sort") + tuple(forms or case.forms):
            pl = L.case_plan(case, form)
            try:
                status, out = L.run(case, form, coors=coors, inputs=inputs)
            except RuntimeError as e:
                _device_error(e)
            try:
                if not pl.ok:
                    refused += 1
                    assert status == -3, f"the restated plan refuses, the library answered status {status}"
                else:
                    accepted += 1
                    assert status == 0, f"the restated plan accepts ({pl.kind}), the library answered status {status}"
                    _compare(oracle, case, out, coors)
            except AssertionError as e:
                failures.append(f"{case.id} [{form}]: {str(e).strip()[:300]}")
    print(f"\n{label}: {len(cases)} cases, {accepted} runs compared, {refused} refusals, "
          f"{time.perf_counter() - t0:.2f} s")
    assert not failures, f"{len(failures)} (case, form) pairs differ:\n" + "\n".join(failures[:40])


def test_lds_order_probe_holds():
    """`auto` is the library's own choice only where the probe passes (else ops.voxelize diverts it to the sort form)."""
    from paddle3d_amd.ops import voxelize

    assert voxelize.lds_atomic_order_ok(torch.device("cuda", torch.cuda.current_device()))


def test_cells(oracle):
    cases = L.family("cells")
    _sweep(oracle, cases, label="cells")
    for case in cases:   # the same points through dynamic_voxelize
        pts = L.frame_points(case, 0)
        cells, inside = L.ref_cells(pts, case.vs, case.pr)
        want = np.where(inside[:, None], cells[:, ::-1], -1).astype(np.int32)
        got = L.run_dynamic(case)
        bad = np.nonzero((got != want).any(1))[0]
        assert len(bad) == 0, (case.id, len(bad), pts[bad[:5], :3].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())


def test_points(oracle):
    _sweep(oracle, L.family("points"), label="points")


def test_groups(oracle):
    _sweep(oracle, L.family("groups"), label="groups")


def test_slots(oracle):
    _sweep(oracle, L.family("slots"), label="slots")


def test_voxels(oracle):
    _sweep(oracle, L.family("voxels"), label="voxels")


def test_grids(oracle):
    _sweep(oracle, L.family("grids"), label="grids")


def test_rowq_bound(oracle):
    """max_voxels * rowq < 2^24 - 4096 at P = 1, D = 4: V = 2^24 - 4096 is refused by the fast forms and leaves the
    full-size outputs untouched; V = 2^24 - 4097 runs once on the wave form (0.5 GB of outputs, compared on the device: the
    first rows with the oracle port at a small cap, every row behind them zero)."""
    keys = lambda rng: L._random_keys(rng, L.PILLAR, 3000)  # noqa: E731
    (v_ok, _), (v_no, _) = L.ROWQ_CASES
    refused = L._unit_case("rowq-refused", "grids", L.PILLAR, keys, 1, v_no, forms=("wave", "tiled", "gather", "s0"))
    for form in refused.forms:
        assert not L.case_plan(refused, form).ok
        status, outs = L.run_raw(refused, form)
        assert status == -3, (form, status)
        assert all(bool((o == -7).all()) for o in outs), form
        del outs
    case = L._unit_case("rowq-accepted", "grids", L.PILLAR, keys, 1, v_ok)
    assert L.case_plan(case, "wave").ok
    status, (vox, co, npv, nv) = L.run_raw(case, "wave")
    assert status == 0
    _head_equals_port(oracle, case, vox, co, npv, nv)


def _head_equals_port(oracle, case, vox, co, npv, nv, head=4096):
    """Device outputs of a one-frame case with a huge V: the first `head` rows equal the oracle port at V = head (the case's
    points open fewer cells than that), every row behind them is zero."""
    small = L.Case(case.id + "-head", case.family, case.vs, case.pr, case.P, head, case.D, case.forms,
                   lambda rng: (L.data(case)[0][0], None))
    rv, rc, rn, rnv = L.port_reference(oracle, small)
    assert int(nv[0]) == rnv < head
    assert np.array_equal(vox[0, :head].cpu().numpy().view(np.uint32), rv.view(np.uint32))
    assert np.array_equal(co[0, :head].cpu().numpy(), rc) and np.array_equal(npv[0, :head].cpu().numpy(), rn)
    assert not bool(vox[0, head:].view(torch.int32).any()) and not bool(co[0, head:].any()) and not bool(npv[0, head:].any())


def test_rowq_bound_counts_the_writer_that_runs(oracle):
    """P = 1, D = 8, V = 2^21: two float4s per row, 2^22 units, taken; with voxels at data_ptr() % 16 == 4 the scalar writer
    would run with 2^24 units, so every fast form refuses and leaves the outputs untouched, and `auto` runs the sort form."""
    keys = lambda rng: L._random_keys(rng, L.PILLAR, 3000)  # noqa: E731
    case = L._unit_case("rowq-misaligned", "rows", L.PILLAR, keys, 1, 1 << 21, D=8, forms=("tiled", "gather", "wave", "s0"))
    for form in case.forms:
        assert L.case_plan(case, form).ok and not L.case_plan(case, form, aligned=False).ok
        status, outs = L.run_raw(case, form, misalign_voxels=True)
        assert status == -3, (form, status)
        assert all(bool((o == -7).all()) for o in outs), form
        del outs
    assert L.case_plan(case, "auto", aligned=False).kind == "sort"
    for form, mis in (("auto", True), ("wave", False)):
        status, (vox, co, npv, nv) = L.run_raw(case, form, misalign_voxels=mis)
        assert status == 0, (form, status)
        _head_equals_port(oracle, case, vox, co, npv, nv)
        del vox, co, npv, nv


def test_rows(oracle):
    cases = L.family("rows")
    _sweep(oracle, cases, label="rows")
    failures = []
    for case in cases:
        for form in ("auto", "sort") + case.forms:
            pl = L.case_plan(case, form)
            assert pl == L.case_plan(case, form, aligned=False)                    # (far below the row-unit bound)
            try:
                status, out = L.run(case, form, misalign=True)                     # points at % 16 == 4
                rstatus, rout = L.run_raw(case, form, misalign_voxels=True)        # voxels at % 16 == 4: the scalar writer
            except RuntimeError as e:
                _device_error(e)
            try:
                assert status == rstatus == (0 if pl.ok else -3), (status, rstatus, pl.ok)
                if pl.ok:
                    _compare(oracle, case, out)
                    _compare(oracle, case, [o.cpu().numpy() for o in rout])
            except AssertionError as e:
                failures.append(f"{case.id} [{form}] misaligned: {str(e).strip()[:300]}")
    assert not failures, "\n".join(failures[:40])


def test_batch(oracle):
    cases = L.family("batch")
    odd = [c for c in cases if c.c("B") % 2 == 1 and c.c("B") > 1]
    assert odd and all(L.case_plan(c, "split").ok for c in odd if c.grid == L.PILLAR)   # 12 / 13 split an odd batch
    _sweep(oracle, cases, coors=True, label="batch")


def test_index(oracle):
    cases = L.index_cases()
    failures, served, none = [], 0, 0
    t0 = time.perf_counter()
    for case in cases:
        pl = L.case_index_plan(case)
        try:
            out = L.run_index(case)
        except RuntimeError as e:
            _device_error(e)
        try:
            assert (out is None) == (pl is None), f"restated rule: {pl}, the library answered {'None' if out is None else 'rows'}"
            if out is None:
                none += 1
                continue
            served += 1
            _compare(oracle, case, out[:4])
            b, _ = L.sizes(case)
            for f in range(b):
                rnv = L.port_reference(oracle, case, f)[3]
                assert (out[4][f, :rnv, 0] == f).all() and (out[4][f, rnv:, 0] == -1).all()
                np.testing.assert_array_equal(out[4][f, :, 1:], out[1][f])
        except AssertionError as e:
            failures.append(f"{case.id} [index]: {str(e).strip()[:300]}")
    print(f"\nindex: {len(cases)} cases, {served} compared, {none} answered None, {time.perf_counter() - t0:.2f} s")
    assert served and none
    assert not failures, f"{len(failures)} cases differ:\n" + "\n".join(failures[:40])
