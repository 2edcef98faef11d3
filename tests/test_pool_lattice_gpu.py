"""The sort, index-build and BEV pooling chain across its borders (tests/pool_lattice.py has the lattice, the restated plans
and the references; tests/test_pool_lattice_cpu.py their own checks).  Every comparison is exact; nothing skips.

test_argsort         stable_argsort on n at 1, 2 and the block / radix tile / scan tile borders, max_key on both sides of every
                     plan switch (1x10, 2x6, 2x10, 3x7, 3x10, 4x8) with key families that move when a pass takes a wrong shift
                     or mask; fp32 keys with NaNs of both signs, +-0, +-inf, denormals and bit neighbours planted.
test_argsort_big     n = 2048 * 4096 + 1 at max_key 1023: the first size at which scan_partials_kernel runs with per = 2.
test_prepare         voxel_pooling_prepare in its three modes: the same sizes, grids of 1023 .. 2^31 cells, fp32 neighbours of
                     the cell boundaries of the real grids with NaN / inf / huge values, and the occupancy extremes; all five
                     index arrays and both counts equal ref_prepare.
test_prepare_refuses grids whose largest cell id does not fit the int32 ranks_bev: PD3_EUNSUPPORTED, nothing written.
test_pool            bev_pool_v2 / bev_pool_v2_bkwd on hand-built interval tables around the 16-point load batch, and on the
                     index sets of the prepare families (test_chain: prepared and pooled on the device end to end).
test_frustum         frustum_to_lidar bit for bit against its fp32 restatement.
"""
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pool_lattice as L  # noqa: E402

pytestmark = pytest.mark.gpu

PREP = {c.id: c for c in L.prepare_cases()}


@pytest.mark.parametrize("case", L.all_sort_cases(), ids=lambda c: c.id)
def test_argsort(case):
    want = L.ref_argsort(L.sort_keys(case), case.mode)
    np.testing.assert_array_equal(L.run_argsort(case), want)
    if case.mode == 0 and case.max_key == (1 << 31) - 1:
        # a max_key beyond the wrapper's range check: the C entry point sorts the same keys on all 32 bits
        keys = torch.from_numpy(L.sort_keys(case).copy()).cuda()
        np.testing.assert_array_equal(L.raw_argsort(keys, 0, 0xFFFFFFFF).cpu().numpy(), want)
    if case.mode == 0 and case.kind == "sizes":
        # and a max_key above the largest key present: more passes than the keys need, the same order
        keys = torch.from_numpy(L.sort_keys(case).copy()).cuda()
        np.testing.assert_array_equal(L.raw_argsort(keys, 0, min(4 * case.max_key + 3, 0xFFFFFFFF)).cpu().numpy(), want)


def test_argsort_big():
    """n = 2048 * 4096 + 1 keys below 1024: one pass, 1024 bins, 4097 radix tiles, 1025 scan tiles over the [digit][tile]
    table -- scan_partials_kernel's 1024 threads take two tiles each (per = 2).  No smaller n reaches that branch (the CPU
    file asserts it).  Keys (i * 389) % 1024 are made on the device and the order is compared there with its closed form."""
    case = L.big_sort_case()
    assert case.plan.per == 2
    i = torch.arange(case.n, dtype=torch.int64, device="cuda")
    keys = ((i * L.BIG_MUL) % (case.max_key + 1)).to(torch.int32)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    order = L.raw_argsort(keys, 0, case.max_key)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    want = L.big_sort_expected(i)
    assert torch.equal(order.long(), want)
    torch.cuda.synchronize()
    print(f"\nargsort n = {case.n}: sort {t1 - t0:.3f} s, closed form and compare {time.perf_counter() - t1:.3f} s")


def _check_prepare(case, got, counts):
    want = L.prep_reference(case)
    assert counts.tolist() == [len(want[0]), len(want[3])], (counts.tolist(), len(want[0]), len(want[3]))
    for name, g, w in zip(("ranks_bev", "ranks_depth", "ranks_feat", "interval_starts", "interval_lengths"), got, want):
        np.testing.assert_array_equal(g, w, err_msg=name)
    assert (got[0] >= 0).all()
    same = got[0][1:] == got[0][:-1]
    assert (np.diff(got[1])[same] > 0).all()          # ranks_depth ascends inside an interval


@pytest.mark.parametrize("case", L.prepare_cases(), ids=lambda c: c.id)
def test_prepare(case):
    status, got, counts = L.run_prepare(case)
    assert status == 0, status
    _check_prepare(case, got, counts)


@pytest.mark.parametrize("case", L.refused_cases(), ids=lambda c: c.id)
def test_prepare_refuses(case):
    """PD3_EUNSUPPORTED for a grid of more than 2^31 cells (2049 x 1024 x 1024 was served with negative ranks_bev while the
    bound stood at 2^32 - 1), for 2^32 - 1 and 2^32 cells, and for a product that wraps int64; nothing is written."""
    status, outs, counts = L.run_prepare(case)
    assert status == -3, status
    assert all((o == -7).all() for o in outs) and (counts == -7).all()


def test_prepare_wrappers_on_nothing_kept():
    from paddle3d_amd.ops import bev_pool_v2 as bp

    case = PREP["occ-none-m0"]
    coor = torch.from_numpy(L.coor_of(case).copy()).cuda().reshape(1, 1, 1, 300, 1, 3)
    assert bp.voxel_pooling_prepare_v2(coor, case.lower, case.step, case.size) == (None,) * 5
    lower, step = np.asarray(case.lower, np.float32), np.asarray(case.step, np.float32)
    for split in (True, False):   # bx = lower + dx / 2 gives the unit grid back
        out = bp.lss_pooling_prepare(coor, step, lower + step / 2, [int(s) for s in case.size], split=split)
        assert len(out) == 5 and all(o.numel() == 0 and o.dtype == torch.int32 for o in out)


def _check_pool(case, out, dg, fg):
    want, wdg, wfg = L.pool_reference(case)
    assert L.same_bits(out, want), ("out", int((out.view(np.uint32) != want.view(np.uint32)).sum()))
    assert L.same_bits(dg, wdg), ("depth_grad", int((dg.view(np.uint32) != wdg.view(np.uint32)).sum()))
    assert L.same_bits(fg, wfg), ("feat_grad", int((fg.view(np.uint32) != wfg.view(np.uint32)).sum()))


@pytest.mark.parametrize("case", L.all_pool_cases(), ids=lambda c: c.id)
def test_pool(case):
    """Forward, depth_grad and feat_grad equal the sequential fp32 reference bit for bit (the references' index sets)."""
    _check_pool(case, *L.run_pool(L.pool_data(case)))


@pytest.mark.parametrize("case", L.chain_cases(), ids=lambda c: c.id)
def test_chain(case):
    """The chain on the device end to end: prepare -> bev_pool_v2 -> re-sort by ranks_feat (stable_argsort) ->
    bev_pool_v2_bkwd, the way BevPoolV2 strings them together, against the references."""
    from paddle3d_amd.ops import bev_pool_v2 as bp
    from paddle3d_amd.ops.sort import stable_argsort

    prep, d = PREP[case.source], L.pool_data(case)
    coor = torch.from_numpy(L.coor_of(prep).copy()).cuda()
    rb, rd, rf, st, ln = bp._prepare(coor, prep.batch, prep.depth_bins, prep.feat_hw, prep.lower, prep.step, prep.size,
                                     prep.mode)
    depth, feat, grad = (torch.from_numpy(a.copy()).cuda() for a in (d.depth, d.feat, d.out_grad))
    out = bp.bev_pool_v2(depth, feat, rd, rf, rb, ln, st, (d.cells, case.channels))
    if rf.numel():
        order = stable_argsort(rf, descending=False)
        np.testing.assert_array_equal(order.cpu().numpy(), L.ref_argsort(d.fwd[1], 0))
        rb2, rd2, rf2 = rb[order].contiguous(), rd[order].contiguous(), rf[order].contiguous()
        head = torch.ones(rf2.shape[0], dtype=torch.bool, device=rf2.device)
        head[1:] = rf2[1:] != rf2[:-1]
        st2 = torch.nonzero(head).squeeze(1).to(torch.int32)
        ln2 = torch.diff(torch.cat([st2, torch.tensor([rf2.shape[0]], dtype=torch.int32, device=rf2.device)])).to(torch.int32)
    else:
        rb2, rd2, rf2, st2, ln2 = rb, rd, rf, st, ln
    dg, fg = bp.bev_pool_v2_bkwd(grad, depth, feat, rd2, rf2, rb2, ln2, st2)
    torch.cuda.synchronize()
    _check_pool(case, out.cpu().numpy(), dg.cpu().numpy(), fg.cpu().numpy())


@pytest.mark.parametrize("case", L.frustum_cases(), ids=lambda c: c.id)
def test_frustum(case):
    got = L.run_frustum(case)
    want = L.ref_frustum_to_lidar(L.frustum_data(case)[0], case.cams, *L.frustum_data(case)[1:])
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
