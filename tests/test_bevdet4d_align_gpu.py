"""BEVDet4D temporal alignment on the device (paddle3d_amd/bevdet4d.py, csrc/bev_shift.hip) against the reference's
own shift_feature (tests/golden/python_bevdet4d_align.npz) and, bit for bit, against the NumPy restatement in
tests/golden/bevdet4d_align_numpy.py at BEVDet4D's full shape (9 frames x 80 x 128 x 128)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import bevdet4d_align_numpy as ba  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
C, H, W = 80, 128, 128


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _channels_last(a):
    """[B, C, H, W] values as the view voxel_pooling_v2 returns: [B, H, W, C] memory permuted to NCHW."""
    return _t(np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))).permute(0, 3, 1, 2)


def _bits(x):
    return x.cpu().numpy().view(np.uint32)


def _scene(B, seed, nadj=8, far=None, bda_kw=None):
    rng = np.random.default_rng(seed)
    rots, trans = ba.poses(rng, B, nadj, far=far)
    feats = [ba.features(rng, (B, C, H, W)) for _ in range(nadj + 1)]
    bda = np.broadcast_to(ba.bda_matrix(**(bda_kw or dict(rot_deg=7.0, flip_x=True))), (B, 3, 3)).copy()
    return feats, rots, trans, bda


def _numpy(feats, rots, trans, bda):
    n = len(feats) - 1
    return ba.align_concat(feats, [rots[0]] * n, [trans[0]] * n, rots[1:], trans[1:], [bda] * n)


def _device(feats_dev, rots, trans, bda, return_grid=True):
    from paddle3d_amd import bevdet4d

    return bevdet4d.align_concat(feats_dev, [_t(r) for r in rots], [_t(t) for t in trans], _t(bda),
                                 return_grid=return_grid)


@pytest.mark.parametrize("B", [1, 2])
def test_full_shape_bit_exact_vs_restatement(B):
    feats, rots, trans, bda = _scene(B, 100 + B)
    want, want_grid = _numpy(feats, rots, trans, bda)
    out, grid = _device([_t(f) for f in feats], rots, trans, bda)
    assert tuple(out.shape) == (B, 9 * C, H, W) and out.is_contiguous()
    assert tuple(grid.shape) == (8 * B, H, W, 2)
    np.testing.assert_array_equal(_bits(grid), want_grid.view(np.uint32))
    np.testing.assert_array_equal(_bits(out), want.view(np.uint32))
    # realistic motion: most of every shifted slice is in range, some of it is not
    zero = (want[:, C:] == 0).mean()
    assert 0.0 < zero < 0.3


def test_shift_feature_vs_reference_golden():
    from paddle3d_amd import bevdet4d

    gold = np.load(os.path.join(HERE, "golden", "python_bevdet4d_align.npz"))
    for i in range(len(ba.GOLDEN_CASES)):
        c = ba.golden_case(i)
        out, grid = bevdet4d.shift_feature(_t(c["input"]), [_t(t) for t in c["trans"]], [_t(r) for r in c["rots"]],
                                           _t(c["bda"]), None if c["bda_adj"] is None else _t(c["bda_adj"]),
                                           return_grid=True)
        o, g = ba.at_pixels(out.cpu().numpy(), grid.cpu().numpy(), ba.golden_pixels(i))
        assert o.shape == gold[f"out_{i}"].shape and g.shape == gold[f"grid_{i}"].shape
        assert np.abs(g - gold[f"grid_{i}"]).max() <= 2e-6, c["name"]
        assert np.abs(o - gold[f"out_{i}"]).max() <= 3e-4, c["name"]
        # and bit for bit the restatement
        want, want_grid = ba.shift_feature(c["input"], c["trans"], c["rots"], c["bda"], c["bda_adj"])
        np.testing.assert_array_equal(_bits(grid), want_grid.view(np.uint32))
        np.testing.assert_array_equal(_bits(out), want.view(np.uint32))


def test_torch_grid_sample_on_the_kernels_grid():
    feats, rots, trans, bda = _scene(2, 201, nadj=3)
    fd = [_t(f) for f in feats]
    out, grid = _device(fd, rots, trans, bda)
    for k in range(1, 4):
        ref = torch.nn.functional.grid_sample(fd[k], grid[(k - 1) * 2:k * 2], mode="bilinear", padding_mode="zeros",
                                              align_corners=True)
        assert float((out[:, k * C:(k + 1) * C] - ref).abs().max()) <= 1e-6


def test_channels_last_and_mixed_layouts_give_identical_bits():
    feats, rots, trans, bda = _scene(2, 301, nadj=4)
    base, _ = _device([_t(f) for f in feats], rots, trans, bda)
    cl = [_channels_last(f) for f in feats]
    assert not cl[1].is_contiguous() and cl[1].stride(1) == 1
    got, _ = _device(cl, rots, trans, bda)
    np.testing.assert_array_equal(_bits(got), _bits(base))
    mixed = [_channels_last(f) if k % 2 else _t(f) for k, f in enumerate(feats)]
    got, _ = _device(mixed, rots, trans, bda)
    np.testing.assert_array_equal(_bits(got), _bits(base))
    # a channel slice of a wider map (strided, neither layout) also reads in place
    wide = _t(np.concatenate([feats[2], feats[2]], axis=1))[:, C:]
    got, _ = _device([_t(feats[0]), _t(feats[1]), wide, _t(feats[3]), _t(feats[4])], rots, trans, bda)
    np.testing.assert_array_equal(_bits(got), _bits(base))


def test_current_frame_is_copied_bit_for_bit():
    feats, rots, trans, bda = _scene(2, 401, nadj=2)
    cur = feats[0].copy()
    cur[0, 0, 0, :4] = [-0.0, np.float32(1e-42), np.inf, -np.inf]  # signed zero, denormal, infinities
    feats[0] = cur
    for dev_cur in (_t(cur), _channels_last(cur)):
        out, _ = _device([dev_cur, _t(feats[1]), _t(feats[2])], rots, trans, bda)
        np.testing.assert_array_equal(_bits(out[:, :C]), cur.view(np.uint32))


def test_far_pose_gives_all_zero_slice():
    feats, rots, trans, bda = _scene(1, 501, nadj=2)
    trans[2] = trans[2] + np.float32(1.0e4)  # adjacent frame 2 about 1e4 m away
    out, grid = _device([_t(f) for f in feats], rots, trans, bda)
    assert not bool(out[:, 2 * C:].any())
    assert bool(out[:, C:2 * C].any())
    assert bool(torch.isfinite(grid).all()) and float(grid[1:].abs().min()) > 10.0


def test_sequential_equals_align_concat():
    from paddle3d_amd import bevdet4d

    nadj = bevdet4d.BEVDET4D_NUM_ADJ
    feats, rots, trans, bda = _scene(1, 601, nadj=nadj)
    whole, _ = _device([_t(f) for f in feats], rots, trans, bda)
    feat_prev = _t(np.concatenate(feats[1:], axis=0))  # [num_adj, C, H, W]
    trans_curr = _t(trans[0]).repeat(nadj, 1, 1)
    rots_curr = _t(rots[0]).repeat(nadj, 1, 1, 1)
    trans_prev = _t(np.concatenate(trans[1:], axis=0))
    rots_prev = _t(np.concatenate(rots[1:], axis=0))
    bda_curr = _t(bda).repeat(nadj, 1, 1)
    seq = bevdet4d.align_concat_sequential(_t(feats[0]), feat_prev, trans_curr, trans_prev, rots_curr, rots_prev,
                                           bda_curr)
    assert tuple(seq.shape) == (1, (nadj + 1) * C, H, W)
    np.testing.assert_array_equal(_bits(seq), _bits(whole))


def test_path_does_not_synchronise():
    from paddle3d_amd import bevdet4d

    feats, rots, trans, bda = _scene(2, 701, nadj=8)
    fd = [_channels_last(f) if k % 2 else _t(f) for k, f in enumerate(feats)]
    rd, td, bd = [_t(r) for r in rots], [_t(t) for t in trans], _t(bda)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = bevdet4d.align_concat(fd, rd, td, bd)
        one = bevdet4d.shift_feature(fd[3], [td[0], td[3]], [rd[0], rd[3]], bd, bd)
        seq = bevdet4d.align_concat_sequential(fd[0][:1], torch.cat([f[:1] for f in fd[1:]]), td[0][:1].repeat(8, 1, 1),
                                               torch.cat([t[:1] for t in td[1:]]), rd[0][:1].repeat(8, 1, 1, 1),
                                               torch.cat([r[:1] for r in rd[1:]]), bd[:1].repeat(8, 1, 1))
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.equal(one, out[:, 3 * C:4 * C])
    assert torch.equal(seq, out[:1])


def test_refusals():
    from paddle3d_amd import bevdet4d

    feats, rots, trans, bda = _scene(1, 801, nadj=1)
    fd = [_t(f) for f in feats]
    rd, td, bd = [_t(r) for r in rots], [_t(t) for t in trans], _t(bda)
    for dt in (torch.float16, torch.float64):
        with pytest.raises(RuntimeError, match="bevdet4d_align"):
            bevdet4d.align_concat([fd[0], fd[1].to(dt)], rd, td, bd)
        with pytest.raises(RuntimeError, match="bevdet4d_align"):
            bevdet4d.shift_feature(fd[1], td, [rd[0].to(dt), rd[1]], bd)
    with pytest.raises(RuntimeError, match="bevdet4d_align"):
        bevdet4d.align_concat([fd[0], fd[1].cpu()], rd, td, bd)
    with pytest.raises(RuntimeError, match="bevdet4d_align"):
        bevdet4d.shift_feature(fd[1], [td[0].cpu(), td[1]], rd, bd)
    with pytest.raises(RuntimeError, match="bevdet4d_align"):
        bevdet4d.align_concat([fd[0], fd[1][:, :40]], rd, td, bd)  # C mismatch
    with pytest.raises(RuntimeError, match="bevdet4d_align"):
        bevdet4d.align_concat([fd[0], fd[1][:, :, :64]], rd, td, bd)  # H mismatch
    with pytest.raises(RuntimeError, match="bevdet4d_align"):
        bevdet4d.align_concat(fd, [rd[0], rd[1][..., :2]], td, bd)  # pose shape
    with pytest.raises(RuntimeError, match="bevdet4d_align"):
        bevdet4d.align_concat(fd, rd, td, bd.repeat(2, 1, 1))  # bda batch
    with pytest.raises(RuntimeError, match="bevdet4d_align"):
        bevdet4d.align_concat(fd, rd[:1], td, bd)  # one pose per frame
