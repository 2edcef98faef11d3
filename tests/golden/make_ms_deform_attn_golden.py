"""Golden vectors for ms_deform_attn from the reference's own Python: the forward methods of BEVFormer's three
attention layers, executed through tests/golden/paddle_shim.py at small seeded shapes,

    TemporalSelfAttention.forward        (models/transformers/attentions/temporal_self_attention.py:140-279)
    MSDeformableAttention3D.forward      (models/transformers/attentions/spatial_cross_attention.py:310-428)
    CustomMSDeformableAttention.forward  (models/transformers/attentions/spatial_cross_attention.py:531-640)

    python tests/golden/make_ms_deform_attn_golden.py     # needs /root/reference; writes python_ms_deform_attn.npz

The methods are executed from their line ranges (the modules' imports drag in the whole framework) on a
SimpleNamespace `self` whose projections are seeded linear maps.  `ms_deform_attn.ms_deform_attn` is bound to an
independent torch formulation (F.grid_sample(align_corners=False, padding_mode="zeros") per level and head, weighted
sum: ms_deform_attn_numpy.grid_sample_attn, evaluated in float64).  Every call records what the caller hands the op --
value, sampling_locations, attention_weights, spatial_shapes, level_start_index, im2col_step -- and the result
(rounded to float32).  That pins the layout contract of the callers: (x, y) order, normalisation by (W, H), the
Z-anchor interleave of MSDeformableAttention3D and TemporalSelfAttention's bev-queue batch.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import ms_deform_attn_numpy as md  # noqa: E402
import paddle_shim as ps  # noqa: E402

REF = "/root/reference"
ATT = os.path.join(REF, "paddle3d/models/transformers/attentions")
TSA = (os.path.join(ATT, "temporal_self_attention.py"), (140, 279))
SCA3D = (os.path.join(ATT, "spatial_cross_attention.py"), (310, 428))
DEC = (os.path.join(ATT, "spatial_cross_attention.py"), (531, 640))

EMBED, HEADS = 64, 2  # C = 32 per head, as in BEVFormer-tiny


def _linear(rng, n_in, n_out, scale):
    w = torch.from_numpy((rng.standard_normal((n_in, n_out)) * scale / np.sqrt(n_in)).astype(np.float32))
    b = torch.from_numpy((rng.standard_normal(n_out) * 0.1 * scale).astype(np.float32))
    return lambda x: ps._wrap(torch.matmul(x.as_subclass(torch.Tensor), w) + b)


def _self(rng, n_in_q, levels, points, extra=None):
    """The attributes the forward methods read; sampling_offsets about one cell of the level."""
    s = types.SimpleNamespace(num_heads=HEADS, num_levels=levels, num_points=points, im2col_step=64,
                              batch_first=True, dropout=lambda x: x)
    nq = extra.get("num_bev_queue", 1) if extra else 1
    s.value_proj = _linear(rng, EMBED, EMBED, 1.0)
    s.sampling_offsets = _linear(rng, n_in_q, HEADS * nq * levels * points * 2, 1.0)
    s.attention_weights = _linear(rng, n_in_q, HEADS * nq * levels * points, 1.0)
    s.output_proj = _linear(rng, EMBED, EMBED, 1.0)
    for k, v in (extra or {}).items():
        setattr(s, k, v)
    return s


def _levels(shapes):
    sh, st, S = md.level_layout(shapes)
    return ps.tensor(sh), ps.tensor(st), S


def main():
    p = ps.install(REF)
    import paddle.nn.functional as F

    calls = []

    def op(value, sampling_locations, attention_weights, spatial_shapes, level_start_index, im2col_step):
        a = [t.as_subclass(torch.Tensor).detach() for t in (value, sampling_locations, attention_weights)]
        sh = spatial_shapes.as_subclass(torch.Tensor).numpy()
        st = level_start_index.as_subclass(torch.Tensor).numpy()
        out = md.grid_sample_attn(*(t.double() for t in a), sh, st)
        calls.append(dict(value=a[0].numpy(), sampling_locations=a[1].numpy(), attention_weights=a[2].numpy(),
                          spatial_shapes=sh, level_start_index=st, im2col_step=np.int64(im2col_step),
                          out=out.float().numpy()))
        return ps._wrap(out.float())

    shim_ops = types.SimpleNamespace(ms_deform_attn=op)
    T = ps.tensor
    out = {}
    rng = np.random.default_rng(2024)

    # TemporalSelfAttention: bev queue of 2 (prev_bev, current), one 8 x 8 BEV level, 4 points
    path, lines = TSA
    ns = ps.exec_lines(path, [lines], dict(paddle=p, F=F, ms_deform_attn=shim_ops, masked_fill=None))
    bs, hw, L = 1, (8, 8), 1
    sh, st, S = _levels([hw])
    q = T(rng.standard_normal((bs, S, EMBED)).astype(np.float32))
    prev = T(rng.standard_normal((bs, S, EMBED)).astype(np.float32))
    value = p.stack([prev, q], 1).reshape([bs * 2, S, EMBED])
    ys, xs = np.meshgrid((np.arange(hw[0]) + 0.5) / hw[0], (np.arange(hw[1]) + 0.5) / hw[1], indexing="ij")
    ref2d = np.stack([xs.reshape(-1), ys.reshape(-1)], -1).astype(np.float32)  # (x, y), as get_reference_points
    ref = T(np.broadcast_to(ref2d[None, :, None, :], (bs * 2, S, L, 2)).copy())
    self = _self(rng, 2 * EMBED, L, 4, dict(num_bev_queue=2))
    with torch.no_grad():
        ns["forward"](self, q, value=value, reference_points=ref, spatial_shapes=sh, level_start_index=st)

    # MSDeformableAttention3D (inside SpatialCrossAttention): 2 rebatched cameras, 2 levels, 4 Z anchors x 2 points
    path, lines = SCA3D
    ns = ps.exec_lines(path, [lines], dict(paddle=p, F=F, ms_deform_attn=shim_ops, masked_fill=None))
    cams, max_len, Z, L = 2, 24, 4, 2
    sh, st, S = _levels([[6, 10], [3, 5]])
    q = T(rng.standard_normal((cams, max_len, EMBED)).astype(np.float32))
    v = T(rng.standard_normal((cams, S, EMBED)).astype(np.float32))
    ref = T(rng.uniform(0.05, 0.95, (cams, max_len, Z, 2)).astype(np.float32))
    self = _self(rng, EMBED, L, 8)
    with torch.no_grad():
        ns["forward"](self, q, value=v, reference_points=ref, spatial_shapes=sh, level_start_index=st)

    # CustomMSDeformableAttention (decoder): 30 object queries over the 10 x 10 BEV, 4 points
    path, lines = DEC
    ns = ps.exec_lines(path, [lines], dict(paddle=p, F=F, ms_deform_attn=shim_ops, masked_fill=None))
    bs, L = 1, 1
    sh, st, S = _levels([[10, 10]])
    q = T(rng.standard_normal((bs, 30, EMBED)).astype(np.float32))
    v = T(rng.standard_normal((bs, S, EMBED)).astype(np.float32))
    ref = T(rng.uniform(0.0, 1.0, (bs, 30, L, 2)).astype(np.float32))
    self = _self(rng, EMBED, L, 4)
    with torch.no_grad():
        ns["forward"](self, q, value=v, reference_points=ref, spatial_shapes=sh, level_start_index=st)

    names = ["tsa", "sca", "decoder"]
    assert len(calls) == len(names)
    for name, c in zip(names, calls):
        for k, a in c.items():
            out[f"{name}_{k}"] = np.ascontiguousarray(a) if np.ndim(a) else np.asarray(a)
        loc = c["sampling_locations"]
        inside = float(((loc >= 0) & (loc <= 1)).all(-1).mean())
        print(f"{name}: value {c['value'].shape}, locations {loc.shape}, {inside:.3f} of the points in [0, 1]^2")
    np.savez_compressed(os.path.join(HERE, "python_ms_deform_attn.npz"), **out)


if __name__ == "__main__":
    main()
