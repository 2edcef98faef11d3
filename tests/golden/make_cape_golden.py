"""Golden vectors for CAPE / CAPE-T's attention layers: tests/golden/python_cape.npz.

    python tests/golden/make_cape_golden.py      (needs the reference checkout; the tests only read the .npz)

The reference's own Python is executed by line range through tests/golden/paddle_shim.py (make_petr_golden.py's
technique), from paddle3d/models/layers/cape_transformer.py:
    QcR_Modulation, V_R_Modulation, pos2posemb3d     :47-91
    SELayer                                          :94-106
    CrossAttention, MLP                              :166-285
    CrossViewAttention                               :700-757
    prepare_emb's world transform                    :540-541, :556-557 (two statements each, run on their own)
    pos2posemb3d's dim_t                             :79-80
What the shim lacks is added here, not in paddle_shim.py: nn.LayerNorm / GELU / Sigmoid / Dropout (torch's), nn.LayerDict
(torch's ModuleDict), paddle.einsum, paddle.full.  paddle.nn.MultiHeadAttention is not in the reference tree and is
restated from its formula as make_petr_golden.py does (q_proj, k_proj, v_proj, out_proj; product = matmul(q * head_dim **
-0.5, k^T); softmax; matmul with v; no dropout at inference).

Every method runs in float32 and in float64 from the same float32 inputs and parameters; each result is stored as the
float64 run with make_bevformer_golden.bound (4 x the difference of the two runs, one fp32 ulp of the largest magnitude
as floor).  Inputs and parameters are regenerated from seeds (inputs(tag), state(tag)); the file holds results, bounds
and the reference's state-dict keys with their shapes.  The transformer's cases are described at TR_CASES.

Cases (hidden 64; cameras of 5 x 7 feature tokens; masks from cameras smaller than the padded image):
    a   2 heads of 32, Q = 37, B = 1, N = 3
    b   4 heads of 16, Q = 37, B = 2 (two frames, as with_time stacks them), N = 2; frame 1's camera 0 wholly masked
    c   2 heads of 32, Q = 16, B = 1, N = 1, all but three tokens masked
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_bevformer_golden import bound  # noqa: E402

REF = os.environ.get("PD3_REFERENCE", "/root/reference")
SRC = "paddle3d/models/layers/cape_transformer.py"
OUT = os.path.join(HERE, "python_cape.npz")
F32 = np.float32

HIDDEN = 64
FEAT = (5, 7)
K = FEAT[0] * FEAT[1]
POS_FEATS = HIDDEN // 2          # the reference's hidden_dim // 2: 3 * POS_FEATS = hidden * 3 // 2
BOUND = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
CASES = {
    "a": dict(seed=11, heads=2, dim_head=32, Q=37, B=1, N=3, valid=[[(5, 7), (4, 7), (5, 5)]]),
    "b": dict(seed=12, heads=4, dim_head=16, Q=37, B=2, N=2, valid=[[(5, 6), (3, 7)], [(0, 0), (5, 7)]]),
    "c": dict(seed=13, heads=2, dim_head=32, Q=16, B=1, N=1, valid=[[(1, 3)]]),
}
TAGS = tuple(CASES)
RESULTS = ("posemb", "posemb_world", "qcr", "v_r", "se", "ca_core", "ca", "cva", "cva0")
DIM_T_FEATS = (8, 32, 96, 128)


def results(tag):
    """The layer-level results stored for a case (the modulations and SELayer of case b, 230 KB, are left out: cases a and
    c hold the same modules)."""
    return tuple(r for r in RESULTS if tag != "b" or r not in ("qcr", "v_r", "se"))


def masks(tag):
    """bool [B, N, K]: true outside each camera's own (rows, columns) of the 5 x 7 map."""
    c = CASES[tag]
    m = np.ones((c["B"], c["N"]) + FEAT, bool)
    for b, cams in enumerate(c["valid"]):
        for n, (h, w) in enumerate(cams):
            m[b, n, :h, :w] = False
    return m.reshape(c["B"], c["N"], K)


def inputs(tag):
    c = CASES[tag]
    rng = np.random.default_rng(c["seed"])
    B, N, Q = c["B"], c["N"], c["Q"]
    f = lambda *s: rng.standard_normal(s).astype(F32)  # noqa: E731
    yaw = rng.uniform(-np.pi, np.pi, (B, N))
    R = np.zeros((B, N, 3, 3), F32)
    R[..., 0, 0], R[..., 0, 1], R[..., 1, 0], R[..., 1, 1] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw)
    R[..., 2, 2] = 1
    R = (R + 0.01 * f(B, N, 3, 3)).astype(F32)
    return dict(x=f(B, Q, HIDDEN), lidar_obj_pe=f(B, Q, HIDDEN), feature=f(B, N, K, HIDDEN), camera_pe=f(B, N, HIDDEN),
                img_embed=f(B, N, K, HIDDEN), bev_embed=f(B, N, Q, HIDDEN), mask=masks(tag), R=R,
                t=rng.uniform(-1.5, 1.5, (B, N, 3)).astype(F32), ref_points=rng.random((B, Q, 3)).astype(F32))


def state(tag, shapes):
    """Parameters under the reference's keys (Paddle's [in, out] Linear weights) for {key: shape}."""
    rng = np.random.default_rng(CASES[tag]["seed"] + 100)
    st = {}
    for k in sorted(shapes):
        s = tuple(shapes[k])
        if k.endswith(BUFFERS):
            continue
        if k.endswith("reference_points.weight"):
            st[k] = rng.uniform(0.05, 0.95, s).astype(F32)
        elif k.endswith(("scale_a", "scale_g")):
            st[k] = rng.uniform(-0.3, 0.3, s).astype(F32)
        elif len(s) == 1 and k.endswith("weight"):  # LayerNorm scale
            st[k] = rng.uniform(0.5, 1.5, s).astype(F32)
        elif len(s) == 1:
            st[k] = rng.normal(0, 0.1, s).astype(F32)
        else:
            st[k] = (rng.normal(0, 1, s) / np.sqrt(s[0])).astype(F32)
    return st


# ---- the transformer's cases: a without time (3 cameras), b with time (2 x 2 cameras, one frame-set), c one camera most
# of whose frustum lies outside cam_position_range (coordinates and coords_mask only)
TR = dict(layers=2, feat_dim=16, stride=32, image=(160, 224), depth_start=1, depth_num=4)
TR_CASES = {"a": dict(with_time=False, cams=3, focal=110.0), "b": dict(with_time=True, cams=2, focal=90.0),
            "c": dict(with_time=False, cams=1, focal=30.0)}
TR_RESULTS = {"a": ("coords3d", "tr"), "b": ("coords3d", "mf_a", "mf_b", "tr_time", "tr_prev"), "c": ("coords3d",)}
EGO_PREV = 6  # the reference reads img_metas[0]['extrinsics'][6]: the first camera of the previous frame of six


def tr_inputs(tag):
    """feature [1, nc, C, 5, 7], mask bool [1, nc, 5, 7], I_inv, R_inv [1, nc, 3, 3], t [1, nc, 3, 1], and the two
    extrinsics the ego matrix is made of (4 x 4, as img_metas holds them); nc = cams, doubled with time."""
    c, t = CASES[tag], TR_CASES[tag]
    rng = np.random.default_rng(c["seed"] + 500)
    nc = t["cams"] * (2 if t["with_time"] else 1)
    base = inputs(tag)
    h, w = TR["image"]
    K = np.array([[t["focal"], 0, w / 2], [0, t["focal"], h / 2], [0, 0, 1]], np.float64)
    I_inv = np.stack([np.linalg.inv(K * np.array([[s, 1, 1], [1, s, 1], [1, 1, 1]])) for s in rng.uniform(0.9, 1.1, nc)])
    R = base["R"].reshape(nc, 3, 3).astype(np.float64)

    def rigid():
        a = rng.uniform(-0.2, 0.2)
        m = np.eye(4)
        m[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        m[:3, 3] = rng.uniform(-1, 1, 3)
        return m.astype(F32)

    return dict(feature=rng.standard_normal((1, nc, TR["feat_dim"]) + FEAT).astype(F32),
                mask=(masks(tag) & (tag != "c")).reshape((1, nc) + FEAT), I_inv=I_inv.astype(F32)[None],
                R_inv=np.linalg.inv(R).astype(F32)[None], t=base["t"].reshape(1, nc, 3, 1),
                ext_cur=rigid(), ext_prev=rigid())


def tr_args(tag):
    """CAPETransformer's constructor arguments but att_layer."""
    t = TR_CASES[tag]
    return dict(num_cameras=t["cams"], num_layers=TR["layers"], feat_dim=TR["feat_dim"], feat_stride=TR["stride"],
                image_height=TR["image"][0], image_width=TR["image"][1], bound=BOUND, with_fpe=True,
                depth_start=TR["depth_start"], depth_num=TR["depth_num"], tf_layer=dict(hidden_dim=HIDDEN),
                with_time=t["with_time"])


# ---- the head's cases: a without time (3 cameras), b with time and the prev-frame branches (2 x 6 cameras: the reference
# reads the previous frame's first camera at index 6 of the frame's extrinsics); 10 classes, code size 10, 2 levels
HEAD_CASES = {"a": dict(cams=3), "b": dict(cams=6)}
PC_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
POST = [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]
CLASSES, CODE, MAX_NUM = 10, 10, 20
HEAD_RESULTS = ("head_cls", "head_bbox")


def decode_cfg(tag):
    return dict(B=1, max_num=MAX_NUM, code=CODE, K=CLASSES, thr=None, post=POST)


def head_tr_args(tag):
    return dict(tr_args(tag), num_cameras=HEAD_CASES[tag]["cams"])


def head_inputs(tag):
    """feature [1, nc, C, 5, 7], intrinsics [1, nc, 4, 4], extrinsics [1, nc, 4, 4] (lidar2cam; img_metas holds their
    transposes), img_shape [nc] (h, w) inside the padded image, timestamp [1, 12]."""
    c, t = CASES[tag], TR_CASES[tag]
    rng = np.random.default_rng(c["seed"] + 700)
    nc = HEAD_CASES[tag]["cams"] * (2 if t["with_time"] else 1)
    h, w = TR["image"]
    intr, ext = np.zeros((nc, 4, 4), F32), np.zeros((nc, 4, 4), F32)
    for i in range(nc):
        f = t["focal"] * rng.uniform(0.9, 1.1)
        intr[i] = [[f, 0, w / 2, 0], [0, f, h / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
        yaw = rng.uniform(-np.pi, np.pi)
        fwd, right = np.array([np.cos(yaw), np.sin(yaw), 0.0]), np.array([np.sin(yaw), -np.cos(yaw), 0.0])
        R = np.stack([right, [0.0, 0.0, -1.0], fwd]) + 0.01 * rng.standard_normal((3, 3))  # rows: the camera's x, y, z
        ext[i, :3, :3], ext[i, :3, 3], ext[i, 3, 3] = R, rng.uniform(-1.0, 1.0, 3), 1
    sizes = [(h, w), (h - 32, w), (h, w - 64), (h - 64, w - 32)]
    stamp = np.concatenate([rng.uniform(0, 0.02, 6), 0.5 + rng.uniform(0, 0.02, 6)]).astype(F32)
    return dict(feature=rng.standard_normal((1, nc, TR["feat_dim"]) + FEAT).astype(F32), intrinsics=intr[None],
                extrinsics=ext[None], img_shape=[sizes[i % 4] for i in range(nc)], timestamp=stamp[None])


def check_selection(g, tag, name="head"):
    """The conditions under which the decode's selection cannot depend on rounding (make_bevformer_decoder_golden's): among
    the frame's max_num + 1 largest float64 scores neighbours differ by more than twice the score bound, and no selected
    centre is within the box bound of a face of post_center_range."""
    s = g[f"{tag}_{name}_all_scores"]
    sb, bb = float(g[f"{tag}_{name}_scores_bound"]), float(g[f"{tag}_{name}_boxes_bound"])
    top = np.sort(s[0])[::-1][:MAX_NUM + 1]
    gap = float(np.min(top[:-1] - top[1:]))
    assert gap > 2 * sb, (tag, name, "neighbouring scores", gap, sb)
    ctr, faces = g[f"{tag}_{name}_centres"], np.asarray(POST, np.float64)
    margin = float(min(np.abs(ctr - faces[:3]).min(), np.abs(ctr - faces[3:]).min()))
    assert margin > bb, (tag, name, "a centre within the bound of a range face", margin, bb)
    return dict(gap=gap, score_bound=sb, face_margin=margin, counts=g[f"{tag}_{name}_count"].tolist())


BUFFERS = ("image_plane", "bound", "cam_bound")  # made by the constructor, not drawn by state()


def load():
    return dict(np.load(OUT))


def key_shapes(g, tag, name):
    return json.loads(str(g[f"{tag}_keys_{name}"]))


# ---- the reference run (needs the reference checkout) ---------------------------------------------------------------


def _install(dt):
    import paddle_shim as ps

    p = ps.install(REF)
    nn = p.nn
    ps._DT["float32"] = dt
    p.float32 = dt
    plain = lambda t: t.as_subclass(torch.Tensor) if isinstance(t, torch.Tensor) else t  # noqa: E731
    # 'b n Q d, b n K d -> b n Q K' (spaces between the axes) -> 'bnQd,bnKd->bnQK'
    p.einsum = lambda eq, *ops: ps._wrap(torch.einsum(eq.replace(" ", ""), *[plain(o) for o in ops]))
    p.full = lambda shape, value, dtype=None: ps._wrap(torch.full(tuple(int(s) for s in shape), value,
                                                                  dtype=ps._dt(dtype) if dtype is not None else dt))
    nn.LayerNorm = torch.nn.LayerNorm
    nn.GELU = torch.nn.GELU
    nn.Sigmoid = torch.nn.Sigmoid
    nn.Dropout = torch.nn.Dropout
    nn.LayerDict = torch.nn.ModuleDict
    to_tensor = p.to_tensor  # the head makes float32 arrays of the camera matrices: the float64 run takes them as float64

    def to_dt(data, dtype=None, **k):
        t = to_tensor(data, dtype=dtype, **k)
        return ps._wrap(t.to(dt)) if t.is_floating_point() else t

    p.to_tensor = to_dt
    nn.Embedding = torch.nn.Embedding
    nn.ReLU = torch.nn.ReLU
    import paddle.nn.functional as F
    import torch.nn.functional as TF
    F.interpolate = lambda x, size=None, **k: ps._wrap(TF.interpolate(plain(x), size=tuple(int(v) for v in size)))
    p.full_like = lambda x, v, dtype=None: ps._wrap(torch.full_like(plain(x), v))
    p.isnan = lambda x: ps._wrap(torch.isnan(x))
    p.log = lambda x: ps._wrap(torch.log(x))
    p.maximum = lambda x, y: ps._wrap(torch.maximum(x, y))
    ps.Tensor.clip = lambda self, min=None, max=None: torch.clamp(self, min=min, max=max)
    reg = torch.nn.Module.register_buffer
    nn.Layer.register_buffer = lambda self, name, t, persistable=True: reg(self, name, t.as_subclass(torch.Tensor))

    class MultiHeadAttention(nn.Layer):
        def __init__(self, embed_dim, num_heads, dropout=0.0):
            super().__init__()
            self.num_heads, self.head_dim = num_heads, embed_dim // num_heads
            for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
                setattr(self, n, nn.Linear(embed_dim, embed_dim))

        def forward(self, query, key=None, value=None, attn_mask=None):
            b, m, d = query.shape[0], self.num_heads, self.head_dim
            q, k, v = (plain(proj(t)).reshape(b, -1, m, d).permute(0, 2, 1, 3) for proj, t in
                       ((self.q_proj, query), (self.k_proj, key), (self.v_proj, value)))
            product = torch.matmul(q * (d ** -0.5), k.transpose(-1, -2))
            assert attn_mask is None
            out = torch.matmul(torch.softmax(product, -1), v).permute(0, 2, 1, 3).reshape(b, -1, m * d)
            return self.out_proj(out)

    nn.MultiHeadAttention = MultiHeadAttention
    return ps, p


def _reference(tag, dt):
    import paddle_shim as ps

    saved = torch.get_default_dtype()
    torch.set_default_dtype(dt)
    try:
        ps, p = _install(dt)
        return _run(tag, dt, ps, p)
    finally:
        ps._DT["float32"] = torch.float32
        torch.set_default_dtype(saved)


def _run(tag, dt, ps, p):
    import types

    import paddle.nn.functional as F

    c, inp = CASES[tag], inputs(tag)
    T = lambda a: ps._wrap(torch.from_numpy(np.ascontiguousarray(a)).to(dt) if a.dtype != bool  # noqa: E731
                           else torch.from_numpy(np.ascontiguousarray(a)))
    ns = dict(paddle=p, F=F, nn=p.nn, np=np, math=__import__("math"), copy=__import__("copy"),
              recompute=None, manager=sys.modules["paddle3d.apis"].manager)
    path = os.path.join(REF, SRC)
    ps.exec_lines(path, [(47, 91), (94, 106), (166, 285), (700, 757)], ns)
    ns["List"] = __import__("typing").List
    ns["param_init"] = sys.modules["paddle3d.models.layers.param_init"]
    ps.exec_lines(os.path.join(REF, "paddle3d/models/layers/layer_libs.py"), [(252, 258)], ns)
    ps.exec_lines(path, [(109, 162), (289, 697)], ns)
    out, keys = {}, {}

    def build(name, cls, *args, **kw):
        mod = ns[cls](*args, **kw)
        shapes = {k: list(v.shape) for k, v in mod.state_dict().items()}
        keys[name] = shapes
        st = state(tag, {f"{name}.{k}": s for k, s in shapes.items()})
        mod = mod.to(dt).eval()
        with torch.no_grad():
            for k, v in mod.state_dict().items():
                if f"{name}.{k}" in st:
                    v.copy_(torch.from_numpy(st[f"{name}.{k}"]).to(dt))
        return mod

    n = lambda t: t.detach().as_subclass(torch.Tensor).numpy()  # noqa: E731
    with torch.no_grad():
        i = {k: T(v) for k, v in inp.items()}
        out["posemb"] = n(ns["pos2posemb3d"](i["ref_points"], POS_FEATS))
        # prepare_emb's statements on their own: ref_points * (bound[1] - bound[0]) + bound[0]; + t; R @
        w = dict(ns, self=types.SimpleNamespace(bound=T(np.asarray(BOUND, F32).reshape(2, 3))), ref_points=i["ref_points"],
                 t=i["t"], R=i["R"])
        ps.exec_lines(path, [(540, 541)], w)
        w["ref_points_unormalized"] = w["ref_points_unormalized"][:, None]
        ps.exec_lines(path, [(556, 557)], w)
        out["posemb_world"] = n(ns["pos2posemb3d"](w["world"], 8))
        qcr, v_r = build("QcR", "QcR_Modulation", HIDDEN), build("V_R", "V_R_Modulation", HIDDEN)
        out["qcr"] = n(qcr(i["x"], i["R"]))
        out["v_r"] = n(v_r(i["feature"], i["R"]))
        se = build("fpe", "SELayer", HIDDEN)
        out["se"] = n(se(i["img_embed"], i["feature"]))
        ca = build("cross_attend", "CrossAttention", HIDDEN, c["heads"], c["dim_head"], True)
        tap = {}
        ca.proj.register_forward_pre_hook(lambda m, a: tap.__setitem__("core", a[0].detach().clone()))
        k_a, q_a = i["feature"] + i["camera_pe"][:, :, None], i["x"] + i["lidar_obj_pe"]
        out["ca"] = n(ca(i["img_embed"], i["bev_embed"], k_a, q_a, i["feature"], i["mask"]))
        out["ca_core"] = n(tap["core"])
        for name, cond in (("cva", True), ("cva0", None)):
            layer = build(name, "CrossViewAttention", c["Q"], HIDDEN, True, heads=c["heads"], dim_head=c["dim_head"],
                          conditional=bool(cond))
            out[name] = n(layer(i["x"], T(out["qcr"]), i["lidar_obj_pe"], i["feature"], i["camera_pe"], i["mask"],
                                i["img_embed"], i["bev_embed"], None))
        # ---- the transformer (position_embeding, prepare_emb, forward) and MLP_Fusion with Ego_emb
        ti = tr_inputs(tag)
        tc = TR_CASES[tag]
        ext = [np.eye(4, dtype=F32)] * (EGO_PREV + 1)
        ext[0], ext[EGO_PREV] = ti["ext_cur"], ti["ext_prev"]
        nc = ti["feature"].shape[1]
        metas = [dict(pad_shape=[TR["image"] + (3,)], lidar2img=[np.eye(4)] * nc, extrinsics=ext)]
        taps = {}
        inv_sig = ns["inverse_sigmoid"]
        ns["inverse_sigmoid"] = lambda x: (taps.__setitem__("norm", n(x).copy()), inv_sig(x))[1]
        att = ns["CrossViewAttention"](c["Q"], HIDDEN, True, heads=c["heads"], dim_head=c["dim_head"])
        tr = build("tr", "CAPETransformer", att_layer=att, **tr_args(tag))
        tf, tm, tI = T(ti["feature"]), T(ti["mask"]), T(ti["I_inv"])
        hook = tr.position_encoder.register_forward_pre_hook(
            lambda m, x: taps.__setitem__("coords3d", n(x[0]).copy()))
        _, cmask = tr.position_embeding(tf.reshape([-1, tc["cams"], TR["feat_dim"], *FEAT]),
                                        tI.reshape([-1, tc["cams"], 3, 3]), metas, tm.reshape([-1, tc["cams"], *FEAT]))
        hook.remove()
        out["coords3d"], out["coords_norm"], out["coords_mask"] = taps["coords3d"], taps["norm"], n(cmask)
        if "tr" in TR_RESULTS[tag]:
            out["tr"] = n(tr(tf, tm, tI, T(ti["R_inv"]), T(ti["t"]), metas)[0])
        if "tr_time" in TR_RESULTS[tag]:
            cur, prev = tr(tf, tm, tI, T(ti["R_inv"]), T(ti["t"]), metas, return_prev_query=True)[:2]
            out["tr_time"], out["tr_prev"] = n(cur), n(prev)
            mf = build("mf", "MLP_Fusion", HIDDEN)
            a_, b_ = mf(i["x"][:1], i["x"][1:], metas)
            out["mf_a"], out["mf_b"] = n(a_), n(b_)
        # ---- the head: forward's eval path (both levels) and get_bboxes on the last level
        if tag in HEAD_CASES:
            from make_bevformer_decoder_golden import _pad_decode

            HEAD_PY = os.path.join(REF, "paddle3d/models/heads/dense_heads/cape_dn_head.py")
            assigner = "paddle3d/models/heads/dense_heads/target_assigner/hungarian_assigner.py"
            nan_to_num = ps.exec_lines(os.path.join(REF, assigner), [(38, 69)], dict(ns))["nan_to_num"]
            hns = dict(ns, nan_to_num=nan_to_num, inverse_sigmoid=inv_sig)
            ps.exec_lines(HEAD_PY, [(209, 228), (423, 592), (983, 1002)], hns)
            denorm = ps.exec_lines(os.path.join(REF, "paddle3d/utils/box.py"), [(107, 138)], dict(ns))["denormalize_bbox"]
            coder_fns = ps.exec_lines(os.path.join(REF, "paddle3d/utils/box_coder.py"), [(133, 214)],
                                      dict(ns, denormalize_bbox=denorm))
            coder = types.SimpleNamespace(point_cloud_range=PC_RANGE, post_center_range=list(POST), max_num=MAX_NUM,
                                          score_threshold=None, num_classes=CLASSES)
            coder.decode_single = lambda *a: coder_fns["decode_single"](coder, *a)
            coder.decode = lambda d: coder_fns["decode"](coder, d)
            lin, nn_ = p.nn.Linear, p.nn

            class _Head(nn_.Layer):  # the parameters of CAPETemporalDNHead (_init_layers, :166-194) around the transformer
                def __init__(self):
                    super().__init__()
                    self.transformer = ns["CAPETransformer"](att_layer=ns["CrossViewAttention"](
                        c["Q"], HIDDEN, True, heads=c["heads"], dim_head=c["dim_head"]), **head_tr_args(tag))
                    self.code_weights = torch.nn.Parameter(torch.ones(CODE))
                    self.cls_branches = nn_.LayerList([nn_.Sequential(
                        lin(HIDDEN, HIDDEN), nn_.LayerNorm(HIDDEN), nn_.ReLU(), lin(HIDDEN, HIDDEN), nn_.LayerNorm(HIDDEN),
                        nn_.ReLU(), lin(HIDDEN, CLASSES)) for _ in range(6)])
                    self.reg_branches = nn_.LayerList([nn_.Sequential(
                        lin(HIDDEN, HIDDEN), nn_.ReLU(), lin(HIDDEN, HIDDEN), nn_.ReLU(), lin(HIDDEN, CODE))
                        for _ in range(6)])

            ns["_Head"] = _Head
            head = build("head", "_Head")
            head.position_level, head.with_time, head.with_prev_aux_loss = 0, tc["with_time"], tc["with_time"]
            head.pc_range, head.bbox_coder = PC_RANGE, coder
            head._get_camera_parameters = types.MethodType(hns["_get_camera_parameters"], head)
            hi = head_inputs(tag)
            hnc = hi["feature"].shape[1]
            hmetas = [dict(pad_shape=[TR["image"] + (3,)], img_shape=[sh + (3,) for sh in hi["img_shape"]],
                           lidar2img=[np.eye(4)] * hnc, extrinsics=[e.T for e in hi["extrinsics"][0]],
                           intrinsics=list(hi["intrinsics"][0]), timestamp=list(hi["timestamp"][0]))]
            houts = hns["forward"](head, [T(hi["feature"])], hmetas)
            out["head_cls"], out["head_bbox"] = n(houts["all_cls_scores"]), n(houts["all_bbox_preds"])
            cls, bbox = (ps._wrap(houts[k].as_subclass(torch.Tensor)[-1:].to(torch.float32).to(dt))
                         for k in ("all_cls_scores", "all_bbox_preds"))
            ret = hns["get_bboxes"](types.SimpleNamespace(bbox_coder=coder), dict(all_cls_scores=cls, all_bbox_preds=bbox),
                                    None)
            out.update(_pad_decode(decode_cfg(tag), "head", cls.as_subclass(torch.Tensor)[0],
                                   bbox.as_subclass(torch.Tensor)[0], ret))
        dims = {}
        for feats in DIM_T_FEATS:
            d = dict(ns, num_pos_feats=feats, temperature=10000)
            ps.exec_lines(path, [(79, 80)], d)
            dims[feats] = n(d["dim_t"])
    return out, keys, dims


def main():
    out = {}
    for tag in TAGS:
        (r32, keys, dims), (r64, _, _) = _reference(tag, torch.float32), _reference(tag, torch.float64)
        for name, shapes in keys.items():
            out[f"{tag}_keys_{name}"] = np.asarray(json.dumps(shapes))
        # every discrete result is the reference's alone: coords_mask equal in both runs, no normalised coordinate within
        # its bound of a clip point (0, 1, eps, 1 - eps), where the coordinate's branch or its logarithm's slope changes
        assert np.array_equal(r32["coords_mask"], r64["coords_mask"]), tag
        assert tag != "c" or 0.5 < r64["coords_mask"].mean() < 1, r64["coords_mask"].mean()  # most, not all, outside
        # (per element, with 4 x the element's own difference of the two runs as its bound: case c's coordinates reach
        # far outside the range, where their error is large and no clip point is near.  The first depth bin is
        # depth_start = cam_position_range[2] itself: z is exactly 0 there in both runs, with no rounding.)
        n32, n64 = r32["coords_norm"].astype(np.float64), r64["coords_norm"]
        clips = (0.0, 1.0, 1e-5, 1.0 - 1e-5)
        exact = np.any([(n32 == x) & (n64 == x) for x in clips], 0)
        dist = np.min([np.abs(n64 - x) for x in clips], 0)
        nb = np.maximum(4 * np.abs(n32 - n64), np.spacing(np.abs(n64).astype(F32)).astype(np.float64))
        assert (dist > nb)[~exact].all(), (tag, "a normalised coordinate within its bound of a clip point")
        margin, nb = float((dist / nb)[~exact].min()), 1.0
        out[f"{tag}_coords_mask"] = r64["coords_mask"]
        print(f"{tag} coords_mask masked {r64['coords_mask'].mean():.2f}, smallest clip distance / bound {margin:.3g} "
              f"> {nb:g}")
        if tag in HEAD_CASES:  # the decode's discrete results are the reference's alone
            for k in ("labels", "rows", "count"):
                assert np.array_equal(r32[f"head_{k}"], r64[f"head_{k}"]), (tag, k, "the two runs select differently")
                out[f"{tag}_head_{k}"] = r64[f"head_{k}"]
            out[f"{tag}_head_all_scores"], out[f"{tag}_head_centres"] = r64["head_all_scores"], r64["head_centres"]
            for k in ("boxes", "scores"):
                out[f"{tag}_head_{k}"] = r64[f"head_{k}"]
                out[f"{tag}_head_{k}_bound"], out[f"{tag}_head_{k}_ref_err"] = bound(r32[f"head_{k}"], r64[f"head_{k}"])
            sb, _ = bound(1 / (1 + np.exp(-r32["head_cls"][-1].astype(np.float64))), 1 / (1 + np.exp(-r64["head_cls"][-1])))
            out[f"{tag}_head_scores_bound"] = np.float64(max(float(sb), float(out[f"{tag}_head_scores_bound"])))
            print(tag, "decode", check_selection(out, tag))
        for name in results(tag) + TR_RESULTS[tag] + (HEAD_RESULTS if tag in HEAD_CASES else ()):
            b, err = bound(r32[name], r64[name])
            assert np.isfinite(r64[name]).all(), (tag, name)  # every query of the cases has an unmasked key
            out[f"{tag}_{name}"], out[f"{tag}_{name}_bound"], out[f"{tag}_{name}_ref_err"] = r64[name], b, err
            print(f"{tag} {name:13s} {str(r64[name].shape):18s} ref err {err:.3e} bound {b:.3e}")
    for feats, d in dims.items():
        assert d.dtype == np.float32
        out[f"dim_t_{feats}"] = d
    m = masks("b")
    assert m[1, 0].all() and not m[1, 1].any() and not masks("a").all(-1).any()
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    main()
