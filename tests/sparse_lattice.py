"""The sparse convolution stack's border lattice (a helper module like tests/conv_lattice.py, not a conftest).

Two halves, both crosses and not products:

* gather-GEMM cases (GemmCase): synthetic neighbour tables -- random rows in [-1, n_in) -- built directly, so that a row
  count is exact and no index builder is involved.  A row sweep per kernel at its tile border (32 / 64 / 128 / 256 rows), the
  16-row block and the 8192-row window, in raster and in tile order, at the exact size and in capacity form (the count in
  device memory, the arrays the next multiple of 8192 rows long); a channel / kernel-volume sweep on both sides of every
  clause of the fp32 dispatch (fp32_path restates it) and over every template instance of the three entries; operands
  at data_ptr() % 16 == 4; every epilogue at the smallest case; the refusals the host-side checks make before a launch.
* index-builder cases (IndexCase): small grids whose geometry, occupancy or size sits on a border of the hash path
  (`indices`) or of the sorted-key path (`plan`), one case with keys at and above 2^31, the grid-size refusals.

References: ref_indices / ref_plan are plain NumPy on coordinates, from the definition and with no key packing;
gather_reference is the float64 gather-matmul tests/test_sparse_conv_gpu.py::test_features_bf16x3_is_fp32_arithmetic
writes out.

Data classes (gemm_data): "exact" = small integers (scale in {-1, 1, 2}) whose every partial sum and output is representable,
so that a kernel must equal the float64 reference bit for bit whatever its summation order -- fp16-rounded and bf16-split
operands are exact there too; "random" = the distributions of tests/test_sparse_conv_gpu.py under the bars it already
holds (BARS).

Everything here runs on the CPU except call_gemm / tile_order_dev, which the GPU tests use.
"""
from __future__ import annotations

import itertools
import zlib
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

SENTINEL = -7.0     # what an output holds where a kernel must not write
WINDOW = 8192       # sp_window_tile / pd3_sparse_tile_order
N_IN = 97           # input rows of the synthetic neighbour tables
TAIL = 8            # sentinel rows allocated behind every output

BARS = {
    "fp32": "abs 2e-4 on unit-variance rows and 1/sqrt(cin * kvol) weights (test_conv_matches_dense_oracle)",
    "x3": "err <= max(2 * err of the fp32 entry, 2e-7 * mag) and err < 2e-6 * mag on normal x log-normal data "
          "(test_features_bf16x3_is_fp32_arithmetic)",
    "f16": "2e-4 * max(1, mag), + 1e-3 * mag where the output is fp16, against float64 on the same fp16-rounded operands "
           "(test_features_f16_matches_fp32_math_on_fp16_operands)",
}


# ---- the fp32 dispatch, restated from pd3_sparse_conv3d_features_ordered (sparse_conv.hip) -------------------------------
def fp32_path(cin, cout, kvol, feats_aligned=True, weight_aligned=True):
    """The kernel the fp32 entry runs: rows<NB,T> (128-row tiles), mfma<NB> (64), valu<1|2> (32; ':goto' where the matrix
    core branch hands over), or refuse:<clause>."""
    if cout > 128:
        return "refuse:cout"
    if cin % 16 == 0 and kvol <= 27 and cout in (16, 32, 64, 128) and weight_aligned and feats_aligned:
        return f"rows<{cout // 16},{8 if cin % 32 == 0 else 4}>"
    via = ""
    if cout % 16 == 0 and weight_aligned and (cin % 4 != 0 or feats_aligned):
        if cout // 16 in (1, 2, 4, 8):
            return f"mfma<{cout // 16}>"
        via = ":goto"
    if (cin * cout + 32 * cin) * 4 + 32 * 4 > 160 * 1024:
        return "refuse:lds"
    return ("valu<1>" if cout <= 64 else "valu<2>") + via


def mma16_path(entry, cin, cout, kvol):
    """Template instance of the f16 / bf16x3 entries (sf_chunk / sx_chunk), or refuse:shape."""
    if cin % 16 or cout not in (32, 64, 128) or kvol > 27:
        return "refuse:shape"
    if entry == "x3":
        return f"x3<{cout // 32},{32 if cin % 32 == 0 else 16}>"
    return f"f16<{cout // 32},{64 if cin % 64 == 0 else (32 if cin % 32 == 0 else 16)}>"


def tile_rows(path):
    for head, tile in (("rows", 128), ("mfma", 64), ("valu", 32), ("x3<", 256), ("f16<", 256)):
        if path.startswith(head):
            return tile
    raise KeyError(path)


# ---- gather-GEMM cases ---------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GemmCase:
    entry: str           # fp32 / x3 / f16 / gg16 (pd3_gather_gemm_f16 through ops.sparse_conv3d.gather_gemm_f16's entry)
    axis: str            # rows / channels / align / epilogue / refuse:<clause>
    rows: int
    cin: int
    cout: int
    kvol: int
    order: bool = False  # rows in tile order (pd3_sparse_tile_order)
    cap: bool = False    # capacity form: the count in device memory, arrays the next multiple of 8192 rows long
    epi: tuple = ("bias", "relu")   # of bias, bn, res, relu
    opt: tuple = ()      # sorted (key, value): out_f32, ld, off, misalign (feats / weight), status, half (scale only)

    def o(self, key, default=None):
        return dict(self.opt).get(key, default)

    @property
    def id(self):
        extra = "".join(f"-{k}{v}" for k, v in self.opt)
        return (f"{self.entry}-{self.axis}-r{self.rows}-ci{self.cin}-co{self.cout}-k{self.kvol}"
                f"{'-order' if self.order else ''}{'-cap' if self.cap else ''}-{'+'.join(self.epi) or 'plain'}{extra}")

    @property
    def path(self):
        fa, wa = self.o("misalign") != "feats", self.o("misalign") != "weight"
        if self.entry == "fp32":
            return fp32_path(self.cin, self.cout, self.kvol, fa, wa)
        return mma16_path("x3" if self.entry == "x3" else "f16", self.cin, self.cout, self.kvol)

    @property
    def out_f16(self):
        return self.entry in ("f16", "gg16") and not self.o("out_f32", False)

    @property
    def alloc_rows(self):
        return (self.rows // WINDOW + 1) * WINDOW if self.cap else self.rows


def _g(entry, axis, rows, cin, cout, kvol, order=False, cap=False, epi=("bias", "relu"), **opt):
    return GemmCase(entry, axis, rows, cin, cout, kvol, order, cap, tuple(epi), tuple(sorted(opt.items())))


# one shape per kernel for the row sweep: (entry, cin, cout), at kernel volume 3
ROW_KERNELS = [("fp32", 4, 8), ("fp32", 5, 16), ("fp32", 16, 16), ("x3", 16, 32), ("f16", 16, 32)]
ROWS_SMALL = 300        # the channel sweep's row count: two tiles of 256 rows, more of the others
CIN_SWEEP = (1, 3, 4, 5, 7, 16, 17, 32, 33, 48, 64, 128)
COUT_SWEEP = (1, 8, 16, 24, 32, 48, 64, 112, 128)
KVOL_SWEEP = (1, 2, 3, 8, 9, 27, 28, 36)
MMA16_CIN, MMA16_COUT, MMA16_KVOL = (16, 32, 48, 64, 128), (32, 64, 128), (1, 3, 27)
EPILOGUES = [tuple(n for n, on in zip(("bias", "bn", "res", "relu"), bits) if on)
             for bits in itertools.product((False, True), repeat=4)]


def row_counts(tile):
    return sorted({1, 15, 16, 17, tile - 1, tile, tile + 1, WINDOW - 1, WINDOW, WINDOW + 1})


def rows_cases():
    out = []
    for entry, cin, cout in ROW_KERNELS:
        tile = tile_rows(_g(entry, "rows", 1, cin, cout, 3).path)
        for rows in row_counts(tile):
            for order in (False, True):
                for cap in (False, True):
                    out.append(_g(entry, "rows", rows, cin, cout, 3, order, cap))
    return out


def channel_cases():
    out = []
    for cout in (16, 24):                      # matrix-core kernels / VALU kernel
        out += [_g("fp32", "channels", ROWS_SMALL, cin, cout, 3) for cin in CIN_SWEEP]
    for cin in (5, 16, 32):                    # mfma<NB> / rows<NB,4> / rows<NB,8>, VALU between them
        out += [_g("fp32", "channels", ROWS_SMALL, cin, cout, 3) for cout in COUT_SWEEP]
    for cin, cout in ((4, 8), (5, 16), (16, 16), (32, 112)):
        out += [_g("fp32", "channels", ROWS_SMALL, cin, cout, k, order=1 < k <= 31) for k in KVOL_SWEEP]
    out.append(_g("fp32", "channels", ROWS_SMALL, 256, 120, 1))   # the largest VALU tile the 160 KiB LDS bound lets through
    for entry in ("x3", "f16"):
        out += [_g(entry, "channels", ROWS_SMALL, cin, cout, k, order=k > 1)
                for cin in MMA16_CIN for cout in MMA16_COUT for k in MMA16_KVOL]
    seen, uniq = set(), []
    for c in out:
        if c.id not in seen:
            seen.add(c.id)
            uniq.append(c)
    return uniq


def align_cases():
    """(case with an operand at data_ptr() % 16 == 4).  fp32: runs, another kernel; the 16-bit entries: status -1."""
    out = []
    for cin, cout in ((16, 16), (5, 16), (16, 128), (32, 48)):
        for which in ("feats", "weight"):
            out.append(_g("fp32", "align", ROWS_SMALL, cin, cout, 3, misalign=which))
    for entry in ("x3", "f16", "gg16"):
        for which in ("feats", "weight"):
            out.append(_g(entry, "align", ROWS_SMALL, 16, 32, 3, misalign=which, status=-1))
    return out


def epilogue_cases():
    out = []
    for entry, cin, cout in ROW_KERNELS:
        out += [_g(entry, "epilogue", 17, cin, cout, 3, epi=e) for e in EPILOGUES]
    out += [_g("f16", "epilogue", 17, 16, 32, 3, epi=e, out_f32=True) for e in ((), ("bias", "bn", "res", "relu"))]
    for ld, off in ((32, 0), (40, 0), (40, 8), (96, 64), (36, 4)):
        out += [_g("gg16", "epilogue", 17, 16, 32, 3, epi=e, ld=ld, off=off) for e in ((), ("bias",), ("bias", "relu"))]
    return out


def refuse_cases():
    """Shapes the host-side checks reject before a launch, with the documented status (-1 invalid, -3 unsupported)."""
    out = [_g("fp32", "refuse:cout<=128", 17, 16, 144, 3, status=-3),
           _g("fp32", "refuse:valu-lds", 17, 272, 120, 1, status=-3)]
    for entry in ("x3", "f16", "gg16"):
        out.append(_g(entry, "refuse:kvol<=27", 17, 16, 32, 28, status=-3))
        out.append(_g(entry, "refuse:cin%16", 17, 24, 32, 3, status=-3))
        out.append(_g(entry, "refuse:cout", 17, 16, 48, 3, status=-3))
    for entry in ("fp32", "x3", "f16"):
        out.append(_g(entry, "refuse:scale-without-shift", 17, 16, 32, 3, epi=("bn",), half=True, status=-1))
    out.append(_g("gg16", "refuse:out_off%4", 17, 16, 32, 3, ld=40, off=2, status=-1))
    out.append(_g("gg16", "refuse:off+cout<=ld", 17, 16, 32, 3, ld=40, off=12, status=-1))
    return out


TILE_ORDER_REFUSALS = [(32, -1), (0, -1)]   # (kernel volume, status) of pd3_sparse_tile_order; 31 is the last it takes


def all_gemm_cases():
    return rows_cases() + channel_cases() + align_cases() + epilogue_cases() + refuse_cases()


# ---- gather-GEMM data ------------------------------------------------------------------------------------------------------
def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def exact_limits(c: GemmCase):
    """(max|x|, max|w|) of the exact class.  fp16 outputs must stay below 2048: a sum of kvol * cin * density products of
    variance (xm (xm + 1) / 3) (wm (wm + 1) / 3), doubled by the scale, is checked on the reference itself."""
    if c.out_f16:
        return (2, 1) if c.cin * c.kvol <= 2048 else (1, 1)
    return 4, 2


def exact_bound(c: GemmCase):
    return 2048.0 if c.out_f16 else 2.0 ** 24


def _gemm_data(c: GemmCase, kind: str):
    return _gemm_data_of(GemmCase(c.entry, "", c.rows, c.cin, c.cout, c.kvol, False, c.cap,
                                  opt=(("out_f32", True),) if c.o("out_f32") else ()), kind)


@lru_cache(maxsize=4)
def _gemm_data_of(c: GemmCase, kind: str):
    g = torch.Generator().manual_seed(_seed(c.entry, c.rows, c.cin, c.cout, c.kvol, c.cap, kind))
    rows = c.alloc_rows
    nbr = torch.randint(0, N_IN, (rows, c.kvol), generator=g, dtype=torch.int32)
    nbr[torch.rand((rows, c.kvol), generator=g) < 0.4] = -1
    nbr[3::5] = -1                         # rows without any neighbour: the epilogue of 0
    half = c.entry in ("f16", "gg16")
    if kind == "exact":
        xm, wm = exact_limits(c)
        ints = lambda m, shape: torch.randint(-m, m + 1, shape, generator=g).float()  # noqa: E731
        feats, weight = ints(xm, (N_IN, c.cin)), ints(wm, (c.kvol, c.cin, c.cout))
        bias, shift, res = ints(4, (c.cout,)), ints(4, (c.cout,)), ints(4, (rows, c.cout))
        scale = torch.tensor([-1.0, 1.0, 2.0])[torch.randint(0, 3, (c.cout,), generator=g)]
    else:
        rn = lambda shape: torch.randn(shape, generator=g)  # noqa: E731
        feats, weight = rn((N_IN, c.cin)), rn((c.kvol, c.cin, c.cout))
        if c.entry == "x3":  # values spread over several binades, as its own test has them
            feats, weight = feats * torch.exp(rn(feats.shape)), weight * torch.exp(rn(weight.shape))
        weight = weight / float(c.kvol * c.cin) ** 0.5
        bias, scale, shift, res = rn((c.cout,)), rn((c.cout,)), rn((c.cout,)), rn((rows, c.cout))
        if half:             # operands that are fp16 values already
            feats, weight, res = feats.half().float(), weight.half().float(), res.half().float()
    return dict(feats=feats, nbr=nbr, weight=weight, bias=bias, scale=scale, shift=shift, res=res)


def gemm_data(c: GemmCase, kind: str):
    """The case's operands on the CPU in fp32 (made once per case and shared: do not write to them), with the parts of the
    epilogue the case leaves out set to None."""
    d = dict(_gemm_data(c, kind))
    for name, keys in (("bias", ("bias",)), ("bn", ("scale", "shift")), ("res", ("res",))):
        if name not in c.epi:
            for k in keys:
                d[k] = None
    d["relu"] = "relu" in c.epi
    return d


def gather_reference(feats, nbr, weight, bias=None, scale=None, shift=None, res=None, relu=False):
    """The float64 gather-matmul: out[r] = sum_k feats[nbr[r, k]] @ weight[k] (a zero row where nbr is -1), then + bias,
    * scale + shift, + residual, ReLU -- the order of the kernels' epilogues.  Any device."""
    n_in, cin = feats.shape
    f64 = torch.cat([feats.double(), torch.zeros(1, cin, dtype=torch.float64, device=feats.device)])
    w64 = weight.double().reshape(-1, cin, weight.shape[-1])
    nb = nbr.long()
    nb = torch.where(nb < 0, torch.full_like(nb, n_in), nb)
    out = torch.zeros(nbr.shape[0], w64.shape[-1], dtype=torch.float64, device=feats.device)
    for k in range(w64.shape[0]):
        out += f64.index_select(0, nb[:, k]) @ w64[k]
    if bias is not None:
        out = out + bias.double()
    if scale is not None:
        out = out * scale.double() + shift.double()
    if res is not None:
        out = out + res.double()
    return out.clamp_min(0) if relu else out


def case_reference(c: GemmCase, d):
    """gather_reference of the case's `rows` real rows."""
    res = None if d["res"] is None else d["res"][: c.rows]
    return gather_reference(d["feats"], d["nbr"][: c.rows], d["weight"], d["bias"], d["scale"], d["shift"], res, d["relu"])


def assert_representable(c: GemmCase, d, want):
    """The precondition of bit equality on the exact class: every partial sum an integer below 2^24 (worst case over any
    summation order: the sum of the absolute products), every output below the output format's integer range."""
    xm, wm = float(d["feats"].abs().max()), float(d["weight"].abs().max())
    worst = c.kvol * c.cin * xm * wm + 4
    assert 2 * worst + 8 <= 2.0 ** 24, (c.id, worst)
    assert float(want.abs().max()) <= exact_bound(c), (c.id, float(want.abs().max()))
    assert bool((want == want.round()).all()), c.id


# ---- device calls (GPU tests only) -----------------------------------------------------------------------------------------------
def misaligned(t):
    """A contiguous copy of `t` whose data_ptr() % 16 == 4."""
    step = 4 // t.element_size()
    buf = torch.empty(t.numel() + step, dtype=t.dtype, device=t.device)
    view = buf[step:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def tile_order_dev(nbr, n_dev=None, kvol=None):
    """(status, order) of pd3_sparse_tile_order on a device table; n_dev: the device row count of the capacity form."""
    from paddle3d_amd.ops._common import lib, ptr, stream_ptr

    rows = int(nbr.shape[0])
    order = torch.full((int(lib().pd3_sparse_tile_order_entries(rows)),), -9, dtype=torch.int32, device=nbr.device)
    status = lib().pd3_sparse_tile_order(ptr(nbr), ptr(n_dev), rows, int(nbr.shape[1]) if kvol is None else kvol,
                                         ptr(order), stream_ptr(nbr.device))
    return status, order


def device_operands(c: GemmCase, d, dev="cuda"):
    """The operands as the entry reads them: fp16 rows / residual and packed weights for the 16-bit entries, the count and the
    tile order where the case asks for them, an operand moved to data_ptr() % 16 == 4 where it asks for that."""
    from paddle3d_amd.ops import sparse_conv3d as sp

    half = c.entry in ("f16", "gg16")
    t = {k: (v if v is None or isinstance(v, bool) else v.to(dev)) for k, v in d.items()}
    w = t["weight"]
    refused_shape = c.entry != "fp32" and c.path.startswith("refuse")
    if c.entry == "x3":
        t["wdev"] = torch.zeros(3 * w.numel(), dtype=torch.bfloat16, device=dev) if refused_shape else sp.pack_weight_bf16x3(w)
    elif half:
        t["wdev"] = torch.zeros(w.numel(), dtype=torch.float16, device=dev) if refused_shape else sp.pack_weight_f16(w)
    else:
        t["wdev"] = w.contiguous()
    t["fdev"] = t["feats"].half() if half else t["feats"]
    t["rdev"] = t["res"].half() if half and t["res"] is not None else t["res"]
    if c.o("misalign") == "feats":
        t["fdev"] = misaligned(t["fdev"])
    if c.o("misalign") == "weight":
        t["wdev"] = misaligned(t["wdev"])
    t["n_dev"] = torch.tensor([c.rows], dtype=torch.int32, device=dev) if c.cap else None
    t["order"] = None
    if c.order:
        status, t["order"] = tile_order_dev(t["nbr"], t["n_dev"])
        assert status == 0, (c.id, "pd3_sparse_tile_order", status)
    return t


def new_output(c: GemmCase, dev="cuda"):
    dtype = torch.float16 if c.out_f16 else torch.float32
    return torch.full((c.alloc_rows + TAIL, c.o("ld", c.cout)), SENTINEL, dtype=dtype, device=dev)


def call_gemm(c: GemmCase, t, out):
    """Run the case's C entry point on device_operands `t` into `out`; returns the status (no exception)."""
    from paddle3d_amd.ops._common import lib, ptr, stream_ptr

    L, s = lib(), stream_ptr(out.device)
    shift = None if c.o("half") else t["shift"]
    head = (ptr(t["fdev"]), ptr(t["nbr"]), ptr(t["n_dev"]), c.alloc_rows, c.kvol, c.cin, c.cout, ptr(t["wdev"]),
            ptr(t["bias"]), ptr(t["scale"]), ptr(shift), ptr(t["rdev"]), int(t["relu"] or 0), ptr(t["order"]), ptr(out))
    if c.entry == "fp32":
        return L.pd3_sparse_conv3d_features_ordered(*head, s)
    if c.entry == "x3":
        return L.pd3_sparse_conv3d_features_bf16x3(*head, s)
    if c.entry == "f16":
        return L.pd3_sparse_conv3d_features_f16(*head, int(bool(c.o("out_f32", False))), s)
    return L.pd3_gather_gemm_f16(*head, 0, int(c.o("ld", c.cout)), int(c.o("off", 0)), s)


# ---- index builders: the NumPy reference ---------------------------------------------------------------------------------
def _t3(v):
    return (v, v, v) if isinstance(v, int) else tuple(int(x) for x in v)


def out_shape(shape, ks, st, pd):
    return tuple((s + 2 * p - k) // t + 1 for s, k, t, p in zip(shape, ks, st, pd))


def valid_rows(coords, batch, shape):
    c = np.asarray(coords, np.int64).reshape(-1, 4)
    ok = (c[:, 0] >= 0) & (c[:, 0] < batch)
    for a in range(3):
        ok &= (c[:, a + 1] >= 0) & (c[:, a + 1] < shape[a])
    return ok


def ref_indices(coords, batch, shape, ks, st=1, pd=0, subm=False):
    """One sparse convolution's index set from the definition: (out_coords [n_out, 4], nbr [n_out, K], output shape).
    Regular: every q inside the output shape with p = q * stride - pad + k for some input p and offset k, in raster
    (b, z, y, x) order.  Submanifold: the input rows themselves, in input order (a padding or out-of-range row stays a row
    and has no neighbour).  nbr[q][k] = the row of p, the highest one where a coordinate occurs more than once, or -1."""
    ks, st, pd = _t3(ks), _t3(st), _t3(pd)
    c = np.asarray(coords, np.int64).reshape(-1, 4)
    ok = valid_rows(c, batch, shape)
    row_of = {}
    for i in np.nonzero(ok)[0]:
        row_of[tuple(c[i])] = int(i)          # ascending: the highest row wins
    offsets = list(itertools.product(range(ks[0]), range(ks[1]), range(ks[2])))
    if subm:
        pd = tuple(k // 2 for k in ks)
        oshape, out, live = tuple(shape), [tuple(r) for r in c], ok
    else:
        oshape = out_shape(shape, ks, st, pd)
        reach = set()
        for (b, z, y, x) in row_of:
            for k in offsets:
                n = (z + pd[0] - k[0], y + pd[1] - k[1], x + pd[2] - k[2])
                if all(v >= 0 and v % s == 0 and v // s < o for v, s, o in zip(n, st, oshape)):
                    reach.add((b, n[0] // st[0], n[1] // st[1], n[2] // st[2]))
        out = sorted(reach)
        live = np.ones(len(out), bool)
    nbr = np.full((len(out), len(offsets)), -1, np.int32)
    for r, (b, z, y, x) in enumerate(out):
        if not live[r]:
            continue
        for j, k in enumerate(offsets):
            p = (z * st[0] - pd[0] + k[0], y * st[1] - pd[1] + k[1], x * st[2] - pd[2] + k[2])
            if all(0 <= v < s for v, s in zip(p, shape)):
                nbr[r, j] = row_of.get((b,) + p, -1)
    oc = c.astype(np.int32) if subm else np.asarray(out, np.int32).reshape(-1, 4)
    return oc, nbr, oshape


def ref_chain(coords, batch, shape, chain):
    """indices() applied conv by conv: [(out_coords, nbr, out_shape)] per convolution."""
    cur, cur_shape, out = np.asarray(coords, np.int32), tuple(shape), []
    for ks, st, pd, subm in chain:
        oc, nbr, osh = ref_indices(cur, batch, cur_shape, ks, st, pd, subm)
        out.append((oc, nbr, osh))
        cur, cur_shape = oc, osh
    return out


def ref_plan(coords, batch, shape, chain):
    """plan(): (order, coords of the first set, [(out_coords, nbr, out_shape)] per convolution).  The first set is the real
    rows in raster order, rows of one coordinate in input order; every later set is in raster order."""
    c = np.asarray(coords, np.int64).reshape(-1, 4)
    rows = np.nonzero(valid_rows(c, batch, shape))[0]
    order = np.asarray(sorted(rows, key=lambda i: (tuple(c[i]), i)), np.int64)
    first = c[order].astype(np.int32).reshape(-1, 4)
    return order, first, ref_chain(first, batch, shape, chain)


# ---- index-builder cases ---------------------------------------------------------------------------------------------------
SUBM333 = ((3, 3, 3), (1, 1, 1), (1, 1, 1), True)
DOWN333 = ((3, 3, 3), (2, 2, 2), (1, 1, 1), False)
GEOMETRIES = [
    ("subm333", SUBM333),
    ("subm113", ((1, 1, 3), (1, 1, 1), (0, 0, 1), True)),
    ("subm133", ((1, 3, 3), (1, 1, 1), (0, 1, 1), True)),
    ("k333s2p1", DOWN333),
    ("k333s2p011", ((3, 3, 3), (2, 2, 2), (0, 1, 1), False)),
    ("k311s211p0", ((3, 1, 1), (2, 1, 1), (0, 0, 0), False)),
    ("k111s1p0", ((1, 1, 1), (1, 1, 1), (0, 0, 0), False)),
    ("k111s2p0", ((1, 1, 1), (2, 2, 2), (0, 0, 0), False)),       # inputs on odd cells reach nothing
    ("k222s2p0", ((2, 2, 2), (2, 2, 2), (0, 0, 0), False)),
    ("k222s2p101", ((2, 2, 2), (2, 2, 2), (1, 0, 1), False)),
    ("k222s3p0", ((2, 2, 2), (3, 3, 3), (0, 0, 0), False)),       # stride > kernel
    ("k333s3p0", ((3, 3, 3), (3, 3, 3), (0, 0, 0), False)),
    ("k333s1p2", ((3, 3, 3), (1, 1, 1), (2, 2, 2), False)),       # padding > kernel // 2: the output is the larger grid
]
N_IN_BORDERS = (511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097)   # hash table size, radix tile, scan tile
MAP_TILE = 16384
OUT_GRID_CELLS = tuple(MAP_TILE * m + d for m in (1, 2) for d in (-1, 0, 1, 7))
LARGE = dict(batch=3, shape=(8, 8192, 16384))


@dataclass(frozen=True)
class IndexCase:
    name: str
    axis: str            # geometry / occupancy / n_in / out_grid / large
    batch: int
    shape: tuple
    occ: str             # occupancy generator (index_coords)
    chain: tuple         # ((kernel, stride, padding, subm), ...)
    n: int = 0           # voxels asked for, where the generator takes a count

    @property
    def id(self):
        return f"{self.axis}-{self.name}"

    @property
    def small(self):     # a dense oracle fits
        return self.batch * int(np.prod(self.shape)) <= 40000


def index_cases():
    out, base = [], (2, (5, 6, 7))
    for name, geo in GEOMETRIES:
        out.append(IndexCase(f"{name}-corners", "geometry", *base, "corners", (geo,)))
        out.append(IndexCase(f"{name}-random", "geometry", *base, "random", (geo,), 130))
    chain = (SUBM333, DOWN333)
    for occ in ("corners", "one", "full", "line", "dups", "invalid", "allpad"):
        out.append(IndexCase(occ, "occupancy", *base, occ, chain))
    out.append(IndexCase("full-k222s2p0", "occupancy", *base, "full", (GEOMETRIES[8][1],)))
    out.append(IndexCase("full-k333s1p2", "occupancy", *base, "full", (GEOMETRIES[12][1],)))
    for name, shape in (("W1", (5, 6, 1)), ("H1", (5, 1, 7)), ("D1", (1, 6, 7)), ("W1H1", (5, 1, 1))):
        out.append(IndexCase(name, "occupancy", 2, shape, "random", chain, max(2, int(np.prod(shape)) * 2 * 2 // 5)))
    for n in N_IN_BORDERS:
        out.append(IndexCase(f"n{n}", "n_in", 1, (5, 30, 33), "random", chain, n))
    for cells in OUT_GRID_CELLS:   # a regular convolution whose OUTPUT grid has this many cells, kernel 3 / pad 1 on size-1 axes
        out.append(IndexCase(f"cells{cells}", "out_grid", 1, (1, 1, cells), "ends", (((3, 3, 3), (1, 1, 1), (1, 1, 1), False),),
                             300))
    out.append(IndexCase("keys-above-2^31", "large", LARGE["batch"], LARGE["shape"], "clusters", chain, 3000))
    return out


@lru_cache(maxsize=None)
def _index_coords(c: IndexCase):
    rng = np.random.default_rng(_seed(c.name, c.axis))
    b, (d, h, w) = c.batch, c.shape
    cells = b * d * h * w

    def cells_to_coords(lin):
        lin = np.asarray(lin, np.int64)
        bb, r = np.divmod(lin, d * h * w)
        z, r = np.divmod(r, h * w)
        y, x = np.divmod(r, w)
        return np.stack([bb, z, y, x], 1)

    def pick(n, exclude=()):
        pool = np.setdiff1d(np.arange(cells), np.asarray(exclude, np.int64))
        return cells_to_coords(rng.choice(pool, min(n, len(pool)), replace=False))

    if c.occ == "random":
        co = pick(c.n)
    elif c.occ == "full":
        co = cells_to_coords(rng.permutation(cells))
    elif c.occ == "one":
        co = np.array([[b - 1, d // 2, h // 2, w // 2]])
    elif c.occ == "corners":   # the eight corners and the twelve edge midpoints of every batch item, a few cells inside
        pts = {(z, y, x) for z in (0, d // 2, d - 1) for y in (0, h // 2, h - 1) for x in (0, w // 2, w - 1)
               if sum(v in (0, m - 1) for v, m in ((z, d), (y, h), (x, w))) >= 2}
        co = np.array([(bb,) + p for bb in range(b) for p in sorted(pts)])
        extra = pick(30)
        co = np.unique(np.concatenate([co, extra]), axis=0)
        co = co[rng.permutation(len(co))]
    elif c.occ == "line":      # a full (b, z, y) line, the lines above and below it empty
        co = pick(100)
        co = co[~((co[:, 0] == 0) & (co[:, 1] == 1) & (np.abs(co[:, 2] - 2) <= 1))]
        line = np.array([(0, 1, 2, x) for x in range(w)])
        co = np.concatenate([co, line])
        co = co[rng.permutation(len(co))]
    elif c.occ == "dups":      # ten coordinates at four rows each
        co = pick(110)
        co = np.concatenate([co, co[:10], co[:10], co[:10]])
        co = co[rng.permutation(len(co))]
    elif c.occ in ("invalid", "allpad"):
        co = pick(110)
        bad = co[:40].copy()
        bad[0:10, 0] = b          # b >= batch
        bad[10:20, 1] = -1        # negative z
        bad[20:30, 3] = w         # x == W
        bad[30:40, 0] = -1        # the voxelizer's padding rows
        co = np.concatenate([co[40:], bad]) if c.occ == "invalid" else bad
        co = co[rng.permutation(len(co))]
    elif c.occ == "ends":      # the first and the last cell and c.n more
        co = np.concatenate([pick(c.n, exclude=(0, cells - 1)), cells_to_coords([0, cells - 1])])
        co = co[rng.permutation(len(co))]
    elif c.occ == "clusters":  # neighbourhoods (so that rulebooks are not empty) spread over the whole key range
        m = c.n // 10          # half of the centres anywhere, half at keys >= 2^31
        centres = cells_to_coords(np.concatenate([rng.integers(0, cells, m // 2), rng.integers(1 << 31, cells, m - m // 2)]))
        steps = np.concatenate([np.zeros((m, 10, 1), np.int64), rng.integers(-1, 2, (m, 10, 3))], 2)
        co = (centres[:, None, :] + steps).reshape(-1, 4)
        co = co[valid_rows(co, b, c.shape)]
        ends = np.array([[0, 0, 0, 0], [0, 0, 0, 1], [b - 1, d - 1, h - 1, w - 1], [b - 1, d - 1, h - 1, w - 2]])
        co = np.unique(np.concatenate([co, ends]), axis=0)
        co = co[rng.permutation(len(co))]
    else:
        raise KeyError(c.occ)
    co = np.ascontiguousarray(co.astype(np.int32))
    co.setflags(write=False)
    return co


def index_coords(c: IndexCase):
    """The case's input rows [n, 4] int32 (b, z, y, x), read-only: as `indices` gets them."""
    return _index_coords(c)


@lru_cache(maxsize=None)
def plan_input(c: IndexCase):
    """The same rows shuffled, with a batch = -1 row after every third one: as `plan` gets them."""
    co = index_coords(c)
    rng = np.random.default_rng(_seed(c.name, "plan"))
    co = co[rng.permutation(len(co))]
    n_pad = len(co) // 3 + 1
    mixed = np.concatenate([co, np.full((n_pad, 4), -1, np.int32)])
    slots = np.concatenate([np.arange(len(co)) * 3, np.arange(n_pad) * 9 + 1])   # padding rows land between real ones
    mixed = np.ascontiguousarray(mixed[np.argsort(slots, kind="stable")])
    mixed.setflags(write=False)
    return mixed


@lru_cache(maxsize=None)
def chain_reference(c: IndexCase):
    return ref_chain(index_coords(c), c.batch, c.shape, c.chain)


@lru_cache(maxsize=None)
def plan_reference(c: IndexCase):
    return ref_plan(plan_input(c), c.batch, c.shape, c.chain)


def keys_of(coords, shape):
    """Linear cell index of coordinate rows, in Python integers' range (int64)."""
    c = np.asarray(coords, np.int64).reshape(-1, 4)
    d, h, w = shape
    return ((c[:, 0] * d + c[:, 1]) * h + c[:, 2]) * w + c[:, 3]


# grids no builder takes: (name, batch, shape): 2^32 cells (a 32-bit product wraps to 0) and one cell fewer
GRID_REFUSALS = [("2^32", 4, (16, 8192, 8192)), ("2^32-w", 1, (1, 65536, 65536)), ("2^32-1", 3, (85, 257, 65537))]

# capacity mode: a two-set chain (the input set and two regular sets), each regular set's capacity at count + delta
CAP_CHAIN = (SUBM333, DOWN333, SUBM333, ((3, 3, 3), (2, 2, 2), (0, 1, 1), False))
CAP_GRID = dict(batch=2, shape=(17, 40, 48), n=300)   # sparse enough that no set is capped by its grid's cell count
CAP_CASES = [(j, delta) for j in (1, 2) for delta in (-1, 0, 1)]

TO_DENSE_CASES = [(ch, counted) for ch in (1, 5, 128) for counted in (False, True)]
