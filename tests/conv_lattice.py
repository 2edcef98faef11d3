"""The dense convolution kernels' shape lattice (a helper module like tests/guarded.py, not a conftest).

One record per kernel family -- wrapper, packer, predicate, C entry point, tile geometry -- and from every record the
cases that sit on the border of what its predicate accepts.  The cases are a CROSS, not a product: a spatial sweep at
the smallest channel counts, a channel sweep on one small map, an epilogue sweep on the smallest case:

* height        1, 2, 3, T-1, T, T+1, 2T+1 output rows for the family's tile height T
* valid width   one quad, C-4, C-2, C, C+4, 2C+4 output columns for its tile width C (C-2 where rows may live at pitch4)
* pixel tiles   one tile per image and 1, 7, 8, 9, 17 images (every launcher rounds tiles up to a multiple of 8)
* channels      the predicate's smallest cin / cout, three times the smallest, and the family's own thresholds
* epilogue      bias present / None, ReLU on / off, and for the patch modes a channel offset into a wider output

Refusals: for every clause of a predicate the nearest shape that breaks only that clause.

Data classes (make_data): "exact" = small integers whose every partial sum is representable (so the result does not
depend on the order of summation: a kernel must equal the float64 reference bit for bit), "random" = the
distributions of tests/test_conv_gpu.py, compared under the bars that file already holds (BARS below).

Everything here runs on the CPU; the device calls live in `Family.call`, which the GPU tests use.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

from paddle3d_amd.ops import conv

SENTINEL = -7.0          # what an output tensor holds where a kernel must not write
PTILE_COUNTS = (1, 7, 8, 9, 17)


# ---- cases ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    family: str
    axis: str            # height / width / ptiles / channels / epilogue / refuse:<clause>
    n: int
    cin: int             # per group for the grouped families
    cout: int            # per group for the grouped families
    h: int               # INPUT map
    wv: int              # INPUT valid width
    bias: bool = True
    relu: bool = True
    opt: tuple = ()      # sorted (key, value) pairs: groups, off, ctot, pitch, stride, ...

    def o(self, key, default=None):
        return dict(self.opt).get(key, default)

    @property
    def id(self):
        extra = "".join(f"-{k}{v}" for k, v in self.opt)
        return (f"{self.family}-{self.axis}-n{self.n}-ci{self.cin}-co{self.cout}-{self.h}x{self.wv}"
                f"{'' if self.bias else '-nobias'}{'' if self.relu else '-norelu'}{extra}")


def _case(fam, axis, n, cin, cout, h, wv, bias=True, relu=True, **opt):
    return Case(fam, axis, n, cin, cout, h, wv, bias, relu, tuple(sorted(opt.items())))


@dataclass
class Family:
    """One kernel family.  tile = (output rows, output columns, output channels per workgroup, K channels per trip),
    read from the constexpr block cited in `src`."""
    name: str
    wrapper: str
    packer: str
    predicate: str
    symbol: str
    tile: tuple
    src: str
    kind: str            # nchw3 / patch / grouped / f16 / f16s2 / groupedf16 / scatter
    exact: str = "bits"  # bits: equal to the float64 reference bit for bit; wino43: the restatement bar
    bar: str = "fp32"    # key of BARS for the random class
    cin0: int = 8        # the predicate's smallest channel counts
    cout0: int = 64
    stride: int = 1
    pitch_ok: bool = True   # valid widths that are not a multiple of 4 (stored at pitch4)
    out_f16: bool = False
    opts: dict = field(default_factory=dict)
    extra_channels: tuple = ()  # (cin, cout) pairs next to the family's own thresholds

    # -- predicate ----------------------------------------------------------------------------------------------------
    def accepts(self, c: Case) -> bool:
        k, pitch = self.kind, c.o("pitch", conv.pitch4(c.wv))
        if c.o("stride", self.stride) not in (1, 2):
            return False
        if k == "nchw3":
            if pitch % 4:  # every fp32 NCHW kernel reads aligned float4: the dispatchers never hand over such rows
                return False
            if self.predicate == "supported":
                return conv.supported(c.cin, c.cout, c.h, c.wv, c.o("stride", self.stride))
            if self.predicate == "conv3x3_s2_x3_supported":
                return conv.conv3x3_s2_x3_supported(c.cin, c.cout, c.h, c.wv, c.n)
            if self.predicate == "winograd43_supported":
                return conv.winograd43_supported(c.cin, c.cout, c.h, c.wv) and c.cout % self.opts["tile"] == 0
            w = c.wv if self.predicate == "winograd_supported" else pitch
            return getattr(conv, self.predicate)(c.cin, c.cout, c.h, w)
        if k == "patch":
            mode = self.opts["mode"]
            if mode < 2 and c.wv != pitch:
                return False
            if self.predicate == "patch_x3_supported":
                return conv.patch_x3_supported(mode, c.cin, c.cout, c.h, pitch, c.n, c.o("ctot", c.cout))
            return conv.patch_supported(mode, c.cin, c.cout, c.h, pitch)
        if k == "grouped":
            return conv.grouped_small_supported(c.cin, c.cout, c.h, c.wv)
        if k == "groupedf16":  # (no predicate of its own: CenterHead.forward asks for hc == 64 and 1..4 outputs)
            return c.cin == 64 and 1 <= c.cout <= 4
        if k == "f16":
            return conv.f16_supported(c.cin, c.cout, c.h, c.wv) and c.cout % self.opts["tile"] == 0
        if k == "f16s2":
            return conv.s2_f16_supported(c.cin, c.cout)
        if self.predicate == "scatter_conv_supported":
            return conv.scatter_conv_supported(c.cin, c.cout, c.h, c.wv, c.o("stride", 2))
        if self.predicate == "scatter_conv_s2_f16_supported":
            return conv.scatter_conv_s2_f16_supported(c.cin, c.cout, c.h, c.wv) and c.cout % self.opts["tile"] == 0
        return conv.scatter_conv_sparse_supported(c.cin, c.cout, c.h, c.wv, c.o("stride", 2))

    # -- geometry -----------------------------------------------------------------------------------------------------
    def out_hw(self, c: Case):
        """(rows, valid columns) of the output map."""
        if self.kind == "patch":
            s = {0: 0.5, 1: 1, 2: 2, 3: 4}[self.opts["mode"]]
            return int(c.h * s), int(c.wv * s)
        if self.kind in ("f16s2",) or self.predicate == "scatter_conv_sparse_supported":
            return (c.h - 1) // 2 + 1, (c.wv - 1) // 2 + 1
        s = c.o("stride", self.stride)
        return c.h // s, c.wv // s

    def groups(self, c: Case) -> int:
        return c.o("groups", 1)

    def weight_shape(self, c: Case):
        g = self.groups(c)
        if self.kind == "patch":
            k = {0: 2, 1: 1, 2: 2, 3: 4}[self.opts["mode"]]
            return (c.cin, c.cout, k, k) if self.opts["mode"] >= 2 else (c.cout, c.cin, k, k)
        return (g * c.cout, c.cin, 3, 3)

    def fan_in(self, c: Case) -> int:
        if self.kind == "patch":
            return c.cin * {0: 4, 1: 1, 2: 1, 3: 1}[self.opts["mode"]]
        return c.cin * 9

    # -- the float64 reference, on the logical (unpadded NCHW) tensors ----------------------------------------------------
    def reference(self, c: Case, x, w, b):
        x, w = x.double(), w.double()
        b = None if b is None else b.double()
        if self.kind == "patch":
            mode = self.opts["mode"]
            if mode == 0:
                y = F.conv2d(x, w, b, stride=2)
            elif mode == 1:
                y = F.conv2d(x, w, b)
            else:
                y = F.conv_transpose2d(x, w, b, stride=2 if mode == 2 else 4)
        else:
            y = F.conv2d(x, w, b, stride=c.o("stride", self.stride), padding=1, groups=self.groups(c))
        return torch.relu(y) if c.relu else y

    # -- layouts: logical tensors <-> what the kernel reads and writes -------------------------------------------------------
    def lay_in(self, c: Case, x):
        """Logical input [n, groups * cin, h, wv] -> the kernel's input tensor (CPU)."""
        if self.kind in ("f16", "f16s2", "groupedf16"):
            xh = x.half().permute(0, 2, 3, 1).contiguous()  # NHWC
            if self.opts.get("group_major_in"):
                n, h, w, ch = xh.shape
                xh = xh.view(n, h, w, ch // 64, 64).permute(0, 3, 1, 2, 4).contiguous()
            return xh
        if self.kind == "scatter":
            raise RuntimeError("scatter families build their canvas in make_data")
        pitch = c.o("pitch", conv.pitch4(c.wv))
        return F.pad(x, (0, pitch - c.wv)).contiguous() if pitch > c.wv else x.contiguous()

    def out_shape(self, c: Case):
        ho, wo = self.out_hw(c)
        g = self.groups(c)
        if self.kind == "patch":
            return (c.n, c.o("ctot", c.cout), ho, wo if self.opts["mode"] >= 2 else conv.pitch4(wo))
        if self.kind in ("f16", "f16s2") or self.predicate == "scatter_conv_s2_f16_supported":
            mode = self.opts.get("out", "nhwc")
            if mode == "f32":
                return (c.n, c.cout, ho, wo)
            if mode == "gm":
                return (c.n, c.cout // 64, ho, wo, 64)
            return (c.n, ho, wo, c.cout)
        if self.kind in ("grouped", "groupedf16"):
            return (c.n, c.o("out_groups", g) * c.cout, ho, wo)
        if self.predicate == "scatter_conv_sparse_supported":
            return (c.n, c.cout, ho, wo)
        return (c.n, c.cout, ho, conv.pitch4(wo))

    def out_dtype(self):
        return torch.float16 if self.out_f16 else torch.float32

    def expected(self, c: Case, ref):
        """The float64 reference [n, channels, ho, wo] laid out as the kernel's output: float64, zeros in the padding
        columns, SENTINEL where the kernel must not write."""
        shape = self.out_shape(c)
        mode = self.opts.get("out", "nhwc")
        if self.kind in ("f16", "f16s2") or self.predicate == "scatter_conv_s2_f16_supported":
            if mode == "f32":
                return ref.clone()
            if mode == "gm":
                n, ch, ho, wo = ref.shape
                return ref.view(n, ch // 64, 64, ho, wo).permute(0, 1, 3, 4, 2).contiguous()
            return ref.permute(0, 2, 3, 1).contiguous()
        out = torch.full(shape, SENTINEL, dtype=torch.float64)
        c0, ch = 0, ref.shape[1]
        if self.kind == "patch":
            c0 = c.o("off", 0)
        elif self.kind in ("grouped", "groupedf16"):
            c0 = c.o("out_group0", 0) * c.cout
        out[:, c0:c0 + ch] = 0.0
        out[:, c0:c0 + ch, :, : ref.shape[3]] = ref
        return out

    def expected_all(self, c: Case, ref):
        """[(expected output as float64, its dtype on the device)] -- two entries for the dual-output entry point."""
        if self.opts.get("out") == "dual":
            return [(ref.permute(0, 2, 3, 1).contiguous(), torch.float16), (ref.clone(), torch.float32)]
        return [(self.expected(c, ref), self.out_dtype())]

    # -- weights ------------------------------------------------------------------------------------------------------
    def pack(self, c: Case, w):
        p, g = self.packer, self.groups(c)
        if p in ("pack_grouped_weight", "pack_grouped_weight_f16"):
            return getattr(conv, p)(w, g)
        if p in ("pack_patch_weight", "pack_patch_weight_x3"):
            return getattr(conv, p)(w, self.opts["mode"], self.opts["mode"] >= 2)
        if p in ("pack_winograd43_weight", "pack_conv3x3_f16_weight"):
            return getattr(conv, p)(w, self.opts["tile"])
        if p == "sparse":
            return w
        return getattr(conv, p)(w)

    # -- the device call (GPU tests only) -----------------------------------------------------------------------------------
    def call(self, c: Case, xin, packed, bias, out=None):
        """Run the wrapper on device tensors.  `out` (pre-filled by the caller) where the wrapper takes one.  Returns the
        list of output tensors (two for the dual-output entry)."""
        k, wv = self.kind, (c.wv if c.wv != xin.shape[-1] or c.o("pitch") else None)
        if k == "nchw3":
            cout, wr = c.cout, self.wrapper
            if wr == "conv3x3_bias_relu":
                return [conv.conv3x3_bias_relu(xin, packed, bias, cout, c.relu, stride=c.o("stride", self.stride), out=out,
                                               w_valid=c.wv)]
            if wr == "conv3x3_winograd_bias_relu":
                return [conv.conv3x3_winograd_bias_relu(xin, packed, bias, cout, c.relu, out=out)]
            if wr == "conv3x3_s2_x3_bias_relu":
                return [conv.conv3x3_s2_x3_bias_relu(xin, packed, bias, cout, c.relu, w_valid=c.wv)]
            if wr == "conv3x3_winograd43_ppv_bias_relu":
                v = conv.winograd43_input_transform(xin, w_valid=c.wv)
                return [conv.conv3x3_winograd43_ppv_bias_relu(v, xin.shape, packed, bias, cout, c.relu, out=out, w_valid=c.wv)]
            return [getattr(conv, wr)(xin, packed, bias, cout, c.relu, out=out, w_valid=c.wv)]
        if k == "patch":
            return [getattr(conv, self.wrapper)(xin, packed, bias, self.opts["mode"], c.cout, out, c.o("off", 0), relu=c.relu,
                                                w_valid=c.wv)]
        if k == "grouped":
            return [conv.grouped_conv3x3_small(xin, packed, bias, self.groups(c), out=out, out_groups=c.o("out_groups"),
                                               out_group0=c.o("out_group0", 0))]
        if k == "groupedf16":
            return [conv.grouped_conv3x3_small_f16(xin, packed, bias, self.groups(c), out=out, out_groups=c.o("out_groups"),
                                                   out_group0=c.o("out_group0", 0),
                                                   group_major=bool(self.opts.get("group_major_in")))]
        if k == "f16":
            mode = self.opts.get("out", "nhwc")
            if mode == "dual":
                return list(conv.conv3x3_f16_bias_relu_dual(xin, packed, bias, c.cout, c.relu))
            return [conv.conv3x3_f16_bias_relu(xin, packed, bias, c.cout, c.relu, out_f32_nchw=mode == "f32", out=out,
                                               group_major=mode == "gm")]
        if k == "f16s2":
            return [conv.conv3x3_s2_f16_bias_relu(xin, packed, bias, c.cout, c.relu)]
        # scatter: xin is a SparseCanvas
        if self.wrapper == "scatter_conv3x3_bias_relu":
            return [conv.scatter_conv3x3_bias_relu(xin, packed, bias, c.cout, c.relu)]
        if self.wrapper == "scatter_conv3x3_s2_f16_bias_relu":
            return [conv.scatter_conv3x3_s2_f16_bias_relu(xin, packed, bias, c.cout, c.relu)]
        return [conv.scatter_conv3x3_sparse(xin, packed, bias, None, c.relu)[0]]

    def takes_out(self) -> bool:
        return (self.kind in ("patch", "grouped", "groupedf16")
                or (self.kind == "nchw3" and self.wrapper not in ("conv3x3_s2_x3_bias_relu",))
                or (self.kind == "f16" and self.opts.get("out", "nhwc") != "dual"))

    def needs_bias(self) -> bool:
        return self.predicate == "scatter_conv_sparse_supported"  # (the sparse form fills empty pixels with relu(bias))


# ---- the families ----------------------------------------------------------------------------------------------------------
# tile = (output rows, output columns, output channels per workgroup, input channels per trip)
FAMILIES = {f.name: f for f in [
    # conv3x3.hip:31-33 kCvCo = 64, kCvCi = 8; :383-393 the launcher's tiles: 2x128 / 4x64 / 1x128 / 2x64, else 4x32 (any map)
    Family("direct_s1", "conv3x3_bias_relu", "pack_conv3x3_weight", "supported", "pd3_conv3x3_bias_relu", (4, 32, 64, 8),
           "conv3x3.hip:31-33,385-389", "nchw3"),
    Family("direct_s2", "conv3x3_bias_relu", "pack_conv3x3_weight", "supported", "pd3_conv3x3_bias_relu", (4, 32, 64, 8),
           "conv3x3.hip:31-33,391-395", "nchw3", stride=2),
    # conv_winograd.hip:34-36 kWgCi = 8, kWgCo = 32, kWgTR x kWgTC = 4 x 16 tiles of 2 x 2 outputs
    Family("wino23", "conv3x3_winograd_bias_relu", "pack_winograd_weight", "winograd_supported",
           "pd3_conv3x3_winograd_bias_relu", (8, 32, 32, 8), "conv_winograd.hip:34-36", "nchw3", cout0=32, pitch_ok=False),
    # conv_winograd43.hpp:16-17 kW4Ci = 4, kW4TR x kW4TC = 2 x 16 tiles of 4 x 4 outputs; channels per workgroup 32 / 64
    Family("wino43_t32", "conv3x3_winograd43_bias_relu", "pack_winograd43_weight", "winograd43_supported",
           "pd3_conv3x3_winograd43_bias_relu", (8, 64, 32, 4), "conv_winograd43.hpp:16-17", "nchw3", exact="wino43",
           cin0=4, cout0=32, opts=dict(tile=32), extra_channels=((60, 32), (64, 32))),
    Family("wino43_t64", "conv3x3_winograd43_bias_relu", "pack_winograd43_weight", "winograd43_supported",
           "pd3_conv3x3_winograd43_bias_relu", (8, 64, 64, 4), "conv_winograd43.hpp:16-17", "nchw3", exact="wino43",
           cin0=4, cout0=64, opts=dict(tile=64), extra_channels=((60, 64), (64, 64), (64, 448), (64, 512))),
    # conv_winograd43_pp.hpp:8-9 kPpCi = 8 (two trips of kW4Ci), 64 channels per workgroup, the packed form's pixel tile
    Family("wino43_pp", "conv3x3_winograd43_pp_bias_relu", "pack_winograd43_lane_weight", "winograd43_pp_supported",
           "pd3_conv3x3_winograd43_pp_bias_relu", (8, 64, 64, 8), "conv_winograd43_pp.hpp:8-9", "nchw3", exact="wino43",
           extra_channels=((56, 64), (64, 64), (64, 448), (64, 512), (64, 1152), (64, 1216))),
    # conv_winograd43_pp.hpp:8-9 kPpCi = 8; conv_winograd43_ppv.hip:22 kPvMaxBlocks = 18 channel blocks per workgroup walk
    Family("wino43_ppv", "conv3x3_winograd43_ppv_bias_relu", "pack_winograd43_lane_weight", "winograd43_pp_supported",
           "pd3_conv3x3_winograd43_ppv_bias_relu", (8, 64, 64, 8), "conv_winograd43_pp.hpp:8-9,conv_winograd43_ppv.hip:22",
           "nchw3", exact="wino43",
           extra_channels=((56, 64), (64, 64), (64, 448), (64, 512), (64, 1152), (64, 1216))),
    # conv_s2_x3.hip:26-27 kS2M = 128, kS2K = 48 (3 kx x 16 channels); :269-270 tiles of 8 x 32 output pixels
    Family("s2_x3", "conv3x3_s2_x3_bias_relu", "pack_conv3x3_s2_x3_weight", "conv3x3_s2_x3_supported",
           "pd3_conv3x3_s2_x3_bias_relu", (8, 32, 128, 16), "conv_s2_x3.hip:26-27,269-270", "nchw3", bar="x3", cin0=16,
           cout0=128, stride=2, extra_channels=((16, 1024),)),
    # conv_patch.hip:29-31 kPgM = 64 rows, kPgP = 256 pixels, kPgK = 16; mode 0 tiles are 2 x 128 outputs (:260), the other
    # modes 256 consecutive pixels of the plane (:265): stated here as 4 x 64
    Family("patch0", "patch_conv_bias_relu", "pack_patch_weight", "patch_supported", "pd3_patch_conv_bias_relu",
           (2, 128, 64, 4), "conv_patch.hip:29-31,260", "patch", cin0=4, pitch_ok=False, opts=dict(mode=0)),
    Family("patch1", "patch_conv_bias_relu", "pack_patch_weight", "patch_supported", "pd3_patch_conv_bias_relu",
           (4, 64, 64, 16), "conv_patch.hip:29-31,265", "patch", cin0=16, cout0=1, pitch_ok=False, opts=dict(mode=1),
           extra_channels=((16, 32), (16, 33), (16, 64), (16, 65))),
    Family("patch2", "patch_conv_bias_relu", "pack_patch_weight", "patch_supported", "pd3_patch_conv_bias_relu",
           (4, 64, 16, 16), "conv_patch.hip:29-31,265", "patch", cin0=16, cout0=16, opts=dict(mode=2)),
    Family("patch3", "patch_conv_bias_relu", "pack_patch_weight", "patch_supported", "pd3_patch_conv_bias_relu",
           (4, 64, 4, 16), "conv_patch.hip:29-31,265", "patch", cin0=16, cout0=4, opts=dict(mode=3)),
    # conv_patch_x3.hip:34-36 kPxPix = 256, kPxM = 128, kPxKC = 32; mode 0: a wave's 32 pixels share an output row (:354)
    Family("patch0_x3", "patch_conv_x3_bias_relu", "pack_patch_weight_x3", "patch_x3_supported",
           "pd3_patch_conv_x3_bias_relu", (8, 32, 128, 16), "conv_patch_x3.hip:34-36,353", "patch", bar="x3", cin0=16,
           cout0=128, pitch_ok=False, opts=dict(mode=0), extra_channels=((16, 1024),)),
    Family("patch1_x3", "patch_conv_x3_bias_relu", "pack_patch_weight_x3", "patch_x3_supported",
           "pd3_patch_conv_x3_bias_relu", (4, 64, 128, 32), "conv_patch_x3.hip:34-36", "patch", bar="x3", cin0=32,
           cout0=128, pitch_ok=False, opts=dict(mode=1), extra_channels=((32, 1024),)),
    Family("patch2_x3", "patch_conv_x3_bias_relu", "pack_patch_weight_x3", "patch_x3_supported",
           "pd3_patch_conv_x3_bias_relu", (4, 64, 64, 32), "conv_patch_x3.hip:34-36", "patch", bar="x3", cin0=32,
           cout0=64, opts=dict(mode=2), extra_channels=((32, 1024),)),
    # conv3x3.hip:267-268 kGcCi = 4, kGcR x kGcW = 8 x 128 pixels, one group per workgroup
    Family("grouped", "grouped_conv3x3_small", "pack_grouped_weight", "grouped_small_supported",
           "pd3_grouped_conv3x3_small_slice", (8, 128, 4, 4), "conv3x3.hip:267-268", "grouped", cin0=4, cout0=1,
           pitch_ok=False),
    # conv_f16.hip:35-44 kCfCols = 32, kCfKc = 16, CfShape: M = 64 MB channels, R = 16 rows
    Family("f16_t64", "conv3x3_f16_bias_relu", "pack_conv3x3_f16_weight", "f16_supported", "pd3_conv3x3_f16_bias_relu",
           (16, 32, 64, 16), "conv_f16.hip:35-44", "f16", bar="f16", cin0=16, cout0=64, out_f16=True, opts=dict(tile=64)),
    Family("f16_t128", "conv3x3_f16_bias_relu", "pack_conv3x3_f16_weight", "f16_supported", "pd3_conv3x3_f16_bias_relu",
           (16, 32, 128, 16), "conv_f16.hip:35-44", "f16", bar="f16", cin0=16, cout0=128, out_f16=True, opts=dict(tile=128)),
    Family("f16_t64_f32out", "conv3x3_f16_bias_relu", "pack_conv3x3_f16_weight", "f16_supported",
           "pd3_conv3x3_f16_bias_relu", (16, 32, 64, 16), "conv_f16.hip:35-44", "f16", bar="f16", cin0=16, cout0=64,
           opts=dict(tile=64, out="f32")),
    Family("f16_t128_f32out", "conv3x3_f16_bias_relu", "pack_conv3x3_f16_weight", "f16_supported",
           "pd3_conv3x3_f16_bias_relu", (16, 32, 128, 16), "conv_f16.hip:35-44", "f16", bar="f16", cin0=16, cout0=128,
           opts=dict(tile=128, out="f32")),
    Family("f16_t128_gm", "conv3x3_f16_bias_relu", "pack_conv3x3_f16_weight", "f16_supported",
           "pd3_conv3x3_f16_bias_relu", (16, 32, 128, 16), "conv_f16.hip:35-44", "f16", bar="f16", cin0=16, cout0=128,
           out_f16=True, opts=dict(tile=128, out="gm")),
    Family("f16_t64_dual", "conv3x3_f16_bias_relu_dual", "pack_conv3x3_f16_weight", "f16_supported",
           "pd3_conv3x3_f16_bias_relu_dual", (16, 32, 64, 16), "conv_f16.hip:35-44", "f16", bar="f16", cin0=16, cout0=64,
           out_f16=True, opts=dict(tile=64, out="dual")),
    Family("f16_t128_dual", "conv3x3_f16_bias_relu_dual", "pack_conv3x3_f16_weight", "f16_supported",
           "pd3_conv3x3_f16_bias_relu_dual", (16, 32, 128, 16), "conv_f16.hip:35-44", "f16", bar="f16", cin0=16, cout0=128,
           out_f16=True, opts=dict(tile=128, out="dual")),
    # conv_f16.hip:354 kCs2R = 8 output rows, kCfCols = 32 columns, 128 channels (pack tile 128)
    Family("s2_f16", "conv3x3_s2_f16_bias_relu", "pack_conv3x3_f16_weight", "s2_f16_supported",
           "pd3_conv3x3_s2_f16_bias_relu", (8, 32, 128, 16), "conv_f16.hip:354-362", "f16s2", bar="f16", cin0=16, cout0=128,
           stride=2, out_f16=True, opts=dict(tile=128)),
    # conv_f16.hip:922 tiles of 8 x 32 pixels, one group of 64 channels per block
    Family("grouped_f16", "grouped_conv3x3_small_f16", "pack_grouped_weight_f16", "-", "pd3_grouped_conv3x3_small_f16",
           (8, 32, 4, 64), "conv_f16.hip:922", "groupedf16", bar="f16", cin0=64, cout0=1),
    Family("grouped_f16_gm", "grouped_conv3x3_small_f16", "pack_grouped_weight_f16", "-",
           "pd3_grouped_conv3x3_small_f16_gm", (8, 32, 4, 64), "conv_f16.hip:767", "groupedf16", bar="f16", cin0=64, cout0=1,
           opts=dict(group_major_in=True)),
    # conv3x3.hip:414-421 the fused first layer's tiles: 2 x 128 / 2 x 64, else 4 x 32
    Family("scatter_f32", "scatter_conv3x3_bias_relu", "pack_conv3x3_weight", "scatter_conv_supported",
           "pd3_scatter_conv3x3_bias_relu", (4, 32, 64, 8), "conv3x3.hip:414-421", "scatter", stride=2),
    Family("scatter_f16_t64", "scatter_conv3x3_s2_f16_bias_relu", "pack_conv3x3_f16_weight",
           "scatter_conv_s2_f16_supported", "pd3_scatter_conv3x3_s2_f16_bias_relu", (8, 32, 64, 16), "conv_f16.hip:354-362",
           "scatter", bar="f16", cin0=16, cout0=64, stride=2, out_f16=True, opts=dict(tile=64)),
    Family("scatter_f16_t128", "scatter_conv3x3_s2_f16_bias_relu", "pack_conv3x3_f16_weight",
           "scatter_conv_s2_f16_supported", "pd3_scatter_conv3x3_s2_f16_bias_relu", (8, 32, 128, 16), "conv_f16.hip:354-362",
           "scatter", bar="f16", cin0=16, cout0=128, stride=2, out_f16=True, opts=dict(tile=128)),
    # pillar_conv.hip + sparse_conv_x3.hip: rows of active output pixels, no pixel tile of its own: stated as 8 x 32
    Family("scatter_sparse", "scatter_conv3x3_sparse", "sparse", "scatter_conv_sparse_supported",
           "pd3_pillar_conv_rulebook", (8, 32, 64, 16), "pillar_conv.hip", "scatter", bar="sparse", cin0=16, cout0=64,
           stride=2, extra_channels=((16, 128), (48, 128))),
]}

# The bars of the random class: what the suite already holds for the same kernel on the same distribution.
BARS = {
    "fp32": "abs 2e-4 on unit-variance x and 1/sqrt(fan-in) weights (tests/test_conv_gpu.py: test_conv3x3_matches_torch)",
    "x3": "err <= max(2 * err of the fp32 kernel, 2e-7 * mag) and err < 2e-6 * mag on normal x log-normal data "
          "(test_*_bf16x3_is_fp32_arithmetic)",
    "f16": "2e-4 * max(1, mag) on fp16-rounded operands, + 1e-3 * mag where the output is fp16 "
           "(test_conv3x3_f16_matches_fp32_math_on_fp16_operands)",
    "sparse": "err <= max(2 * err of the dense fp32 kernel, 2e-6 * mag) and err < 1e-3 "
              "(test_scatter_conv_as_sparse_convolution)",
}


# ---- case generation -------------------------------------------------------------------------------------------------------
def _dedup(cases):
    seen, out = set(), []
    for c in cases:
        key = (c.n, c.cin, c.cout, c.h, c.wv, c.bias, c.relu, c.opt)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def accept_cases(fam: Family):
    """The lattice of `fam`: a cross of the axes through the smallest case (see the module docstring)."""
    T, C = fam.tile[0], fam.tile[1]
    s = fam.stride if fam.kind != "patch" else 1
    mode = fam.opts.get("mode")
    # The sweep is stated on the map the tile geometry is stated on: the OUTPUT map for the 3x3 families and patch mode 0
    # (input = `up` x that), the INPUT plane for patch modes 1..3 (256 consecutive pixels of it are one tile).
    up = 2 if mode == 0 else (1 if fam.kind == "patch" else s)
    base_opt = {}
    if fam.kind in ("grouped", "groupedf16"):
        base_opt["groups"] = 2
    ci, co = fam.cin0, fam.cout0
    if fam.kind in ("grouped", "groupedf16"):
        co = 3
    if fam.name == "patch1":
        co = 18  # (the SSD head's kind of channel count: not a multiple of anything)

    def mk(axis, n, cin, cout, ho, wo, **kw):
        opt = dict(base_opt)
        opt.update({k: v for k, v in kw.items() if k not in ("bias", "relu")})
        first = None
        for dh, dw in sorted(((a, b) for a in range(4) for b in range(33)), key=sum):  # the nearest shape the predicate takes
            c = _case(fam.name, axis, n, cin, cout, (ho + dh) * up, (wo + dw) * up, kw.get("bias", True),
                      kw.get("relu", True), **opt)
            first = first or c
            if fam.accepts(c):
                return c
        return first

    out = []
    w0, h0 = C, T            # the spatial sweeps run at one full tile of the other axis
    for ho in (1, 2, 3, T - 1, T, T + 1, 2 * T + 1):
        out.append(mk("height", 1, ci, co, max(1, ho), w0))
    widths = [4, C - 4, C, C + 4, 2 * C + 4] + ([C - 2] if fam.pitch_ok else [])
    if fam.pitch_ok and s == 2 and fam.kind == "nchw3":
        widths.append(C - 1)  # an odd output width: the INPUT rows carry padding columns as well
    for wo in sorted(set(widths)):
        if wo > 0:
            out.append(mk("width", 1, ci, co, h0, wo))
    for n in PTILE_COUNTS:
        out.append(mk("ptiles", n, ci, co, h0, w0))
    hs, ws = min(T, 8), min(C, 16) + 4    # the channel sweep's small map: a partial tile
    chans = [(ci, co), (3 * ci, co), (ci, 3 * co), (3 * ci, 3 * co)] + list(fam.extra_channels)
    if fam.kind in ("grouped", "groupedf16"):
        chans = [(ci, k) for k in (1, 2, 3, 4)] + ([(3 * ci, 3)] if fam.kind == "grouped" else [])
    for cin, cout in chans:
        out.append(mk("channels", 1, cin, cout, hs, ws))
    if fam.kind in ("grouped", "groupedf16"):
        for g in (1, 2, 3):
            out.append(mk("channels", 1, ci, co, hs, ws, groups=g))
        # a slice of the groups written into a wider output (the head's slices)
        out.append(mk("epilogue", 1, ci, co, hs, ws, groups=2, out_groups=5, out_group0=2))
    for bias, relu in ((False, True), (True, False), (False, False)):
        if fam.needs_bias() and not bias:
            continue
        if fam.kind in ("grouped", "groupedf16") and not relu:
            continue  # (the grouped kernels have no ReLU)
        out.append(mk("epilogue", 2, ci, co, hs, ws, bias=bias, relu=relu))
    if fam.kind == "patch":
        out.append(mk("epilogue", 2, ci, co, hs, ws, off=8, ctot=co + 24))
        out.append(mk("epilogue", 1, ci, co, hs, ws, off=0, ctot=co + 8, relu=False))
    if fam.kind in ("grouped", "groupedf16"):
        out = [Case(c.family, c.axis, c.n, c.cin, c.cout, c.h, c.wv, c.bias, False, c.opt) for c in out]
    return [c for c in _dedup(out) if fam.accepts(c)]


def _mutate(c: Case, axis, **kw):
    opt = dict(c.opt)
    fields = {k: kw.pop(k) for k in list(kw) if k in ("n", "cin", "cout", "h", "wv")}
    opt.update(kw)
    return Case(c.family, "refuse:" + axis, fields.get("n", c.n), fields.get("cin", c.cin), fields.get("cout", c.cout),
                fields.get("h", c.h), fields.get("wv", c.wv), c.bias, c.relu, tuple(sorted(opt.items())))


def refuse_cases(fam: Family):
    """For every clause of the family's predicate the nearest shape that breaks only that clause: (clause, base case the
    predicate accepts, the refused case)."""
    base = next(c for c in accept_cases(fam) if c.axis == "channels")
    k, out = fam.kind, []
    T = fam.opts.get("tile")
    if k == "nchw3":
        step = {"supported": 8, "winograd_supported": 8, "winograd43_supported": 4, "winograd43_pp_supported": 8,
                "conv3x3_s2_x3_supported": 16}[fam.predicate]
        out.append((f"cin % {step}", _mutate(base, "cin", cin=base.cin + step // 2)))
        cstep = fam.cout0
        out.append((f"cout % {cstep}", _mutate(base, "cout", cout=base.cout + cstep // 2)))
        if fam.stride == 2:
            out.append(("h % 2", _mutate(base, "h", h=base.h + 1)))
            out.append(("w % 2", _mutate(base, "w", wv=base.wv + 1)))
        if fam.predicate in ("winograd_supported", "winograd43_pp_supported"):
            out.append(("w % 4", _mutate(base, "w", wv=base.wv + 2, pitch=base.wv + 2)))
        if fam.predicate == "supported":
            out.append(("stride in (1, 2)", _mutate(base, "stride", stride=3, h=6, wv=12)))
        if fam.predicate == "conv3x3_s2_x3_supported":
            out.append(("cout <= 1024", _mutate(base, "cout1152", cout=1152)))
    elif k == "patch":
        mode, x3 = fam.opts["mode"], fam.predicate == "patch_x3_supported"
        kc = {0: 16 if x3 else 4, 1: 32 if x3 else 16, 2: 32 if x3 else 16, 3: 16}[mode]
        out.append((f"cin % {kc}", _mutate(base, "cin", cin=base.cin + kc // 2)))
        if fam.cout0 > 1:
            out.append((f"cout % {fam.cout0}", _mutate(base, "cout", cout=base.cout + fam.cout0 // 2)))
        if mode == 0:
            out.append((f"h % {2 if x3 else 4}", _mutate(base, "h", h=base.h + 1)))
            wq = 64 if x3 else 4
            out.append((f"w % {wq}", _mutate(base, "w", wv=base.wv + wq // 2, pitch=base.wv + wq // 2)))
        else:
            out.append(("(h * w) % 4", _mutate(base, "hw", h=3, wv=6, pitch=6)))
        if x3:
            out.append(("cout <= 1024", _mutate(base, "cout1152", cout=1152)))
    elif k == "grouped":
        out.append(("cin_per_group % 4", _mutate(base, "cin", cin=base.cin + 2)))
        out.append(("cout_per_group <= 4", _mutate(base, "cout", cout=5)))
        out.append(("w % 4", _mutate(base, "w", wv=base.wv + 2, pitch=base.wv + 2)))
    elif k == "groupedf16":
        out.append(("channels per group == 64", _mutate(base, "cin", cin=32)))
        out.append(("cout_per_group <= 4", _mutate(base, "cout", cout=5)))
    elif k in ("f16", "f16s2"):
        out.append(("cin % 16", _mutate(base, "cin", cin=base.cin + 8)))
        out.append((f"cout % {T}", _mutate(base, "cout", cout=base.cout + T // 2)))
    else:  # scatter
        step = fam.cin0
        out.append((f"cin % {step}", _mutate(base, "cin", cin=base.cin + step // 2)))
        out.append(("cout % 64" if fam.name != "scatter_sparse" else "cout in (64, 128)",
                    _mutate(base, "cout", cout=base.cout + 32 if fam.name != "scatter_sparse" else 192)))
        if fam.name == "scatter_sparse":
            out.append(("wo % 4", _mutate(base, "w", wv=base.wv + 2)))
        else:
            out.append(("ny % 2", _mutate(base, "h", h=base.h + 1)))
            out.append(("nx % 2", _mutate(base, "w", wv=base.wv + 1)))
    return [(clause, base, c) for clause, c in out]  # (the tests assert: base accepted, refused case not)


def all_accepts():
    return [c for f in FAMILIES.values() for c in accept_cases(f)]


def all_refusals():
    return [(clause, c) for f in FAMILIES.values() for clause, _, c in refuse_cases(f)]


# ---- data ------------------------------------------------------------------------------------------------------------------
def _seed(c: Case) -> int:
    return zlib.crc32(repr((c.family, c.n, c.cin, c.cout, c.h, c.wv, c.opt)).encode()) & 0x7fffffff


def exact_bound(fam: Family, c: Case, xm: int, wm: float, bm: int) -> float:
    """Largest magnitude any partial sum of the case can reach: K * max|x| * max|w| (+ bias).  F(2,3) sums the same
    products after its transforms: B^T d B grows an input by 16, G g G^T keeps |U| <= 9/4 max|w|, A^T M A sums 16
    components -- stated as a factor 64 over the direct form."""
    k = fam.fan_in(c) * xm * wm + bm
    return k * (64 if fam.name == "wino23" else 1)


def exact_limits(fam: Family, c: Case):
    """(max|x|, max|w|, max|bias|, weight step) of the exact class, chosen so that exact_bound stays below 2^24 (2^11 where
    the output is fp16).  F(2,3): weights are multiples of 4 so that U = G g G^T is integer; F(4,3): |w| <= 2."""
    limit = 2 ** 11 if fam.out_f16 else 2 ** 24
    if fam.name == "wino23":
        return 4, 8, 4, 4
    for xm, wm in ((4, 2), (4, 1), (2, 1), (1, 1)):
        if exact_bound(fam, c, xm, wm, 4) < limit:
            return xm, wm, 4, 1
    return 1, 0.25, 4, 0.25  # dyadic fractions: every sum a multiple of 1/4


def make_data(fam: Family, c: Case, kind: str):
    """(x [n, groups * cin, h, wv], weight in torch's layout, bias or None) on the CPU, fp32.  kind = exact / random."""
    g = torch.Generator().manual_seed(_seed(c) + (kind == "random"))
    chans = fam.groups(c) * c.cin
    shape = (c.n, chans, c.h, c.wv)
    wshape = fam.weight_shape(c)
    nb = wshape[1] if (fam.kind == "patch" and fam.opts["mode"] >= 2) else wshape[0]
    if kind == "exact":
        xm, wm, bm, step = exact_limits(fam, c)
        x = torch.randint(-xm, xm + 1, shape, generator=g).float()
        q = int(wm / step)
        w = torch.randint(-q, q + 1, wshape, generator=g).float() * step
        b = torch.randint(-bm, bm + 1, (nb,), generator=g).float()
        bound = exact_bound(fam, c, xm, wm, bm)
        assert bound < (2 ** 11 if fam.out_f16 else 2 ** 24), (c.id, bound)  # the precondition of bit equality
        assert float(x.abs().max()) <= xm and float(w.abs().max()) <= wm
    else:
        x = torch.randn(shape, generator=g)
        if fam.bar in ("x3", "sparse"):  # values spread over e^+-3 (sparse: e^N(0,1), as its own test has it)
            spread = (3 * (2 * torch.rand(shape, generator=g) - 1)) if fam.bar == "x3" else torch.randn(shape, generator=g)
            x = x * torch.exp(spread)
        w = torch.randn(wshape, generator=g) / fam.fan_in(c) ** 0.5
        b = torch.randn((nb,), generator=g)
        if fam.bar == "f16":  # operands that are fp16 values already
            x, w = x.half().float(), w.half().float()
    if fam.kind == "scatter":  # a canvas: 40 % of the cells occupied, the others exact zeros
        occ = torch.rand((c.n, 1, c.h, c.wv), generator=g) < 0.4
        x = x * occ
    return x, w, (b if c.bias else None)


def canvas_rows(x):
    """A dense canvas [n, c, ny, nx] as pillar rows: (features [M, c], coords [M, 4] = batch, 0, y, x) of the non-zero
    cells, shuffled, plus padding rows (batch -1) as a fixed-shape voxelizer leaves them."""
    n, ch, ny, nx = x.shape
    occ = (x != 0).any(1)
    idx = occ.nonzero()
    g = torch.Generator().manual_seed(int(idx.shape[0]) + 1)
    idx = idx[torch.randperm(idx.shape[0], generator=g)]
    feats = x[idx[:, 0], :, idx[:, 1], idx[:, 2]]
    coords = torch.stack([idx[:, 0], torch.zeros_like(idx[:, 0]), idx[:, 1], idx[:, 2]], 1).int()
    pad = torch.tensor([[-1, 0, 0, 0]] * 3, dtype=torch.int32)
    return torch.cat([feats, torch.ones(3, ch)], 0).contiguous(), torch.cat([coords, pad], 0).contiguous()


# ---- F(4x4, 3x3) restated in float32 (the bar of the exact class for the Winograd F(4,3) kernels) -----------------------------
_G43 = [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
        [0, 0, 1]]
_BT43 = [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
         [0, 4, 0, -5, 0, 1]]
_AT43 = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]


def winograd43_f32(x, w, b, relu):
    """conv3x3 / pad 1 of x [n, cin, h, w] as F(4x4, 3x3) in float32 on the CPU: U = G g G^T (rounded to fp32 from fp64
    as pack_winograd43_weight does), V = B^T d B, M = sum over cin of U * V, Y = A^T M A."""
    n, cin, h, wd = x.shape
    g64 = torch.tensor(_G43, dtype=torch.float64)
    bt, at = torch.tensor(_BT43, dtype=torch.float32), torch.tensor(_AT43, dtype=torch.float32)
    u = torch.einsum("ij,ocjk,lk->ocil", g64, w.double(), g64).float()
    th, tw = -(-h // 4), -(-wd // 4)
    xp = F.pad(x.float(), (1, 4 * tw - wd + 1, 1, 4 * th - h + 1))
    d = xp.unfold(2, 6, 4).unfold(3, 6, 4)                       # [n, cin, th, tw, 6, 6]
    v = torch.einsum("ij,ncyxjk,lk->ncyxil", bt, d, bt)
    m = torch.einsum("ocil,ncyxil->noyxil", u, v)
    y = torch.einsum("ij,noyxjk,lk->noyxil", at, m, at)          # [n, cout, th, tw, 4, 4]
    y = y.permute(0, 1, 2, 4, 3, 5).reshape(n, -1, 4 * th, 4 * tw)[:, :, :h, :wd]
    if b is not None:
        y = y + b.float().view(1, -1, 1, 1)
    return torch.relu(y) if relu else y


# ---- unpackers: the packers' documented layouts read backwards ------------------------------------------------------------------
def _g_from_u(u, kind):
    """The 3x3 kernel back from U = G g G^T along both axes.  F(2,3): g0 = U0, g1 = U1 - U2, g2 = U3.
    F(4,3): g0 = 4 U0, g1 = 3 (U2 - U1), g2 = U5."""
    def axis(t, dim):
        s = [t.select(dim, i) for i in range(t.shape[dim])]
        rows = [s[0], s[1] - s[2], s[3]] if kind == 23 else [4 * s[0], 3 * (s[2] - s[1]), s[5]]
        return torch.stack(rows, dim)
    return axis(axis(u.double(), 2), 3)


def unpack(fam: Family, c: Case, p):
    """The torch-layout weight back from the packed form (float64 for the Winograd forms, where U carries 1/6 and 1/24)."""
    name, cout, cin = fam.packer, fam.groups(c) * c.cout, c.cin
    if name == "pack_conv3x3_weight":
        return p.reshape(cout // 64, cin // 8, 4, 9, 2, 64).permute(0, 5, 1, 2, 4, 3).reshape(cout, cin, 3, 3)
    if name == "pack_winograd_weight":
        return _g_from_u(p.permute(0, 2, 4, 1, 3, 5).reshape(cout, cin, 4, 4), 23)
    if name == "pack_winograd43_weight":
        return _g_from_u(p.permute(0, 2, 4, 1, 3, 5).reshape(cout, cin, 6, 6), 43)
    if name == "pack_winograd43_lane_weight":
        return _g_from_u(p.permute(0, 3, 6, 1, 2, 5, 4, 7).reshape(cout, cin, 6, 6), 43)
    if name == "pack_grouped_weight":
        return p.permute(0, 2, 1, 3).reshape(cout, cin, 3, 3)
    if name == "pack_grouped_weight_f16":
        return p.permute(0, 2, 3, 1).reshape(cout, cin, 3, 3).float()
    if name == "pack_conv3x3_f16_weight":
        t = fam.opts["tile"]
        return p.reshape(cout // t, cin // 16, 9, 2, t, 8).permute(0, 4, 1, 3, 5, 2).reshape(cout, cin, 3, 3).float()
    if name == "pack_conv3x3_s2_x3_weight":
        a = p[:, :, : 3 * 128 * 56].reshape(p.shape[0], p.shape[1], 3, 128, 56)[..., :48].double().sum(2).float()
        return a.reshape(cout // 128, cin // 16, 3, 128, 3, 16).permute(0, 3, 1, 5, 2, 4).reshape(cout, cin, 3, 3)
    mode = fam.opts["mode"]
    if name == "pack_patch_weight_x3":
        a = p[:, :, : 3 * 128 * 40].reshape(p.shape[0], p.shape[1], 3, 128, 40)[..., :32].double().sum(2).float()
        if mode == 0:
            return a.reshape(cout // 128, 2, cin // 16, 128, 16, 2).permute(0, 3, 2, 4, 1, 5).reshape(cout, cin, 2, 2)
        if mode == 1:
            return a.permute(0, 2, 1, 3).reshape(cout, cin, 1, 1)
        return a.reshape(2, cout // 64, cin // 32, 2, 64, 32).permute(2, 5, 1, 4, 0, 3).reshape(cin, cout, 2, 2)
    assert name == "pack_patch_weight"
    m, k = p.shape[0] * 64, p.shape[1] * 16
    a = p.permute(0, 3, 1, 2).reshape(m, k)
    if mode == 0:
        return a.reshape(cout, cin, 2, 2)
    if mode == 1:
        return a[:cout].reshape(cout, cin, 1, 1)
    kk = 2 if mode == 2 else 4
    return a.reshape(cout, kk, kk, cin).permute(3, 0, 1, 2)


# ---- the 2 GB operand clause of the bf16x3 predicates, restated from the launchers -----------------------------------------
OOB = 0x7ffffff0  # bf16x3.hpp:33 kPxOob: the buffer offset no tensor may reach


def patch_x3_bytes_ok(mode, batch, cin, cout, ctot, h, w, w_valid):
    """conv_patch_x3.hip:376-381."""
    if mode == 0:
        ho, wo, nmt, steps, plane = h // 2, w // 2, cout // 128, 2 * (cin // 16), (h // 2) * (w // 2)
    elif mode == 1:
        ho, wo, nmt, steps, plane = h, w, cout // 128, cin // 32, h * w
    else:
        ho, wo, nmt, steps, plane = 2 * h, 2 * w_valid, 2 * (cout // 64), cin // 32, h * w
    xb, ob, wb = batch * cin * h * w * 4, batch * ctot * ho * wo * 4, nmt * steps * 32768
    return xb < OOB and ob < OOB and wb < OOB and -(-plane // 256) * batch < 1 << 28


def s2_x3_bytes_ok(batch, cin, cout, h, w, w_valid):
    """conv_s2_x3.hip:269-275 (w = the input's row pitch)."""
    ho, wo = h // 2, conv.pitch4(w_valid // 2)
    xb, ob, wb = batch * cin * h * w * 4, batch * cout * ho * wo * 4, (cout // 128) * 3 * (cin // 16) * 49152
    return xb < OOB and ob < OOB and wb < OOB and batch * -(-wo // 32) * -(-ho // 8) < 1 << 28
