"""The pillar encoders' border lattice (a helper module like tests/voxel_lattice.py, not a conftest): pillar_feature_net /
hard_vfe in all their kernel forms, pd3_pillar_feature_net_indexed, pointpillars_scatter and voxel_mean.

* form() restates the dispatcher of csrc/pfn.hip: for a shape, a path selector and the entry it says which kernel serves
  (single64, packed32[NV, park, NSL], packed64[park], mfma32, mfma64, generic[waves]) or which status answers.  CONSTANTS
  are its numbers; read_constants() pulls the same numbers out of the kernel source, and tests/test_pfn_lattice_cpu.py
  holds one to the other, so an edit of the dispatcher fails the restatement on the CPU, not a GPU run.
* ref_pfn / ref_voxel_mean / ref_scatter / rows_from_index are NumPy fp64 statements of the reference layers' text
  (pillar_encoder.py:81-105, :156-210, voxel_encoder.py:44-57, :94-138, :220-283, pillar_scatter.py:57-93), not of the
  kernels: decorate, THEN the mask multiply; the mean divides by num_points; the max runs over all P rows.  BatchNorm is
  folded (scale, shift), which is the library's contract.  A row with num_points <= 0 is the padding row of a fixed-shape
  batch: the library writes zeros there (the reference never sees such a row), and so does ref_pfn.
* two value classes.  `exact`: every number on a dyadic grid (points and offsets multiples of 1/4, voxel sizes powers of
  two, integer weights, scales in {+-1, +-2, +-1/2, 0, -0.0}, shifts multiples of 1/4, pillars built from pairs mirrored
  about a dyadic centre so that the cluster mean is that centre), so that every partial sum of every summation order is a
  fp32 number: exact_bound() bounds the largest of them in units of its grid, below 2^24, and a kernel must equal the
  fp64 reference rounded to fp32 bit for bit (up to the sign of a zero, which the reference's own relu leaves open).
  `real`: points uniform in their cells of a grid that lies 100 m off the origin (x - centre cancels), U(-1, 1) / sqrt(in)
  weights, scales of both signs with an exact 0, a -0.0 and a 1e-30.  Its tolerance is per element and derived:
  TOL_C(case) * 2^-24 * A, A = the same net in fp64 on absolute values (|a| + |b| for the subtractions), TOL_C = in_dim +
  2 * c1 + 8 = the lengths of the two dot products plus decoration, division and the two BatchNorm FMAs (in_dim + 8 for a
  one-layer net).  The fp32 torch oracle stays inside it on every real case with more than the factor 2 to spare that
  the CPU test demands (it prints the largest error / bound: 0.13), so the constant is not raised; on the MI355X the
  kernels reach 0.13 of it, 8e-5 in absolute terms.
* geometry is asymmetric: vx != vy != vz, three different offsets, x cells and y cells from different ranges with one
  pillar at (0, 0) and one at the far corner, nonzero batch and z columns (a two-centre net must ignore z).
* the case families are crosses, not products; a case's data comes from a seed derived from its id.

Everything runs on the CPU except upload / launch_path / launch_indexed, which the GPU tests use.
"""
from __future__ import annotations

import re
import zlib
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

# ---- the dispatcher's numbers (csrc/pfn.hip), held to the source by read_constants() --------------------------------------
CONSTANTS = dict(
    pk=8,                         # kPkPillars: pillars per chunk of the packed kernels
    max_waves=8,                  # kPfnMaxWaves
    nv=(13, 13, 20),              # (8 P D + 63) / 64 <= 13 ? 13 : 20
    packed_floats=20,             # 8 P D <= 20 * 64
    park32=(96, 96),              # P D >= 96: the maxima park in the raw points' slot (else 8 * 96 floats more)
    park64=64,                    # HardVFE: P D >= kC1 + 64
    vfe_chunk=(8, 32, 64),        # kPc, kNv, kC1 of the HardVFE launch
    nsl=192,                      # indexed: 8 P <= 192 ? 3 : 4 point slots per lane
    lds_kb=(160, 160),            # the generic kernel halves its waves above, then refuses above
    caps=dict(single64=16, mfma=(8, 8), packed64=2, packed32=3, generic=8),   # grid caps in units of 256 blocks
    pd_limits=(128, 128, 256),    # P D of single64, mfma32, mfma64
    p_limits=(64, 32, 64),        # P of packed64, mfma32, mfma64
    pillars_bits=22,              # indexed: num_pillars < 1 << 22
    span_bits=(24, 24),           # indexed: points_per_frame, list_stride < 1 << 24
    cell_bits=16,                 # indexed: (x | y << 16)
    span_mask=0xFFFFFF,
)
PK = CONSTANTS["pk"]
SENTINEL = -77.0                  # outputs are >= 0 (ReLU) or exactly what the input holds (scatter): -77 is "unwritten"


def read_constants(src: str) -> dict:
    """The same numbers, found in the text of csrc/pfn.hip."""
    def one(pat, cast=int):
        m = re.findall(pat, src)
        assert len(m) == 1, (pat, m)
        return tuple(cast(x) for x in m[0]) if isinstance(m[0], tuple) else cast(m[0])

    def many(pat):
        return tuple(int(x) for x in re.findall(pat, src))

    return dict(
        pk=one(r"constexpr int kPkPillars = (\d+);"),
        max_waves=one(r"constexpr int kPfnMaxWaves = (\d+);"),
        nv=one(r"\+ 63\) / 64 <= (\d+) \? (\d+) : (\d+);"),
        packed_floats=one(r"kPkPillars \* a\.p \* a\.d <= (\d+) \* 64"),
        park32=one(r"a\.p \* a\.d >= (\d+) \? 0 : kPkPillars \* (\d+)\)"),
        park64=one(r"max_points \* num_point_dim >= kC1 \+ (\d+) \? 0"),
        vfe_chunk=one(r"constexpr int kPc = (\d+), kNv = (\d+), kC1 = (\d+);"),
        nsl=one(r"ns3 = kPkPillars \* max_points <= (\d+);"),
        lds_kb=(one(r"sizeof\(float\) > (\d+) \* 1024\) waves >>= 1"), one(r"if \(bytes > (\d+) \* 1024\) return")),
        caps=dict(single64=many(r"ceil_div\(num_pillars, 4\), 256 \* (\d+)\)")[0],
                  mfma=many(r"ceil_div\(num_pillars, 4\), 256 \* (\d+)\)")[1:],
                  packed64=one(r"ceil_div\(nchunks, 4\), 256 \* (\d+)\)"),
                  packed32=one(r"\(int64_t\)kPkPillars\), 4\), 256 \* (\d+)\)"),
                  generic=one(r"ceil_div\(num_pillars, waves\), 256 \* (\d+)\)")),
        pd_limits=many(r"(?<!8 \* )max_points \* num_point_dim <= (\d+)"),
        p_limits=many(r"max_points <= (\d+) &&"),
        pillars_bits=one(r"num_pillars < \(\(int64_t\)1 << (\d+)\)"),
        span_bits=(one(r"points_per_frame < \(\(int64_t\)1 << (\d+)\)"), one(r"list_stride < \(\(int64_t\)1 << (\d+)\)")),
        cell_bits=one(r"\(uint32_t\)co\[2\] << (\d+)\)"),
        span_mask=one(r"w = lane < cntp \? \(\(sp\.x & 0x([0-9A-Fa-f]+)u\)", lambda s: int(s, 16)),
    )


@dataclass(frozen=True)
class Form:
    kernel: str = ""       # "" : no launch, `status` answers
    status: int = 0
    nv: int = 0
    park: bool = False
    nsl: int = 0           # indexed form only
    w2g: bool = False      # W2's second half from global memory (the HardVFE packed form)
    waves: int = 0         # generic kernel
    cap: int = 0           # pillars one trip of the grid covers; above it the kernels stride

    def __str__(self):
        if not self.kernel:
            return f"status{self.status}"
        if self.kernel == "packed32":
            return f"packed32[NV={self.nv},park={int(self.park)},NSL={self.nsl}]"
        if self.kernel == "packed64":
            return f"packed64[park={int(self.park)}]"
        if self.kernel == "generic":
            return f"generic[{self.waves}]"
        return self.kernel


def _packed_ok(P, D, cd, c1, c2):
    k = CONSTANTS
    return c2 != 0 and c1 == 32 and c2 == 64 and P <= 32 and D in (4, 5) and D + 3 + cd <= 12 and \
        k["pk"] * P * D <= k["packed_floats"] * 64


def _packed32(P, D, nsl=0):
    k = CONSTANTS
    le, small, large = k["nv"]
    nv = small if (k["pk"] * P * D + 63) // 64 <= le else large
    return Form("packed32", nv=nv, park=P * D >= k["park32"][0], nsl=nsl, cap=256 * k["caps"]["packed32"] * 4 * k["pk"])


def generic_waves(P, D, cd, c1, c2):
    """Waves per workgroup of the generic kernel, 0 where even one wave does not fit the LDS."""
    in_pad = (D + 3 + cd + 3) // 4 * 4
    w_floats = in_pad * c1 + (2 * c1 * c2 if c2 else 0)
    wave_floats = P * in_pad + P * c1
    waves = CONSTANTS["max_waves"]
    while waves > 1 and (w_floats + waves * wave_floats) * 4 > CONSTANTS["lds_kb"][0] * 1024:
        waves >>= 1
    return waves if (w_floats + waves * wave_floats) * 4 <= CONSTANTS["lds_kb"][1] * 1024 else 0


def form(case, path: int = 0, indexed: bool = False, points_per_frame: int = 1, list_stride: int = 1) -> Form:
    """What pd3_pillar_feature_net_path(path) / pd3_pillar_feature_net_indexed does with the case's shape."""
    k = CONSTANTS
    M, P, D, cd, c1, c2 = case.M, case.P, case.D, case.cd, case.c1, case.c2
    two = c2 != 0
    in_dim = D + 3 + cd
    in_pad = (in_dim + 3) // 4 * 4
    if indexed:
        if M < 0 or P <= 0 or D < 3 or case.vper <= 0 or points_per_frame <= 0 or list_stride <= 0 or cd not in (2, 3):
            return Form(status=-1)
        if M == 0:
            return Form()
        if not two:
            return Form(status=-1)    # the entry takes w2 for granted: a null pointer
        if not (_packed_ok(P, D, cd, c1, c2) and case.vper % k["pk"] == 0 and M % case.vper == 0 and
                M < 1 << k["pillars_bits"] and points_per_frame < 1 << k["span_bits"][0] and
                list_stride < 1 << k["span_bits"][1]):
            return Form(status=-3)
        return _packed32(P, D, nsl=3 if k["pk"] * P <= k["nsl"] else 4)
    if not 0 <= path <= 2 or M < 0 or P <= 0 or D < 3 or cd not in (2, 3):
        return Form(status=-1)
    if M == 0:
        return Form()
    if c1 <= 0 or c1 > 64 or c1 % 4 or (two and not 0 < c2 <= 64):
        return Form(status=-3)
    if P * in_pad < c1:
        return Form(status=-3)
    d45 = D in (4, 5)
    if not two and c1 == 64 and P * D <= k["pd_limits"][0] and d45:
        return Form("single64", cap=256 * k["caps"]["single64"] * 4)
    packed_ok = _packed_ok(P, D, cd, c1, c2)
    packed64_ok = two and c1 == 64 and c2 == 64 and P <= k["p_limits"][0] and D == 4 and cd == 3
    if path == 2 and not packed_ok and not packed64_ok:
        return Form(status=-3)
    if packed64_ok and path != 1:
        return Form("packed64", nv=k["vfe_chunk"][1], park=P * D >= k["vfe_chunk"][2] + k["park64"], w2g=True,
                    cap=256 * k["caps"]["packed64"] * 4 * k["vfe_chunk"][0])
    if packed_ok and path != 1:
        return _packed32(P, D)
    if two and c1 == 32 and c2 == 64 and P * D <= k["pd_limits"][1] and P <= k["p_limits"][1] and d45 and in_dim <= 12:
        return Form("mfma32", cap=256 * k["caps"]["mfma"][0] * 4)
    if two and c1 == 64 and c2 == 64 and P * D <= k["pd_limits"][2] and P <= k["p_limits"][2] and D == 4 and cd == 3:
        return Form("mfma64", cap=256 * k["caps"]["mfma"][1] * 4)
    waves = generic_waves(P, D, cd, c1, c2)
    if not waves:
        return Form(status=-3)
    return Form("generic", waves=waves, cap=256 * k["caps"]["generic"] * waves)


def generic_border(D, cd, c1, c2, waves):
    """The largest P the generic kernel serves with `waves` waves (waves = 0: the first P it refuses)."""
    p = 1
    while generic_waves(p, D, cd, c1, c2) > waves or (waves and generic_waves(p + 1, D, cd, c1, c2) == waves):
        p += 1
    return p


# ---- cases ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    family: str
    id: str
    M: int
    P: int
    D: int
    cd: int
    c1: int
    c2: int                # 0: a one-layer net
    values: str            # exact / real
    fill: str = "mixed"
    shift: str = "plain"   # plain / neg (the padded row is all zeros) / big (the padded row beats every stored row)
    claims: tuple = ()
    seed: str = ""         # cases with the same seed and base_m share one data set; theirs are its first M pillars
    base_m: int = 0
    vper: int = 0          # index family: pillars per frame
    list_extra: int = 0    # index family: list_stride - points_per_frame

    def c(self, key, default=None):
        return dict(self.claims).get(key, default)

    @property
    def cout(self):
        return self.c2 or self.c1

    @property
    def in_dim(self):
        return self.D + 3 + self.cd


def tol_c(case):
    return case.in_dim + (2 * case.c1 if case.c2 else 0) + 8


def _seed(s):
    return zlib.crc32(s.encode())


GEOMETRY = {  # vx, vy, vz, x_off, y_off, z_off; x cells, y cells, z cells (z from 1: the column is never all zero)
    "exact": ((0.25, 0.5, 2.0, -1.25, 0.75, -2.5), 64, 16, 4),
    "real": ((0.2, 0.3, 4.5, -100.3, 100.7, -2.75), 1440, 400, 4),
}


def geometry(case):
    return tuple(float(np.float32(v)) for v in GEOMETRY[case.values][0])


# ---- fill patterns ------------------------------------------------------------------------------------------------------
def _rows_patterns(P):
    """name -> (num_points of a chunk's eight pillars, the claim: R, live mask, end mask of the first 16-row block).
    A rows case has 16 pillars, so its two chunks go to two waves: "R8P-then-ones" and "full-one-full-one" check the
    restart of the running maxima between the pillars of a chunk (from -inf for a full pillar, from the padded row for a
    short one; the cases pair them with the large shift1, so the two starts differ).  The restart between two chunks that
    ONE wave walks is the stride family's: its sets open with a chunk of full pillars and hold one-point pillars at the
    grid cap, and the packed kernels' sets carry the large shift1 too."""
    full = [P] * 8
    return {
        "R0": ([0] * 8, dict(R=0, live=0x00, end0=0x0000)),
        "R1-only-last-live": ([0] * 7 + [1], dict(R=1, live=0x80, end0=0x0001)),
        "R15": ([7, 8] + [0] * 6, dict(R=15, live=0x03, end0=0x4040)),
        "R16-ends-on-block": ([10, 6] + [0] * 6, dict(R=16, live=0x03, end0=0x8200)),
        "R17": ([16, 1] + [0] * 6, dict(R=17, live=0x03, end0=0x8000)),
        "R32": ([16, 16] + [0] * 6, dict(R=32, live=0x03, end0=0x8000)),
        "R8P-then-ones": (full, dict(R=8 * P, live=0xFF)),
        "straddle2": ([10, 10] + [0] * 6, dict(R=20, live=0x03, end0=0x0200)),
        "straddle3": ([15, 20] + [0] * 6, dict(R=35, live=0x03, end0=0x4000)),
        "first-empty": ([0, 5, 3, 0, 0, 0, 0, 2], dict(R=10, live=0x86, end0=0x0290)),
        "alternating": ([3, 0] * 4, dict(R=12, live=0x55, end0=0x0924)),
        "full-one-full-one": ([P, 1] * 4, dict(R=4 * P + 4, live=0xFF)),
        "above-P": ([2 * P, 3, 2 * P, 1, 0, 2 * P, P, P - 1], dict(R=5 * P + 3, live=0xEF)),
    }


ROWS_PATTERNS = tuple(_rows_patterns(20))


def chunk_layout(counts, P):
    """The packed walk's row layout of one chunk, restated: (R, live mask, not-full mask, end mask per 16-row block)."""
    st = np.clip(np.minimum(np.asarray(counts), P), 0, None)
    ends = np.cumsum(st)
    R = int(ends[-1])
    live = sum(1 << q for q in range(len(st)) if st[q] > 0)
    notfull = sum(1 << q for q in range(len(st)) if st[q] < P)
    masks = [0] * ((R + 15) // 16)
    for q in range(len(st)):
        if st[q] > 0:
            masks[(ends[q] - 1) // 16] |= 1 << int((ends[q] - 1) % 16)
    return R, live, notfull, masks


def _counts(case, rng, M):
    P = case.P
    if case.fill == "mixed":
        c = rng.integers(1, P + 1, M)
        # one row short, full, one point, padding, num_points above P (the P rows are summed, the mean divides by 2 P)
        for i, v in ((0, max(P - 1, 1)), (1, P), (2, 1), (3, 0), (4, 2 * P), (5, P), (6, 0), (M - 2, 0)):
            if 0 <= i < M:
                c[i] = v
        return c
    if case.fill == "sparse":      # the stride family: 1 .. 3 points, a few full pillars, a few padding rows
        c = np.minimum(rng.integers(1, 4, M), P)
        c[::97] = P
        c[5::211] = 0
        c[:PK] = P                 # a chunk of full pillars, and the chunk the same wave walks next holds one point each
        cap = case.c("cap")
        if cap and M > cap:
            c[cap:cap + PK] = 1
        return c
    if case.fill == "frames":      # the index family: counts stay within P (the entry's contract)
        c = np.where(rng.random(M) < 0.25, rng.integers(1, P + 1, M), np.minimum(rng.integers(1, 4, M), P))
        c[rng.random(M) < 0.1] = 0
        v = case.vper
        c[0] = P
        c[3::v] = 0                # padding rows in the middle and at the end of every frame
        c[v - 1::v] = 0
        e = case.c("empty_frame")
        if e is not None:
            c[e * v:(e + 1) * v] = 0
        return c
    pat, _ = _rows_patterns(P)[case.fill]
    second = [1] * PK if case.fill == "R8P-then-ones" else list(rng.integers(1, P + 1, PK))
    return np.asarray((pat + second)[:M])


@lru_cache(maxsize=6)
def _base_data(key):
    case = key
    M, P, D = case.base_m or case.M, case.P, case.D
    rng = np.random.default_rng(_seed(case.seed or case.id))
    (vx, vy, vz, xo, yo, zo), ncx, ncy, ncz = GEOMETRY[case.values]
    npv = _counts(case, rng, M).astype(np.int32)
    st = np.clip(np.minimum(npv, P), 0, None)
    co = np.stack([rng.integers(0, 3, M), rng.integers(1, ncz, M), rng.integers(0, ncy, M), rng.integers(0, ncx, M)], 1)
    livei = np.flatnonzero(npv > 0)
    if len(livei):
        co[livei[0], 2:] = 0
        co[livei[0], 0] = 2
        co[livei[-1], 2:] = (ncy - 1, ncx - 1)
    co[npv <= 0] = (-1, 0, 0, 0)
    centre = np.stack([co[:, 3] * vx + xo, co[:, 2] * vy + yo, co[:, 1] * vz + zo], 1)
    k = np.arange(P)
    if case.values == "exact":
        # mirrored pairs about m, plus m itself where the count is odd: the sum of the stored rows is count * m
        m = centre + rng.integers(-4, 5, (M, 3)) / 4.0
        dl = rng.integers(-6, 7, (M, (P + 1) // 2, 3)) / 4.0
        delta = dl[:, k // 2] * np.where(k % 2 == 0, 1.0, -1.0)[None, :, None]
        delta[(st % 2 == 1)[:, None] & (k[None, :] == st[:, None] - 1)] = 0.0
        xyz = m[:, None, :] + delta
        rest = rng.integers(0, 16, (M, P, max(D - 3, 0))) / 4.0
    else:
        xyz = centre[:, None, :] + rng.uniform(-0.5, 0.5, (M, P, 3)) * np.array([vx, vy, vz])
        rest = rng.uniform(0, 1, (M, P, max(D - 3, 0)))
    vox = np.concatenate([xyz, rest], 2)[:, :, :D].astype(np.float32)   # (D < 3 only in the case the entry turns away)
    vox[k[None, :] >= st[:, None]] = 0.0
    return vox, npv, co.astype(np.int32)


def _key(case):
    """The case that owns the shared data set."""
    if not case.seed:
        return case
    return Case(case.family, case.seed, case.base_m, case.P, case.D, case.cd, case.c1, case.c2, case.values, case.fill,
                case.shift, tuple(x for x in case.claims if x[0] in ("cap", "empty_frame")), case.seed, case.base_m,
                case.vper, case.list_extra)


def pillars(case):
    """(voxels [M, P, D] fp32 with zero padded rows, num_points [M] int32, coors [M, 4] int32 = batch, z, y, x)."""
    vox, npv, co = _base_data(_key(case))
    return vox[:case.M], npv[:case.M], co[:case.M]


def params(case):
    """Folded parameters: dict(w1 [in, c1], s1, b1, w2 [2 c1, c2] or None, s2, b2), fp32."""
    rng = np.random.default_rng(_seed("params/" + (case.seed or case.id)))
    exact = case.values == "exact"

    def layer(i, o, wmax, shift):
        if exact:
            w = rng.integers(-wmax, wmax + 1, (i, o)).astype(np.float32)
            s = rng.choice(np.array([1, -1, 2, -2, 0.5, -0.5], np.float32), o)
            b = (rng.integers(-8, 9, o) / 4.0).astype(np.float32)
        else:
            w = (rng.uniform(-1, 1, (i, o)) / np.sqrt(i)).astype(np.float32)
            s = (rng.uniform(0.5, 1.5, o) * rng.choice([-1.0, 1.0], o)).astype(np.float32)
            b = rng.normal(0, 0.2, o).astype(np.float32)
        for j, v in enumerate((0.0, -0.0) if exact else (0.0, -0.0, 1e-30)):   # as many of the specials as fit
            if j + 1 < o:
                s[j + 1] = v
        if shift == "neg":
            b = -np.abs(b) - np.float32(0.25)
        elif shift == "big":
            b = np.abs(b) + np.float32(64.0)
        return w, s.astype(np.float32), b.astype(np.float32)

    w1, s1, b1 = layer(case.in_dim, case.c1, 2, case.shift)
    if not case.c2:
        return dict(w1=w1, s1=s1, b1=b1, w2=None, s2=None, b2=None)
    w2, s2, b2 = layer(2 * case.c1, case.c2, 1, "plain")
    return dict(w1=w1, s1=s1, b1=b1, w2=w2, s2=s2, b2=b2)


# ---- the references --------------------------------------------------------------------------------------------------------
MUTATIONS = ("swap_v", "swap_xy", "z_in_2d", "min_div", "pad_in_full", "drop_last")


def ref_pfn(vox, npv, coors, prm, geo, cd, mut=None, absolute=False, stages=None, block=2048):
    """PillarFeatureNet.forward / HardVFE.forward (eval, folded BatchNorm) in fp64 -> [M, C].  absolute: the same net on
    absolute values (the A of the tolerance); stages: a dict that receives the largest magnitude of every stage.
    mut: a deliberately wrong variant (MUTATIONS), for the CPU test that shows the cases tell them apart."""
    M = len(npv)
    cout = (prm["w2"] if prm["w2"] is not None else prm["w1"]).shape[1]
    out = np.zeros((M, cout))
    for i in range(0, M, block):
        s = slice(i, i + block)
        out[s] = _ref_block(vox[s], npv[s], coors[s], prm, geo, cd, mut, absolute, stages)
    return out


def _ref_block(vox, npv, coors, prm, geo, cd, mut, absolute, stages):
    f = vox.astype(np.float64)
    M, P, _ = f.shape
    a = np.abs if absolute else (lambda v: v)
    sgn = 1.0 if absolute else -1.0

    def note(name, v):
        if stages is not None and v.size:
            stages[name] = max(stages.get(name, 0.0), float(np.abs(v).max()))

    live = npv > 0
    n = np.where(live, npv, 1).astype(np.float64)
    if mut == "min_div":
        n = np.minimum(n, P)
    vx, vy, vz, xo, yo, zo = (float(v) for v in geo)
    if mut == "swap_v":
        vx, vy = vy, vx
    co = coors.astype(np.float64)
    cx, cy, cz = co[:, 3], co[:, 2], co[:, 1]
    if mut == "swap_xy":
        cx, cy = cy, cx
    if mut == "z_in_2d" and cd == 2:
        cy = cz
    f = a(f)
    ssum = f[:, :, :3].sum(1, keepdims=True)               # features[:, :, :3].sum(axis=1, keepdim=True)
    note("sum", ssum)
    mean = ssum / n.reshape(-1, 1, 1)                      # / num_points
    f_cluster = f[:, :, :3] + sgn * mean
    centre = np.stack([a(cx) * a(vx) + a(xo), a(cy) * a(vy) + a(yo), a(cz) * a(vz) + a(zo)], 1)[:, None, :cd]
    f_center = f[:, :, :cd] + sgn * centre
    x = np.concatenate([f, f_cluster, f_center], -1)
    k = np.arange(P)
    x = x * (npv.reshape(-1, 1) > k.reshape(1, -1))[:, :, None]   # get_paddings_indicator, after the decoration
    note("x", x)
    rows = np.ones((M, P), bool)                           # the max runs over all P rows
    if mut == "drop_last":
        st = np.clip(np.minimum(npv, P), 0, None)
        rows[(k[None, :] == st[:, None] - 1) & (st[:, None] >= 2)] = False
    if mut == "pad_in_full":                               # one more all-zero row, whatever the pillar's count
        x = np.concatenate([x, np.zeros((M, 1, x.shape[2]))], 1)
        rows = np.concatenate([rows, np.ones((M, 1), bool)], 1)
    layers = [(prm["w1"], prm["s1"], prm["b1"])]
    if prm["w2"] is not None:
        layers.append((prm["w2"], prm["s2"], prm["b2"]))
    for li, (w, s, b) in enumerate(layers):
        acc = x @ a(w.astype(np.float64))
        note(f"acc{li + 1}", acc)
        y = np.maximum(acc * a(s.astype(np.float64)) + a(b.astype(np.float64)), 0.0)
        note(f"y{li + 1}", y)
        ymax = np.where(rows[:, :, None], y, -np.inf).max(1, keepdims=True)
        x = ymax if li == len(layers) - 1 else np.concatenate([y, np.broadcast_to(ymax, y.shape)], 2)
    out = x[:, 0, :]
    out[~live] = 0.0
    return out


@lru_cache(maxsize=6)
def _base_ref(key):
    vox, npv, co = _base_data(key)
    prm, geo = params(key), geometry(key)
    ref = ref_pfn(vox, npv, co, prm, geo, key.cd)
    return ref, ref_pfn(vox, npv, co, prm, geo, key.cd, absolute=True)


def reference(case):
    """(fp64 reference [M, C], per-element tolerance [M, C]: zeros for the exact class)."""
    ref, A = _base_ref(_key(case))
    ref, A = ref[:case.M], A[:case.M]
    if case.values == "exact":
        return ref, np.zeros_like(ref)
    return ref, tol_c(case) * 2.0 ** -24 * A


EXACT_UNITS = dict(sum=4, x=8, acc1=8, y1=16, acc2=16, y2=32)   # the dyadic grid of every stage, as 1 / step


def exact_stages(case):
    """The largest magnitude any partial sum of an exact case's stages can reach, from the limits the exact class draws its
    values within (not from the data): sums of absolute values bound the partial sums of every summation order, in the
    manner of conv_lattice.exact_bound.  A point lies within 2.5 of its pillar centre (the mirror centre within 1, a pair
    within 1.5 of that), further columns below 4, |W1| <= 2, |W2| <= 1, |scale| <= 2, |shift| <= 2 (66 for `big`)."""
    (vx, vy, vz, xo, yo, zo), ncx, ncy, ncz = GEOMETRY["exact"]
    c = [(ncx - 1) * vx + abs(xo), (ncy - 1) * vy + abs(yo), (ncz - 1) * vz + abs(zo)]
    p = [v + 2.5 for v in c]
    row = sum(p) + max(case.D - 3, 0) * 3.75 + sum(2 * v for v in p) + sum(p[i] + c[i] for i in range(case.cd))
    st = dict(sum=case.P * max(p), x=max(2 * max(p), max(p[i] + c[i] for i in range(case.cd))), acc1=2 * row)
    st["y1"] = 2 * st["acc1"] + {"plain": 2.0, "neg": 2.25, "big": 66.0}[case.shift]
    if case.c2:
        st["acc2"] = 2 * case.c1 * st["y1"]
        st["y2"] = 2 * st["acc2"] + 2.0
    return st


def exact_bound(case):
    """exact_stages in units of the grid each stage lives on.  Points, offsets and shifts are multiples of 1/4 and the
    weights integers, so the sums of the points live on 1/4; the cluster mean of a pillar with num_points = 2 P is half its
    centre, so the decorated rows and layer 1's dot product live on 1/8; a scale of 1/2 takes y1 and layer 2's dot product
    to 1/16 and y2 to 1/32.  Below 2^24 every one of them is a fp32 number."""
    return max(v * EXACT_UNITS[k] for k, v in exact_stages(case).items())


def measured_stages(case, rows=None):
    """The same maxima measured on the case's data (the fp64 net on absolute values)."""
    vox, npv, co = pillars(case)
    if rows is not None:
        vox, npv, co = vox[rows], npv[rows], co[rows]
    st = {}
    ref_pfn(vox, npv, co, params(case), geometry(case), case.cd, absolute=True, stages=st)
    return st


def reference_rows(case, rows):
    """reference() of some of a case's pillars, computed on the spot (the CPU tests' samples of the large shared sets)."""
    vox, npv, co = pillars(case)
    prm, geo = params(case), geometry(case)
    ref = ref_pfn(vox[rows], npv[rows], co[rows], prm, geo, case.cd)
    if case.values == "exact":
        return ref, np.zeros_like(ref)
    return ref, tol_c(case) * 2.0 ** -24 * ref_pfn(vox[rows], npv[rows], co[rows], prm, geo, case.cd, absolute=True)


def compare(case, out, ref, tol):
    """None, or what is wrong with a kernel's output."""
    if not np.isfinite(out).all():
        return "non-finite output"
    if case.values == "exact":
        bad = out != ref.astype(np.float32)
    else:
        bad = np.abs(out.astype(np.float64) - ref) > tol
    if not bad.any():
        return None
    r, c = np.argwhere(bad)[0]
    return f"{int(bad.sum())} elements differ, first at pillar {r} channel {c}: got {out[r, c]!r}, reference {ref[r, c]!r}, " \
           f"tolerance {tol[r, c]!r}"


def ref_voxel_mean(vox, npv):
    """VoxelMean.forward: the sum over all P rows / num_points (a zero count divides by zero: nan or +-inf)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return vox.astype(np.float64).sum(1) / npv.astype(np.float64).reshape(-1, 1)


def ref_scatter(feats, coords, batch, ny, nx, first_wins=False):
    """PointPillarsScatter.forward_batch: a zeros canvas per sample, paddle.scatter(overwrite=True) of the sample's rows
    at y * nx + x -- the last writer of a cell wins --, transposed to [C, ny * nx].  Rows whose batch or cell lies outside
    (the -1 padding rows of a fixed-shape batch among them) are dropped, which is the library's contract.
    Returns (canvas [B, C, ny, nx], inverse map [B, ny * nx]: the winning row, -1 for an empty cell)."""
    M, C = feats.shape
    b, y, x = coords[:, 0].astype(np.int64), coords[:, 2].astype(np.int64), coords[:, 3].astype(np.int64)
    ok = (b >= 0) & (b < batch) & (y >= 0) & (y < ny) & (x >= 0) & (x < nx)
    rows = np.flatnonzero(ok)
    cell = (b[rows] * ny + y[rows]) * nx + x[rows]
    inv = np.full(batch * ny * nx, -1, np.int64)
    if first_wins:
        big = np.full(batch * ny * nx, M, np.int64)
        np.minimum.at(big, cell, rows)
        inv = np.where(big < M, big, -1)
    else:
        np.maximum.at(inv, cell, rows)
    canvas = np.zeros((batch * ny * nx, C), feats.dtype)
    canvas[inv >= 0] = feats[inv[inv >= 0]]
    canvas = canvas.reshape(batch, ny * nx, C).transpose(0, 2, 1).reshape(batch, C, ny, nx)
    return np.ascontiguousarray(canvas), inv.reshape(batch, ny * nx).astype(np.int32)


# ---- a hand-made index (pd3_pillar_feature_net_indexed) ------------------------------------------------------------------
@lru_cache(maxsize=3)
def _base_index(key):
    """(points [F, N, D], span [M, 2], plist [F, list_stride]) that name the pillars of the case: the stored rows lie
    permuted in the frame's cloud among points no pillar holds, the pillars' runs lie in the list in arbitrary order with
    gaps between them (entries no span names hold a valid point index, 0, so that a kernel that read one would be wrong,
    not out of bounds), padding rows read (0, 0)."""
    vox, npv, _ = _base_data(key)
    M, P, D = vox.shape
    v = key.vper
    F = M // v
    rng = np.random.default_rng(_seed("index/" + key.id))
    st = np.clip(npv, 0, P).reshape(F, v)
    n_pts = int(st.sum(1).max()) + 7
    stride = n_pts + key.list_extra
    filler = 7.75 if key.values == "exact" else 3.1
    points = np.full((F, n_pts, D), filler, np.float32)
    plist = np.zeros((F, stride), np.int32)
    span = np.zeros((M, 2), np.int32)
    for f in range(F):
        cnt = st[f]
        total = int(cnt.sum())
        where = rng.permutation(n_pts)[:total]                      # cloud position of the frame's j-th stored row
        q_of = np.repeat(np.arange(v), cnt)
        k_of = np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        points[f, where] = vox[f * v + q_of, k_of]
        order = rng.permutation(v)
        gaps = rng.integers(0, 3, v)
        gaps = np.minimum(gaps, np.maximum(stride - total - (np.cumsum(gaps) - gaps), 0))
        start_in_order = np.cumsum(gaps + cnt[order]) - cnt[order]
        start = np.empty(v, np.int64)
        start[order] = start_in_order
        first = np.cumsum(cnt) - cnt                                  # a pillar's first row among the frame's stored rows
        pos = np.repeat(start, cnt) + k_of
        assert total == 0 or pos.max() < stride
        plist[f, pos] = where[np.repeat(first, cnt) + k_of]
        live = cnt > 0
        span[f * v:(f + 1) * v, 0] = np.where(live, start, 0)
        span[f * v:(f + 1) * v, 1] = cnt
    return points, span, plist


def index_of(case):
    """(points [F, N, D], span [M, 2], plist [F, list_stride]) of an index case: the first M / vper frames of its set."""
    points, span, plist = _base_index(_key(case))
    F = case.M // case.vper
    return points[:F], span[:case.M], plist[:F]


def rows_from_index(points, span, plist, P):
    """The padded tensor an index stands for: (voxels [M, P, D] with zero padded rows, num_points [M])."""
    F, _, D = points.shape
    M = len(span)
    v = M // F
    frame = np.arange(M) // v
    k = np.arange(P)
    cnt = np.minimum(span[:, 1], P)
    valid = k[None, :] < cnt[:, None]
    li = np.where(valid, span[:, :1] + k[None, :], 0)
    pid = plist[frame[:, None], li]
    vox = points[frame[:, None], pid] * valid[:, :, None]
    return vox.astype(np.float32), span[:, 1].astype(np.int32)


# ---- the families ------------------------------------------------------------------------------------------------------
def _net(c1, c2, cd):
    return ("vfe" if cd == 3 else "pfn") + (f"{c1}x{c2}" if c2 else f"{c1}")


def _mk(family, tag, M, P, D, cd, c1, c2, values, **kw):
    cid = f"{family}-{tag + '-' if tag else ''}{_net(c1, c2, cd)}-P{P}-D{D}-M{M}-{values}"
    return Case(family, cid, M, P, D, cd, c1, c2, values, **kw)


def _both(*a, **kw):
    return [_mk(*a, v, **kw) for v in ("exact", "real")]


PD_TWO = ((26, 4), (21, 5), (19, 5), (24, 4), (20, 5), (24, 5), (25, 4), (25, 5), (32, 4), (26, 5), (32, 5), (33, 4),
          (16, 4), (17, 4), (1, 4), (2, 5))
WAVE_NET = dict(D=5, cd=2, c1=64, c2=64)    # a two-layer net no fast form takes (64 / 64 with D = 5): the generic kernel
STRIDE_NETS = (("packed32", 0, 20, 5, 2, 32, 64), ("mfma32", 1, 20, 5, 2, 32, 64), ("single64", 0, 20, 5, 2, 64, 0),
               ("generic", 0, 8, 3, 2, 32, 64), ("packed64", 0, 64, 4, 3, 64, 64), ("mfma64", 1, 64, 4, 3, 64, 64))
INDEX_SHAPES = ((20, 5, 2, 8, 1), (20, 4, 3, 8, 5), (24, 4, 2, 16, 2), (24, 5, 3, 16, 5), (25, 4, 3, 4096, 1),
                (25, 5, 2, 4096, 2), (32, 4, 2, 8, 2), (32, 5, 3, 4096, 5))     # P, D, cd, pillars per frame, frames


def _build():
    cs = []
    # -- dispatch
    for P, D in PD_TWO:
        for cd in (2, 3):
            cs += _both("dispatch", "", 67, P, D, cd, 32, 64)
    for P, D in ((25, 5), (32, 4), (26, 5)):                       # P D = 125, 128, 130: single64 | generic
        cs += _both("dispatch", f"PD{P * D}", 67, P, D, 2, 64, 0)
    for P in (16, 17, 31, 32, 33, 48, 64, 65):
        cs += _both("dispatch", "", 67, P, 4, 3, 64, 64)
    for c1 in (4, 12, 36, 60, 64):
        cs += _both("dispatch", "width", 67, 9, 4, 2, c1, 17)
    for c2 in (1, 3, 63, 64):
        cs += _both("dispatch", "width", 67, 9, 4, 2, 36, c2)
    for D, cd in ((3, 2), (3, 3), (6, 2), (6, 3), (7, 2), (7, 3)):   # D = 7 with three centre dims: in_dim = 13 > 12
        cs += _both("dispatch", "width", 67, 9, D, cd, 32, 64)
    cs += _both("dispatch", "width", 67, 9, 4, 2, 32, 0)
    cs += _both("dispatch", "xs-holds-c1", 67, 5, 4, 2, 64, 17, claims=(("status", -3),))   # P * in_pad = 60 < 64
    cs += _both("dispatch", "xs-holds-c1", 67, 6, 4, 2, 64, 17, claims=(("waves", 8),))
    w = WAVE_NET
    for waves in (8, 4, 2, 1):
        last = generic_border(w["D"], w["cd"], w["c1"], w["c2"], waves)
        cs += _both("dispatch", f"waves{waves}-last", 67, last, w["D"], w["cd"], w["c1"], w["c2"], claims=(("waves", waves),))
        if waves > 1:
            cs += _both("dispatch", f"waves{waves // 2}-first", 67, last + 1, w["D"], w["cd"], w["c1"], w["c2"],
                        claims=(("waves", waves // 2),))
    cs += _both("dispatch", "waves0-refused", 67, generic_border(w["D"], w["cd"], w["c1"], w["c2"], 0), w["D"], w["cd"],
                w["c1"], w["c2"], claims=(("status", -3),))
    for M in (1, 7, 8, 9):
        cs += _both("dispatch", "", M, 20, 5, 2, 32, 64)
        cs += _both("dispatch", "", M, 64, 4, 3, 64, 64)
    cs += _both("dispatch", "D2-invalid", 67, 9, 2, 2, 32, 64, claims=(("status", -1),))
    # the padded row against the stored rows: all zeros, and above every stored row (a full pillar must not contain it, a
    # pillar one row short must; `mixed` puts both at the head of the case)
    for shift in ("neg", "big"):
        for P, D, cd, c1, c2 in ((20, 5, 2, 32, 64), (32, 4, 3, 32, 64), (20, 5, 2, 64, 0), (64, 4, 3, 64, 64),
                                 (9, 4, 2, 36, 17)):
            cs += _both("dispatch", f"shift1-{shift}", 67, P, D, cd, c1, c2, shift=shift)
    # -- rows: the packed walk's row layouts, one chunk built on purpose and one ordinary chunk behind it
    # both LDS layouts of both packed kernels: P D = 100, 128 (32 / 64) and 256 (64 / 64) park a pillar's maxima in the
    # slot of its raw points, P D = 92 and 124 in their own slots
    for P, D, cd, c1, c2 in ((20, 5, 2, 32, 64), (32, 4, 3, 32, 64), (64, 4, 3, 64, 64), (23, 4, 2, 32, 64),
                             (31, 4, 3, 64, 64)):
        for name in ROWS_PATTERNS:
            claims = tuple(_rows_patterns(P)[name][1].items())
            cs += _both("rows", name, 16, P, D, cd, c1, c2, fill=name, claims=claims,
                        shift="big" if name in ("full-one-full-one", "R8P-then-ones") else "plain")
    # -- stride: both sides of one trip and of two trips of every kernel's grid; one data set per kernel and class
    for kernel, path, P, D, cd, c1, c2 in STRIDE_NETS:
        cap = form(Case("", "", 1, P, D, cd, c1, c2, "real"), path).cap
        sizes = (cap - 8, cap, cap + 8) + ((2 * cap, 2 * cap + 8) if kernel != "packed64" else ())
        for values in ("exact", "real"):
            for M in sizes:
                # the packed kernels with the large shift1: the wave that walked the chunk of full pillars (maxima from
                # -inf) walks the chunk of one-point pillars next (maxima from the padded row, which then wins)
                cs.append(_mk("stride", kernel, M, P, D, cd, c1, c2, values, fill="sparse", base_m=max(sizes),
                              shift="big" if kernel.startswith("packed") else "plain",
                              seed=f"stride/{kernel[:6]}/{P}/{D}/{cd}/{c1}/{c2}/{cap}/{values}",
                              claims=(("cap", cap), ("kernel", kernel), ("path", path))))
    # -- index
    for i, (P, D, cd, vper, frames) in enumerate(INDEX_SHAPES):
        claims = (("frames", frames),) + ((("empty_frame", 2),) if frames == 5 else ())
        cs += _both("index", f"v{vper}-f{frames}", vper * frames, P, D, cd, 32, 64, fill="frames", vper=vper,
                    list_extra=(0, 9, 64)[i % 3], claims=claims)
    cap = form(Case("", "", 1, 20, 5, 2, 32, 64, "real"), 0).cap
    for values in ("exact", "real"):
        for M in (cap - 8, cap, cap + 8, 2 * cap, 2 * cap + 8):
            cs.append(_mk("index", "stride-v8", M, 20, 5, 2, 32, 64, values, fill="frames", vper=8, list_extra=5,
                          base_m=2 * cap + 8, seed=f"index-stride/{values}", claims=(("cap", cap), ("frames", M // 8))))
    return tuple(cs)


CASES = _build()


def family(name):
    return [c for c in CASES if c.family == name]


def paths(case):
    """The path selectors a case runs with: all three, or the one its claim names."""
    p = case.c("path")
    return (0, 1, 2) if p is None else (p,)


# ---- pointpillars_scatter / voxel_mean --------------------------------------------------------------------------------
@dataclass(frozen=True)
class ScatterCase:
    id: str
    M: int
    C: int
    batch: int
    ny: int
    nx: int
    kind: str = "unique"     # unique / dup2 / dup50 / invalid
    feats_off: int = 0       # floats past a 16-byte boundary
    out_off: int = 0

    @property
    def vec4(self):
        """The float4 writer runs: plane and channels multiples of 4, both pointers on 16 bytes."""
        return (self.ny * self.nx) % 4 == 0 and self.C % 4 == 0 and not self.feats_off and not self.out_off


def _scatter_cases():
    cs = [ScatterCase(f"scatter-C{c}-plane64", 40, c, 2, 8, 8) for c in (1, 3, 4, 8, 65)]
    cs += [ScatterCase(f"scatter-C{c}-plane{ny * nx}", 20, c, 2, ny, nx) for c in (4, 8) for ny, nx in ((5, 5), (6, 7))]
    cs += [ScatterCase("scatter-dup2-last-row-writes", 42, 8, 2, 8, 8, "dup2"),
           ScatterCase("scatter-dup50-last-row-writes", 90, 8, 2, 8, 8, "dup50"),
           ScatterCase("scatter-dup50-scalar-writer", 90, 3, 2, 5, 5, "dup50"),
           ScatterCase("scatter-invalid-rows-dropped", 48, 8, 2, 8, 8, "invalid"),
           ScatterCase("scatter-invalid-rows-dropped-scalar", 48, 3, 2, 6, 7, "invalid"),
           ScatterCase("scatter-feats-misaligned", 40, 8, 2, 8, 8, feats_off=1),
           ScatterCase("scatter-canvas-misaligned", 40, 8, 2, 8, 8, out_off=1),
           ScatterCase("scatter-both-misaligned", 40, 8, 2, 8, 8, "dup2", feats_off=1, out_off=1),
           ScatterCase("scatter-no-pillars", 0, 8, 2, 8, 8)]
    return tuple(cs)


SCATTER_CASES = _scatter_cases()


def scatter_data(c: ScatterCase):
    """(feats [M, C] of small nonzero integers, a different one per element; coords [M, 4] = batch, z, y, x)."""
    rng = np.random.default_rng(_seed(c.id))
    plane = c.ny * c.nx
    feats = (np.arange(c.M * c.C, dtype=np.float32) + 1).reshape(c.M, c.C)
    m_u = c.M - {"dup2": 1, "dup50": 49, "invalid": 8}.get(c.kind, 0)
    cells = rng.choice(c.batch * plane, m_u, replace=False)
    co = np.stack([cells // plane, rng.integers(1, 4, m_u), cells % plane // c.nx, cells % c.nx], 1)
    if c.kind in ("dup2", "dup50"):       # the writers share a cell with one unique row; the input's last row is one
        n = c.M - m_u + 1                 # writers of the cell, the unique row among them
        co = np.concatenate([co[:5], np.repeat(co[5:6], n - 2, 0), co[5:], co[5:6]])
    elif c.kind == "invalid":             # every invalid row aims at a cell an earlier valid row holds
        bad = np.array([[-1, 0, 0, 0], [c.batch, 1, co[0, 2], co[0, 3]], [c.batch + 1, 1, 0, 0],
                        [0, 1, c.ny, 0], [0, 1, 0, c.nx], [1, 1, -1, 0], [1, 1, 0, -1], [-1, 1, co[1, 2], co[1, 3]]])
        co = np.concatenate([co[:m_u // 2], bad[:4], co[m_u // 2:], bad[4:]])
    return feats, co.astype(np.int32).reshape(c.M, 4)


@dataclass(frozen=True)
class MeanCase:
    id: str
    M: int
    P: int
    D: int
    values: str


MEAN_CASES = tuple(MeanCase(f"mean-M{m}-P{p}-D{d}-{v}", m, p, d, v)
                   for m, p, d in ((85, 1, 3), (86, 10, 3), (63, 10, 4), (64, 35, 4), (65, 1, 4), (51, 35, 5), (52, 10, 5),
                                   (1, 10, 4), (300, 35, 5))
                   for v in ("exact", "real"))


def mean_data(c: MeanCase):
    """(voxels, num_points): counts 0 .. P and above; a zero count on an all-zero row (nan) and on a stored row (+inf)."""
    rng = np.random.default_rng(_seed(c.id))
    npv = rng.integers(1, c.P + 1, c.M).astype(np.int32)
    for i, v in ((2, 0), (3, 0), (4, 2 * c.P), (5, c.P)):
        if i < c.M:
            npv[i] = v
    st = np.minimum(npv, c.P)
    if c.M > 3:
        st[3] = 1                      # num_points == 0 on a row that holds a point
    vox = rng.integers(1, 64, (c.M, c.P, c.D)) / 4.0 if c.values == "exact" else rng.uniform(0.5, 70.0, (c.M, c.P, c.D))
    vox = vox.astype(np.float32)
    vox[np.arange(c.P)[None, :] >= st[:, None]] = 0.0
    return vox, npv


# ---- GPU side ------------------------------------------------------------------------------------------------------------
def upload(case, vox, npv, co, prm):
    import torch

    dev = torch.device("cuda")
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         dict(vox=vox, npv=npv, co=co, **{k: v for k, v in prm.items() if v is not None}).items()}
    return t


def _net_args(case, t):
    import ctypes as C

    from paddle3d_amd.ops._common import ptr

    vx, vy, vz, xo, yo, zo = geometry(case)
    return [case.cd, C.c_float(vx), C.c_float(vy), C.c_float(vz), C.c_float(xo), C.c_float(yo), C.c_float(zo),
            ptr(t["w1"]), ptr(t["s1"]), ptr(t["b1"]), case.c1, ptr(t.get("w2")), ptr(t.get("s2")), ptr(t.get("b2")), case.c2]


def launch_path(case, t, path):
    """(status, out [M, C] on the host, pre-filled with SENTINEL) of pd3_pillar_feature_net_path."""
    import torch

    from paddle3d_amd.ops._common import lib, ptr, stream_ptr

    out = torch.full((case.M, case.cout), SENTINEL, dtype=torch.float32, device=t["vox"].device)
    rc = lib().pd3_pillar_feature_net_path(ptr(t["vox"]), ptr(t["npv"]), ptr(t["co"]), case.M, case.P, case.D,
                                           *_net_args(case, t), ptr(out), path, stream_ptr(out.device))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def launch_indexed(case, t, points, span, plist, points_per_frame=None, list_stride=None):
    """(status, out) of pd3_pillar_feature_net_indexed on a hand-made index (None: the arrays' own sizes)."""
    import torch

    from paddle3d_amd.ops._common import lib, ptr, stream_ptr

    dev = t["co"].device
    pts, sp, pl = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (points, span, plist))
    out = torch.full((case.M, case.cout), SENTINEL, dtype=torch.float32, device=dev)
    n = points.shape[1] if points_per_frame is None else points_per_frame
    ls = plist.shape[1] if list_stride is None else list_stride
    rc = lib().pd3_pillar_feature_net_indexed(ptr(pts), n, ptr(sp), ptr(pl), ls, ptr(t["co"]), case.M, case.vper, case.P,
                                              case.D, *_net_args(case, t), ptr(out), stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()
