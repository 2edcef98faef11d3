"""Box sets a detector hands to rotated NMS but independent random draws never produce (a helper module like
tests/conv_lattice.py, not a conftest): near-duplicates, half and quarter turns, axis-aligned contacts, degenerate fields.

Why they matter: two convex quadrilaterals in general position meet in at most 8 vertices, and the reference admits a
corner as "inside" with a 1e-2 margin, so two boxes that nearly coincide give 8 edge crossings plus up to 8 admitted
corners.  box_overlap (csrc/iou3d_geom.hpp) sorts polygons of up to 8 vertices in registers and polygons of 9 ... 16 in
LDS; boxes drawn independently (synth.nms_boxes) reach the second path in about three pairs per million.

Every generator is `f(seed, n, ...) -> float32 [n, 7]` rows (x, y, z, dx, dy, dz, heading), deterministic in its arguments,
built in float64 and cast once.  tests/test_box_families_cpu.py pins on the oracle port what each family is for (vertex
histograms, IoU above 1, no polygon above 16 vertices); the GPU tests compare the kernels on them bit for bit.
"""
from __future__ import annotations

import numpy as np

from paddle3d_amd import synth

NEAR = dict(d_heading=2e-3, d_centre=5e-3, d_extent=8e-3)
WIDE = dict(d_heading=3e-2, d_centre=2e-2, d_extent=2e-2)


def parents(seed, k=1):
    """k general-position boxes of synth.nms_boxes, float64 [k, 7]: what the clusters are built around."""
    return synth.nms_boxes(seed, n=k)[0].astype(np.float64)


def _jitter(rng, parent, n, d_heading, d_centre, d_extent):
    b = np.tile(np.asarray(parent, np.float64).reshape(1, 7), (n, 1))
    b[:, 6] += rng.uniform(-d_heading, d_heading, n)
    b[:, :2] += rng.uniform(-d_centre, d_centre, (n, 2))
    b[:, 3:5] += rng.uniform(-d_extent, d_extent, (n, 2))
    return b


def _cluster64(rng, parent, n, spread, quarter=False):
    b = _jitter(rng, parent, n, **spread)
    if quarter:  # a quarter turn with the extents swapped is the same rectangle
        odd = rng.random(n) < 0.5
        b[odd, 6] += np.pi / 2
        b[odd, 3], b[odd, 4] = b[odd, 4].copy(), b[odd, 3].copy()
    b[rng.random(n) < 0.5, 6] += np.pi  # the same box seen with heading theta and theta + pi
    b[7::7] = b[0]  # exact copies
    return b


def near_duplicate_cluster(seed, n, parent=None):
    """One parent n times: heading U(+-2e-3), centre U(+-5e-3), extents U(+-8e-3), a random half turned by pi, every
    7th box an exact copy of box 0."""
    rng = np.random.default_rng([seed, 1])
    return _cluster64(rng, parents(seed)[0] if parent is None else parent, n, NEAR).astype(np.float32)


def wide_cluster(seed, n, parent=None):
    """The same recipe with heading +-3e-2, centre and extents +-2e-2: polygons of 4 ... 16 vertices, IoU spread over
    (0.9, 1], so that the keep list depends on the threshold."""
    rng = np.random.default_rng([seed, 2])
    return _cluster64(rng, parents(seed)[0] if parent is None else parent, n, WIDE).astype(np.float32)


def quarter_turn(seed, n, parent=None):
    """The near-duplicate cluster with a random half of the boxes stated as heading + pi/2 with dx and dy swapped."""
    rng = np.random.default_rng([seed, 3])
    return _cluster64(rng, parents(seed)[0] if parent is None else parent, n, NEAR, quarter=True).astype(np.float32)


def _lattice_cell(x0, y0, dx, dy, sq):
    """Contacts around one dx x dy box at (x0, y0), headings exactly 0, pi/2, pi, -pi/2 (as float32 states them)."""
    h = [0.0, float(np.float32(np.pi / 2)), float(np.float32(np.pi)), float(np.float32(-np.pi / 2))]
    z, dz = -1.0, 1.5
    return [
        [x0, y0, z, dx, dy, dz, h[0]],                      # the box
        [x0, y0, z, dy, dx, dz, h[1]],                      # the same rectangle, a quarter turn
        [x0, y0, z, dx, dy, dz, h[2]],                      # half a turn
        [x0, y0, z, dy, dx, dz, h[3]],                      # three quarters
        [x0 + dx, y0, z, dx, dy, dz, h[0]],                 # shares the edge x = x0 + dx / 2
        [x0, y0 + dy, z, dx, dy, dz, h[2]],                 # shares the edge y = y0 + dy / 2
        [x0 + dx, y0 + dy, z, dy, dx, dz, h[1]],            # shares one corner
        [x0 - dx, y0 - dy, z, dx, dy, dz, h[0]],            # the opposite corner
        [x0, y0, z, dx / 2, dy / 2, dz, h[0]],              # strictly inside: 4 corners, no crossing
        [x0 + dx / 8, y0, z, dy / 4, dx / 4, dz, h[3]],     # inside, turned
        [x0 + dx / 2, y0, z, dx, dy, dz, h[0]],             # half overlap, collinear edges
        [x0, y0 + 2 * dy, z, sq, sq, dz, h[0]],             # a square ...
        [x0, y0 + 2 * dy, z, sq, sq, dz, float(np.float32(np.pi / 4))],  # ... and itself turned by pi/4: 8 crossings
        [x0, y0 + 2 * dy, z, sq, sq, dz, float(np.float32(-np.pi / 4))],
    ]


def axis_aligned_lattice(seed, n):
    """Cells of boxes that share an edge, share a corner, coincide after a quarter / half turn, lie strictly inside one
    another, and squares turned by pi/4; extents exactly representable in one cell, not in the next; shuffled."""
    rng = np.random.default_rng([seed, 4])
    rows = []
    c = 0
    while len(rows) < n:
        exact = c % 2 == 0
        dx, dy, sq = (4.0, 2.0, 2.0) if exact else tuple(rng.uniform([3.5, 1.5, 1.0], [5.0, 2.5, 3.0]))
        x0, y0 = (16.0 * c, 0.0) if exact else (16.0 * c + rng.uniform(-1, 1), rng.uniform(-30, 30))
        rows += _lattice_cell(x0, y0, dx, dy, sq)
        c += 1
    b = np.asarray(rows, np.float64)
    return b[rng.permutation(len(b))[:n]].astype(np.float32)


def specials(seed, n):
    """Degenerate field values among near-duplicates of one ordinary box: dx = 0, dx = dy = 0, negative dx, NaN in x,
    inf in dx, heading 100 rad, a near-duplicate pair centred at (1e4, 1e4).  n below the number of specials takes a
    seeded subset; the rest of a larger set is the near-duplicate cluster of the ordinary box."""
    rng = np.random.default_rng([seed, 5])
    p = np.array([1.25, -2.5, -1.0, 4.2, 1.9, 1.6, 0.3])

    def var(**kw):
        q = p.copy()
        for k, v in kw.items():
            q[dict(x=0, y=1, dx=3, dy=4, h=6)[k]] = v
        return q

    far = var(x=1e4, y=1e4)
    rows = [p, var(dx=0.0), var(dx=0.0, dy=0.0), var(dx=-4.2), var(x=np.nan), var(dx=np.inf), var(h=100.0),
            var(h=100.0 + np.pi), far, _jitter(rng, far, 1, **NEAR)[0], var(dy=0.0, h=0.3 + np.pi / 2),
            var(dx=-4.2, dy=-1.9)]
    b = np.asarray(rows, np.float64)
    b = b[rng.permutation(len(b))[:n]]
    if n > len(b):
        b = np.concatenate([b, _cluster64(rng, p, n - len(b), NEAR)])
        b = b[rng.permutation(n)]
    return b.astype(np.float32)


def mixture(seed, n, k=4, parent_seed=None):
    """k clusters (near-duplicate, wide, quarter turn in turn; about n / 2 boxes in all) around general-position parents,
    scattered among general-position boxes of synth.nms_boxes and shuffled: several kept boxes per set."""
    rng = np.random.default_rng([seed, 6])
    ps = parents(seed if parent_seed is None else parent_seed, k)
    m = max(1, n // (2 * k))
    kinds = ((NEAR, False), (WIDE, False), (NEAR, True))
    parts = [_cluster64(rng, ps[c], m, *kinds[c % 3]) for c in range(k)]
    rest = n - m * k
    if rest > 0:
        parts.append(synth.nms_boxes(seed + 7919, n=rest)[0].astype(np.float64))
    b = np.concatenate(parts)[:n]
    return b[rng.permutation(n)].astype(np.float32)


CLUSTERS = {"near": near_duplicate_cluster, "wide": wide_cluster, "quarter": quarter_turn}
FAMILIES = dict(CLUSTERS, lattice=axis_aligned_lattice, specials=specials, mixture=mixture)
# The seeds the tests draw every family with.  What a cluster gives depends on its parent (a 0.7 m box keeps more corners
# within the 1e-2 margin than a 7 m one): tests/test_box_families_cpu.py holds these seeds to what the families are for.
SEEDS = {"near": (0, 2, 15), "wide": (9, 8, 6), "quarter": (7, 3, 6), "lattice": (0, 1), "specials": (0, 1, 2),
         "mixture": (0, 1, 2)}

# ---- the exact sets the GPU tests draw (tests/test_box_families_cpu.py checks the same ones on the port) ----------------
NMS_SIZES = (2, 63, 64, 65, 128, 129, 300)       # around the 64-box tile of nms_mask_kernel, several tiles
POOL_SIZES = (64, 91, 92, 128)                   # n (n - 1) / 2 candidates around the 4096-pair pool of nms_pairs_kernel
PAIRWISE_SIZES = ((1, 1), (15, 17), (16, 16), (17, 15), (64, 65), (129, 129))  # around pairwise_kernel's 16 x 16 block
PAIRWISE = (("near", "near"), ("near", "wide"), ("wide", "quarter"), ("quarter", "near"), ("lattice", "lattice"),
            ("specials", "specials"), ("mixture", "mixture"))


def pairwise_case(fam_a, fam_b, num_a, num_b):
    """(a [num_a, 7], b [num_b, 7]) drawn with different seeds around the SAME parents, so that the matrix is full of
    near-coincident pairs rather than of exact copies."""
    sa, sb = SEEDS[fam_a][0], SEEDS[fam_b][1]
    if fam_a in CLUSTERS:
        p = parents(sa)[0]
        return CLUSTERS[fam_a](sa, num_a, parent=p), CLUSTERS[fam_b](sb, num_b, parent=p)
    if fam_a == "mixture":
        return mixture(sa, num_a), mixture(sb, num_b, parent_seed=sa)
    return FAMILIES[fam_a](sa, num_a), FAMILIES[fam_b](sb, num_b)
