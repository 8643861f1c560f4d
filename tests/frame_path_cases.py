"""TEST INFRASTRUCTURE: the inputs that the CPU and the GPU tests of the frame path share (csrc/frames.hip, normals.hip, lidar_depth.hip,
post.hip; tests/test_frame_path_cpu.py, tests/test_frame_path_kernels_gpu.py).  Every case is a dict of numpy arrays that names the
clause it aims at (`clause`); test_frame_path_cpu.py asserts with the definitions alone that it reaches that clause, so that a case
which stops reaching it fails on the CPU.  Nothing here runs a kernel; every case is made once per process and is read-only.  Two
frames (or images) throughout, and the two differ.

Spoiled table entries (s0 = -1, s1 = n_src) send an unchecked kernel one source row and one source pixel past either end of the
source at the most; the sources of those cases are at most 5 x 11 x 3 bytes or floats, so that distance is at most (11 + 1) 3 = 36
elements, inside the 256 elements in front of and the 264 behind every sentinel_buffers.Flat view: a missing clamp shows as a wrong
result, never as a fault."""
import functools

import numpy as np

import frame_path_raw_reference as raw
import splat_cases as pc
import splat_reference as sr
from scene_cases import ALIGNED_SIZE, FRAMES, PIXEL_CLAUSE, PIXEL_SIZES, SKY, _frozen, lanes, start_sums  # noqa: F401 (shared with the tests)

F, D = np.float32, np.float64

# ------------------------------------------------------------------------------------------------ frames.hip and normal_stream
SEGMENT = 512                                                  # output pixels of a row that a workgroup of 128 lanes x 4 pixels owns
# output width -> (source (H0, W0), output (H, W)): a non-integer shrink (11 -> 4, 5 -> 2), enlargements, and rows both ways
RESIZE_SHAPES = {4: ((5, 11), (2, 4)), 5: ((2, 3), (3, 5)), 516: ((3, 5), (2, 516)), 513: ((4, 7), (3, 513))}
WIDTH_CLAUSE = {4: "W % 4 == 0: the wide form, one lane", 5: "W % 4 != 0: the bounded form, the second lane holds one pixel",
                516: "the wide form, the second row segment holds one lane", 513: "the bounded form, the second row segment holds one pixel"}
U8_MODES = (("linear", raw.LINEAR, 1, False), ("linear", raw.LINEAR, 3, False), ("nearest", raw.NEAREST, 1, False), ("nearest", raw.NEAREST, 3, False),
            ("palette", raw.LINEAR, 3, True))
PALETTE_IDS = (0, 20, 21, 255)
DEPTH_CORNERS = (100.0, 0.0, np.nan, 150.0)                    # frame 0's first and last pixel, frame 1's


def row_lanes(W):
    """(row segments, lanes of the last segment, pixels of the last lane) of a row of W output pixels."""
    segs = -(-W // SEGMENT)
    last = W - (segs - 1) * SEGMENT
    return segs, -(-last // 4), last - (-(-last // 4) - 1) * 4


@functools.lru_cache(maxsize=None)
def resize_case(width):
    """What every resize entry reads at one output width: bytes of one and three channels, class ids, metres and normals of two
    frames, and the three kinds of table, whole and spoiled."""
    (H0, W0), (H, W) = RESIZE_SHAPES[width]
    rng = np.random.default_rng(width)
    ids = rng.integers(0, 21, (FRAMES, H0, W0)).astype(np.uint8)
    ids[0].reshape(-1)[:4] = PALETTE_IDS
    ids[1].reshape(-1)[-4:] = PALETTE_IDS
    metres = rng.uniform(5.0, 95.0, (FRAMES, H0, W0)).astype(F)                          # frame 1 in range; frame 0 negative on the left, above 100 m on the right
    metres[0, :, :(W0 + 1) // 2], metres[0, :, (W0 + 1) // 2:] = rng.uniform(-20.0, -1.0, (H0, (W0 + 1) // 2)), rng.uniform(101.0, 140.0, (H0, W0 // 2))
    metres[0, 0, 0], metres[0, -1, -1], metres[1, 0, 0], metres[1, -1, -1] = DEPTH_CORNERS
    tables = {k: (make(W0, W), make(H0, H)) for k, make in (("u8", raw.table_u8), ("nearest", raw.table_nearest), ("f32", raw.table_f32))}
    bad = {k: (raw.spoiled(x, W0), raw.spoiled(y, H0)) for k, (x, y) in tables.items()}
    return _frozen(dict(name=f"{H0}x{W0} -> {H}x{W}", clause=WIDTH_CLAUSE[width], H0=H0, W0=W0, H=H, W=W,
                        u8_1=rng.integers(0, 256, (FRAMES, H0, W0, 1)).astype(np.uint8), u8_3=rng.integers(0, 256, (FRAMES, H0, W0, 3)).astype(np.uint8),
                        ids=ids, metres=metres, f32=rng.uniform(-3.0, 3.0, (FRAMES, H0, W0)).astype(F),
                        normals=rng.uniform(-1.0, 1.0, (FRAMES, H0, W0, 3)).astype(F), tables=tables, spoiled=bad, norm=raw.norm_table()))


# (name, what is moved: strides as functions of HW and the element offsets of dst (floats) and u8_out (bytes), the clause)
# Two streams of four frames of three planes; the call writes frames 1 and 2 of stream 1.  Each falsified layout keeps every other term
# of the wide predicate true: the placed base dst + stream_stride + frame_stride stays a multiple of four floats.
STREAM_LAYOUTS = {
    "planar": dict(cs=lambda hw: 4 * hw, fs=lambda hw: hw, ss=lambda hw: 12 * hw, dst=0, u8=0, clause="every term true: the wide form where W % 4 == 0"),
    "dst one float off": dict(cs=lambda hw: 4 * hw, fs=lambda hw: hw, ss=lambda hw: 12 * hw, dst=1, u8=0, clause="aligned16(dst + slab ss + frame0 fs) false alone"),
    "channel_stride % 4 == 1": dict(cs=lambda hw: 4 * hw + 1, fs=lambda hw: hw, ss=lambda hw: 12 * hw + 4, dst=0, u8=0, clause="(channel_stride & 3) == 0 false alone"),
    "frame_stride % 4 == 2": dict(cs=lambda hw: 4 * hw + 8, fs=lambda hw: hw + 2, ss=lambda hw: 12 * hw + 26, dst=0, u8=0, clause="(frame_stride & 3) == 0 false alone"),
    "u8_out one byte off": dict(cs=lambda hw: 4 * hw, fs=lambda hw: hw, ss=lambda hw: 12 * hw, dst=0, u8=1, clause="aligned4(u8_out) false alone"),
    "frames outermost": dict(cs=lambda hw: hw, fs=lambda hw: 3 * hw, ss=lambda hw: 12 * hw, dst=0, u8=0, clause="channel_stride = H W, frame_stride = 3 H W: admitted, wide"),
}
SLAB, FRAME0 = 1, 1


def stream_layout(name, H, W):
    """-> dict(ss, cs, fs, n (floats of the destination: two streams), dst, u8 (element offsets), terms (the wide predicate's terms
    that do not depend on the allocation))."""
    lay, hw = STREAM_LAYOUTS[name], H * W
    ss, cs, fs = lay["ss"](hw), lay["cs"](hw), lay["fs"](hw)
    return dict(name=name, clause=lay["clause"], ss=ss, cs=cs, fs=fs, n=2 * ss, dst=lay["dst"], u8=lay["u8"],
                terms=dict(W=W % 4 == 0, dst=(lay["dst"] + SLAB * ss + FRAME0 * fs) % 4 == 0, cs=cs % 4 == 0, fs=fs % 4 == 0, u8=lay["u8"] % 4 == 0))


# ------------------------------------------------------------------------------------------------ mudg_depth_normals
MIN_DEPTH, MAX_DEPTH, REL_STEP = 0.5, 80.0, 0.25
NORMAL_DEPTHS = (MIN_DEPTH, MAX_DEPTH, np.nan, np.inf, -3.0)   # exactly on either bound, not a number, infinite, negative: not usable
LOW_WORD_SKY = SKY + 2 ** 32


@functools.lru_cache(maxsize=None)
def normals_case(hw):
    """Depths about 10 m (every step inside the limit) with a fifth of the pixels empty, so that pixels with any set of neighbours
    occur; the two frames meet in rows chosen against a neighbour taken across the frame boundary: (frame 1, row 0, column 1) has an
    empty pixel below it and (frame 0, last row, column 2) an empty one above it, so neither has a vertical neighbour, while the
    row on the other side of the boundary is full.  Where there is room: the depths that are not usable, a label whose low word alone
    is sky's, and z = 8 between 6 and 10 under r = 0.25 (a step of exactly r z counts) with 9 above it."""
    H, W = hw
    rng = np.random.default_rng(31 * H + W)
    depth = (10.0 + rng.uniform(-0.5, 0.5, (FRAMES, H, W)) + np.arange(FRAMES)[:, None, None] * 0.25).astype(F)
    depth[rng.random(depth.shape) < 0.2] = 0
    labels = rng.integers(0, 19, (FRAMES, H, W)).astype(np.int64)
    labels[labels == SKY] = 3
    labels[rng.random(labels.shape) < 0.05] = SKY
    lo, hi = depth[0, H - 1], depth[1, 0]                                                # the two rows that meet
    lo[:], hi[:] = F(10.25), F(10.5)
    labels[0, H - 1], labels[1, 0] = 3, 3
    labels[0, 0, 3], labels[1, H - 1, 0] = SKY, SKY
    special = {}
    if H >= 3:
        depth[1, 1, 1], depth[0, H - 2, 2] = 0, 0
        special["boundary"] = ((1, 0, 1), (0, H - 1, 2))
    if H * W >= 35:
        f = 0
        for k, v in enumerate(NORMAL_DEPTHS):
            depth[f, 1 + k % (H - 2), 3 + k // (H - 2)] = v
            labels[f, 1 + k % (H - 2), 3 + k // (H - 2)] = 3
        depth[1, 1:4, 3:6] = F([[10.0, 9.0, 10.0], [6.0, 8.0, 10.0], [10.0, 0.0, 10.0]])
        labels[1, 1:4, 3:6] = 3
        labels[1, 2, 6] = LOW_WORD_SKY
        depth[1, 2, 6] = F(10.0)
        special.update(step=(1, 2, 4), low_word=(1, 2, 6))
    table = np.array([[0.9 * W, 1.1 * W, 0.5 * W, 0.45 * H], [1.2 * W, 1.0 * W, 0.4 * W, 0.5 * H]], dtype=D)
    return _frozen(dict(name=f"{H}x{W}", clause=PIXEL_CLAUSE[hw] + "; a neighbour is in the frame", H=H, W=W, depth=depth, labels=labels, table=table, special=special))


# ------------------------------------------------------------------------------------------------ mudg_metric_normals
SCORE_PIXELS, SCORE_GROUPS = 8192, 32                           # csrc/normals.hip
SCORE_SIZES = PIXEL_SIZES + ((2, 6), (43, 192), (91, 91))
SCORE_CLAUSE = {(2, 6): "hw % 4 == 0 with W % 4 != 0: the wide form", (43, 192): "8256 pixels: two workgroups a frame in the wide form, five sweeps",
                (91, 91): "8281 pixels: two workgroups a frame in the one-pixel form, seventeen sweeps"}
VALID_BYTES = (0, 1, 2, 255)


def score_launch(hw):
    """(pixels a lane owns, workgroups a frame, sweeps of the stride loop) of metric_normals at H x W with aligned bases."""
    n = hw[0] * hw[1]
    px = 4 if n % 4 == 0 else 1
    groups = min(-(-n // SCORE_PIXELS), SCORE_GROUPS)
    return px, groups, -(-n // (groups * 256 * px))


def _beyond_one(rng, sign):
    """(u, g): bytes and an fp32 normal (anti)parallel to p = 2 u - 255 whose cosine leaves [-1, 1] before the clamp."""
    import normals_reference as nm
    for _ in range(4000):
        u = rng.integers(0, 256, 3).astype(np.uint8)
        g = (F(sign) * (2 * u.astype(np.int64) - 255).astype(F) * F(rng.uniform(0.001, 0.01))).astype(F)
        c, _ = nm.cosines(u, g)
        if sign * c > 1.0:
            return u, g
    raise AssertionError("no cosine beyond one found")


@functools.lru_cache(maxsize=None)
def score_case(hw):
    """Bytes of a generated stream, true normals and validity bytes of two frames.  The first and the last pixel of each frame count.
    Where there is room, frame 0 holds the special pixels; at 5 x 7 every pixel of frame 1 falls in bin 0."""
    H, W = hw
    n = H * W
    rng = np.random.default_rng(7 * H + 3 * W)
    pred = rng.integers(0, 256, (FRAMES, n, 3)).astype(np.uint8)
    gt = rng.normal(0.0, 1.0, (FRAMES, n, 3))
    gt = (gt / np.linalg.norm(gt, axis=-1, keepdims=True)).astype(F)
    valid = np.array(VALID_BYTES, dtype=np.uint8)[rng.integers(0, 4, (FRAMES, n))]
    valid[:, 0], valid[:, n - 1] = 1, 255
    special = {}
    if n >= 35:
        up, gp = _beyond_one(rng, 1)
        um, gm = _beyond_one(rng, -1)
        rows = ((np.uint8([1, 2, 3]), F([0, 0, 0])), (np.uint8([1, 2, 3]), F([np.nan, 0, 1])), (np.uint8([1, 2, 3]), F([np.inf, 0, 1])), (up, gp), (um, gm),
                (np.uint8([128, 128, 128]), F([1, -1, 0])), (np.uint8([255, 255, 255]), F([1, 1, 1])), (np.uint8([0, 0, 0]), F([1, 1, 1])))
        for k, (u, g) in enumerate(rows):
            pred[0, 2 + k], gt[0, 2 + k], valid[0, 2 + k] = u, g, 1
        special = dict(zero=2, nan=3, inf=4, above=5, below=6, right_angle=7, plus_one=8, minus_one=9)
    if hw == (5, 7):
        pred[1], gt[1] = 255, F(1.0)
    shape = (FRAMES, H, W)
    clause = SCORE_CLAUSE.get(hw) or PIXEL_CLAUSE[hw].replace("W % 4", "hw % 4")
    return _frozen(dict(name=f"{H}x{W}", clause=clause, H=H, W=W, pred=pred.reshape(*shape, 3), gt=gt.reshape(*shape, 3), valid=valid.reshape(shape), special=special))


# ------------------------------------------------------------------------------------------------ mudg_lidar_splat_visible
CAM = pc.CAM
SPLAT_IMAGES = ((1, 1), (5, 3), (17, 65), (37, 53))
SPLAT_CLOUDS = (1, 255, 256, 257)                               # candidates: a workgroup owns 256
NEAR_KEY = int(raw.make_keys(0.25, 7))                          # padding of the occluder keys: a near depth
VISIBLE_VARIANTS = ("reach 4", "reach 1", "reach 16", "rel_keep 1", "no occluders")


def start_keys(H, W, seed):
    """Keys to draw on top of: a third empty, a third nearer than any candidate (0.3 m), a third farther (190 m)."""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 3, (H, W))
    if H * W >= 3:
        kind.reshape(-1)[:3] = (0, 1, 2)
    keys = raw.make_keys(np.where(kind == 1, F(0.3), F(190.0)), rng.integers(0, 4000, (H, W)))
    return np.where(kind == 0, sr.EMPTY, keys), kind


@functools.lru_cache(maxsize=None)
def visible_case(k):
    """Image k of SPLAT_IMAGES with cloud k of SPLAT_CLOUDS as one segment, the occluder keys drawn from the same candidates at size 1."""
    (H, W), n = SPLAT_IMAGES[k], SPLAT_CLOUDS[k]
    rng = np.random.default_rng(500 + k)
    xyz, _ = pc._cloud(rng, n, H, W, 2.0)
    xyz[-1] = pc._pixels_to_points([0.5 * W], [0.5 * H], [0.4])[0]                       # the last lane's point is near: it shows
    Z = sr.splat_keys(xyz, pc.EYE, CAM, 1.0, H, W)
    keys, kind = start_keys(H, W, k)
    last = {1: "holds one lane", 255: "lacks one lane", 256: "is full", 257: "holds one lane (the second)"}[n]
    return _frozen(dict(name=f"{H}x{W}, {n} candidates", clause=f"idx < total: the last workgroup {last}; the minimum with a nearer, a farther and an empty key",
                        H=H, W=W, xyz=xyz, ids=None, segments=np.array([[0, n]], dtype=np.int64), mats=pc.EYE[None], occluders=Z, keys=keys, kind=kind, size=2.0))


EIGHT_RUNS = ((400, 60), (0, 70), (130, 120), (590, 5), (300, 2), (599, 1), (250, 30), (310, 12))    # candidates 255 .. 256 are one run: it straddles 256


@functools.lru_cache(maxsize=None)
def segments_case(kind):
    """600 points on 17 x 65 with ids over three matrices (the first eight ids out of range).  "eight": EIGHT_RUNS, 300 candidates;
    "twice": the same run of 50 points as two segments."""
    H, W = 17, 65
    rng = np.random.default_rng(77)
    xyz, _ = pc._cloud(rng, 600, H, W, 2.0)
    ids = rng.integers(0, 3, 600).astype(np.int32)
    mats = np.stack([pc.EYE, pc.shifted(2.0, 0.0, 0.0), pc.shifted(0.0, 3.0, 0.0)])
    runs = EIGHT_RUNS if kind == "eight" else ((400, 50), (400, 50))
    ids[400:408] = (-1, 3, pc.INT32_MIN, pc.INT32_MAX, -7, 1000, 0, 2)
    xyz[400:408] = pc._pixels_to_points(8.5 + 6.0 * np.arange(8), np.full(8, 8.5), np.full(8, 0.3))    # in view and nearest at every matrix
    at = raw.candidate_points(runs)
    Z = sr.splat_keys(xyz[at], mats, CAM, 1.0, H, W, ids=ids[at])
    keys, kindmap = start_keys(H, W, 9)
    clause = ("seg.start[s + 1] <= idx: eight runs, one across the workgroup boundary; the id clamp; ids read at the point's place" if kind == "eight"
              else "two runs that name the same points: equal depths, the lower candidate number wins")
    return _frozen(dict(name=f"{kind} segments", clause=clause, H=H, W=W, xyz=xyz, ids=ids, segments=np.array(runs, dtype=np.int64), mats=mats, occluders=Z,
                        keys=keys, kind=kindmap, size=2.0))


# The hand-made occluders: probes at depth 10 m on 37 x 53, point size 2, reach 4, each alone in its neighbourhood.
# (home (row, column), occluders as (d_row, d_column, depth), hidden?, what it shows); "limit" stands for fp32(10 fp32(0.95)).
PROBE_Z, PROBE_REACH, PROBE_KEEP = 10.0, 4, 0.95
LIMIT = F(PROBE_Z) * F(PROBE_KEEP)
PROBES = (
    ((6, 6), ((0, 4, 5.0), (0, -4, 5.0)), True, "occluders at exactly reach on both sides: hidden"),
    ((6, 17), ((0, 5, 5.0), (0, -5, 5.0)), False, "at reach + 1: not hidden"),
    ((6, 28), ((0, 2, 5.0),), False, "one side only: not hidden"),
    ((6, 39), ((0, 1, 5.0), (0, -3, 5.0)), True, "the row alone"),
    ((18, 6), ((1, 0, 5.0), (-3, 0, 5.0)), True, "the column alone"),
    ((18, 17), ((1, 1, 5.0), (-3, -3, 5.0)), True, "the diagonal (1, 1) alone"),
    ((18, 28), ((1, -1, 5.0), (-3, 3, 5.0)), True, "the diagonal (1, -1) alone"),
    ((18, 39), ((0, 2, float(LIMIT)), (0, -2, float(LIMIT))), False, "a depth of exactly zc rel_keep: not nearer"),
    ((30, 6), ((0, 2, 5.0), (-2, 0, 5.0)), False, "one side each of two directions: not hidden"),
    ((30, 17), ((0, 2, float(np.nextafter(LIMIT, F(0)))), (0, -2, 5.0)), True, "a depth one step below the limit: nearer"),
    ((1, 1), ((0, 1, 5.0), (0, -1, 5.0)), True, "lines that leave the image at a corner"),
    ((35, 51), ((1, 1, 5.0), (-1, -1, 5.0)), True, "lines that leave the image at the far corner"),
    ((30, -1), ((0, 1, 5.0), (0, 2, 5.0), (1, 1, 5.0), (-1, 1, 5.0)), False, "a home pixel outside the image: one side of every line is outside, the sprite still lands"),
)


@functools.lru_cache(maxsize=None)
def probe_case():
    H, W = 37, 53
    homes = np.array([p[0] for p in PROBES])
    u = np.where(homes[:, 1] < 0, -0.4, homes[:, 1] + 0.5)
    xyz = pc._pixels_to_points(u, homes[:, 0] + 0.5, np.full(len(PROBES), PROBE_Z))
    Z = np.full((H, W), sr.EMPTY, dtype=np.uint64)
    for (j, i), occ, _, _ in PROBES:
        for dj, di, z in occ:
            assert Z[j + dj, i + di] == sr.EMPTY
            Z[j + dj, i + di] = raw.make_keys(F(z), 123)
    keys = np.full((H, W), sr.EMPTY, dtype=np.uint64)
    return _frozen(dict(name="hand-made occluders", clause="nearer(): in the image, not empty, depth < limit; hidden: both sides of one direction within reach",
                        H=H, W=W, xyz=xyz, ids=None, segments=np.array([[0, len(PROBES)]], dtype=np.int64), mats=pc.EYE[None], occluders=Z, keys=keys, size=2.0,
                        want_hidden=np.array([p[2] for p in PROBES])))


# ------------------------------------------------------------------------------------------------ mudg_lidar_depth_resolve
RESOLVE_PIXELS = (1, 255, 256, 257)
ODD_WORDS = (0x7FC00001, 0x80000000, 0x7F800000, 0x00000001, 0xFFFFFFFE, 0xFFFFFFFF)      # a NaN with a payload, -0, inf, a denormal, ...


@functools.lru_cache(maxsize=None)
def resolve_case(pixels, full=False):
    """Keys of `pixels` pixels: empty ones, ordinary depths and high words that are no ordinary depth (all of them with a low word
    that is not all ones, so none is empty); full: no empty key.  Occluder keys of any content."""
    rng = np.random.default_rng(pixels)
    keys = raw.make_keys(rng.uniform(0.1, 190.0, pixels).astype(F), rng.integers(0, 1 << 32, pixels))
    if not full:
        keys[rng.random(pixels) < 0.4] = sr.EMPTY
    if pixels > 1:
        odd = np.array([(w << 32) | 5 for w in ODD_WORDS], dtype=np.uint64)
        keys[1:1 + len(odd)] = odd
        keys[-1] = raw.make_keys(F(17.25), 3)
        if not full:
            keys[0] = sr.EMPTY
    else:
        keys[0] = sr.EMPTY if not full else np.uint64((ODD_WORDS[0] << 32) | 5)
    occluders = raw.make_keys(rng.uniform(0.1, 190.0, pixels).astype(F), rng.integers(0, 1 << 32, pixels))
    return _frozen(dict(name=f"{pixels} pixels, {'full' if full else 'with empty keys'}", clause="i < total in the last workgroup; the high word bit for bit; both key images emptied",
                        keys=keys, occluders=occluders))


# ------------------------------------------------------------------------------------------------ mudg_depth_complete
COMPLETE_SIZES = ((1, 1), (1, 40), (40, 1), (31, 33), (33, 65), (3, 300))
COMPLETE_CLAUSE = {(1, 1): "one pixel: every neighbourhood is the border", (1, 40): "one row, two tiles", (40, 1): "one column, two tiles",
                   (31, 33): "a tile one row short and a second one column wide; the frame boundary", (33, 65): "2 x 3 tiles, the last ones one row / column wide",
                   (3, 300): "the row pass's seam: columns 256 .. 299 belong to the second workgroup"}
COMPLETE_M = 100.0
COMPLETE_SPECIAL = (np.nan, np.inf, -4.0, 0.05, 0.1, 99.95, 150.0)                        # all of them empty after step 1
SEAM_COLUMN = 245                                                                        # steps 2 - 4 carry a value 5 columns: to 250
STALE = 0x42                                                                             # as fp32 48.56.. (filled), as a stage nonzero


@functools.lru_cache(maxsize=None)
def complete_case(hw):
    """Sparse metres of two frames and their labels.  31 x 33: frame 0's last three rows are full and frame 1's first ten are empty.
    3 x 300: frame 0 holds one value, at (1, SEAM_COLUMN); frame 1 one at (2, 5)."""
    H, W = hw
    rng = np.random.default_rng(H * 1000 + W)
    depth = np.where(rng.random((FRAMES, H, W)) < 0.08, rng.uniform(1.0, 95.0, (FRAMES, H, W)), 0.0).astype(F)
    if H * W >= 40:
        depth.reshape(FRAMES, -1)[:, 3:3 + len(COMPLETE_SPECIAL)] = COMPLETE_SPECIAL
        depth[0].reshape(-1)[-1], depth[1].reshape(-1)[0] = 30.0, 60.0
    else:
        depth[:, 0, 0] = (30.0, 60.0)
    if hw == (31, 33):
        depth[0, -3:], depth[1, :10] = rng.uniform(20.0, 40.0, (3, W)).astype(F), 0
        depth[0, -1, -1] = 30.0
    if hw == (3, 300):
        depth[:] = 0
        depth[0, 1, SEAM_COLUMN], depth[1, 2, 5] = 30.0, 60.0
    labels = rng.integers(0, 19, (FRAMES, H, W)).astype(np.int64)
    labels[labels == SKY] = 3
    labels[rng.random(labels.shape) < 0.1] = SKY
    labels[0, 0, 0], labels[1, -1, -1] = SKY + 2 ** 32, SKY
    return _frozen(dict(name=f"{H}x{W}", clause=COMPLETE_CLAUSE[hw], H=H, W=W, depth=depth, labels=labels))


@functools.lru_cache(maxsize=None)
def complete_want(hw, extrapolate, labelled):
    """The definition's (out, source) of a case: computed once, shared by the tests."""
    c = complete_case(hw)
    out, source = raw.depth_complete(c["depth"], c["labels"] if labelled else None, SKY, COMPLETE_M, extrapolate)
    out.setflags(write=False), source.setflags(write=False)
    return out, source


# ------------------------------------------------------------------------------------------------ post.hip
def unit_values():
    """Every preimage x = 2 k / 255 - 1 of a byte with its fp32 neighbours on either side, -1 and 1, values beyond both ends, the
    infinities and NaN."""
    k = np.arange(256, dtype=D)
    x = (2.0 * k / 255.0 - 1.0).astype(F)
    return np.concatenate([np.nextafter(x, F(-2)), x, np.nextafter(x, F(2)), F([-1, 1, -1.5, 1.5, -1e30, 1e30, -np.inf, np.inf, np.nan, 0.0, -0.0])]).astype(F)


def sheet_values(clamp, rescale):
    """The values of a sheet under one setting, only those whose byte the header defines (-1 < the product < 256).  Under the
    rescale: all of unit_values with the clamp, those in [-1, 1] without.  Without the rescale the bytes change at k / 255: the image
    (x + 1) / 2 in [0, 1] of those, and with the clamp what lies above 1 (what lies below 0, NaN included, has no byte)."""
    v = unit_values()
    if clamp and rescale:
        return v
    inside = v[np.isfinite(v) & (v >= -1) & (v <= 1)]
    if rescale:
        return inside
    half = ((inside + F(1)) / F(2)).astype(F)
    return np.concatenate([half, F([1.5, 1e30, np.inf, np.nextafter(F(1), F(2))])]).astype(F) if clamp else half


def filled(values, shape, roll):
    """`shape` filled by cycling through `values` from `roll` on: neighbouring frames hold different values."""
    n = int(np.prod(shape))
    return np.resize(np.roll(values, -roll), n).reshape(shape).astype(values.dtype)


U8_HW = (1, 255, 257)
SHEET_SIZES = ((3, 4), (5, 7), (9, 120))
SHEET_SETTINGS = ((1, 1), (1, 0), (0, 1), (0, 0))               # (clamp, rescale)
POST_PIXELS = (1, 255, 256, 257)
TRIPLES = ((0, 0, 0), (0, 0, 1), (255, 255, 255))


@functools.lru_cache(maxsize=None)
def u8_video(C, HW):
    shape = (2, C, 2, HW)
    v = filled(unit_values(), shape, 5 * HW)
    if HW == 1:
        v.reshape(-1)[:] = np.resize(F([np.nan, np.inf, -np.inf, -1, 1, -1.5, 1.5, 0.0, 2 / 255 - 1, 0.5, -0.25, 1e30]), v.size)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def sheet_video(C, hw, clamp, rescale):
    v = filled(sheet_values(clamp, rescale), (2, C, 2) + hw, 7 * hw[1])
    if clamp:                                                                            # what only the clamp makes a byte of, in every sample
        beyond = F([np.nan, np.inf, -np.inf, -1.5, 1.5, 1e30]) if rescale else F([1.5, np.inf, 1e30, 1.0, 2.0, 1e10])
        for n in range(2):
            v[n].reshape(-1)[1:7] = np.roll(beyond, n)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def u8_pixels(pixels):
    rng = np.random.default_rng(pixels)
    f = rng.integers(0, 256, (pixels, 3)).astype(np.uint8)
    if pixels >= 3:
        f[:3] = TRIPLES
        f[-1] = (255, 255, 254)
    else:
        f[0] = (0, 0, 1)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def equidistant_colours():
    """Colours whose two nearest palette entries are equally near, one per pair of entries that a search over 200000 colours finds."""
    rng = np.random.default_rng(19)
    c = rng.integers(0, 256, (3, 200000)).astype(np.uint8)
    d = raw.palette_distances(c)
    order = np.argsort(d, axis=0, kind="stable")[:2]
    two = np.take_along_axis(d, order, axis=0)
    tie = np.nonzero(two[0] == two[1])[0]
    seen, keep = set(), []
    for t in tie:
        pair = (int(order[0, t]), int(order[1, t]))
        if pair not in seen:
            seen.add(pair)
            keep.append(t)
    out = c[:, keep].copy()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def semantic_image(hw):
    rng = np.random.default_rng(hw)
    img = rng.integers(0, 256, (3, hw)).astype(np.uint8)
    if hw > 1:
        ties = equidistant_colours()
        own = raw.PALETTE19.T.astype(np.uint8)
        special = np.concatenate([own, ties], axis=1)[:, :hw - 1]
        img[:, 1:1 + special.shape[1]] = special
    else:
        img[:, 0] = equidistant_colours()[:, 0]
    img.setflags(write=False)
    return img


ENTRY_POINTS = ("resize_u8", "resize_f32", "dense_stream", "depth_normals", "normal_stream", "metric_normals", "lidar_splat_visible", "lidar_depth_resolve",
                "depth_complete", "frames_to_u8", "depth_from_u8", "semantic_nearest", "log_sheet")
SOURCES = ("frames.hip", "normals.hip", "lidar_depth.hip", "post.hip")
