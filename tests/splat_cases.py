"""TEST INFRASTRUCTURE: the inputs that the CPU and the GPU tests of the splat kernels (csrc/splat.hip, splat_shared.h) share.  Each case
names the clause of the kernel it aims at (`clause`) and, as `reach`, the properties that tests/test_splat_cpu.py asserts of it with
the definition alone (tests/splat_reference.py), so that a table which stops reaching its clause fails on the CPU.  Nothing here runs a
kernel; every case is made once per process."""
import functools

import numpy as np

import splat_reference as sr

F = np.float32
EYE = np.eye(4)[:3].astype(F)
ZERO = np.zeros((3, 4), dtype=F)
CAM = np.array([1, 1, 0, 0], dtype=F)                          # u = x / z, v = y / z
MAX_SPRITE = 8                                                 # csrc/splat_shared.h
TW, TH, HALO = 64, 16, 6                                       # csrc/splat.hip: the compose tile and the dilation's reach
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1

IMAGE_SIZES = ((1, 1), (1, 7), (5, 3), (17, 65), (37, 53))
SPRITE_SIZES = (1.0, 2.5, 4.0, 7.0)
SIDES = {1.0: (1,), 2.5: (2, 3), 4.0: (4,), 7.0: (7,)}         # pixels a side that an unclipped sprite of this size covers
CLOUD_SIZES = (1, 255, 256, 257)


def shifted(dx=0.0, dy=0.0, dz=0.0):
    m = EYE.copy()
    m[:, 3] = (dx, dy, dz)
    return m


def _pixels_to_points(u, v, z):
    z = np.asarray(z, dtype=F)
    return np.stack([np.asarray(u, dtype=F) * z, np.asarray(v, dtype=F) * z, z], axis=1).astype(F)


def _cloud(rng, n, H, W, size):
    """n points whose image positions spread a sprite and a half beyond every border, depths between 0.5 and 150."""
    m = float(size) * 1.5
    u, v = rng.uniform(-m, W + m, n), rng.uniform(-m, H + m, n)
    return _pixels_to_points(u, v, rng.uniform(0.5, 150.0, n)), rng.integers(0, 256, (n, 3)).astype(np.uint8)


def _case(name, clause, reach, H, W, size, xyz, rgb, mats, ids=None, znear=sr.ZNEAR, zfar=sr.ZFAR, **extra):
    mats = np.asarray(mats, dtype=F)
    assert mats.ndim == 4 and mats.shape[2:] == (3, 4)                                  # (poses, nmat, 3, 4)
    return dict(name=name, clause=clause, reach=tuple(reach), H=H, W=W, size=float(size), xyz=np.asarray(xyz, dtype=F),
                rgb=np.asarray(rgb, dtype=np.uint8), mats=mats, ids=None if ids is None else np.asarray(ids, dtype=np.int32),
                znear=znear, zfar=zfar, **extra)


THREE_POSES = np.stack([EYE, shifted(0.75, -0.5, 0.25), shifted(-1.25, 0.5, 1.0)])[:, None]


def _sized_cases():
    out = []
    for k, (H, W) in enumerate(IMAGE_SIZES):
        for s, size in enumerate(SPRITE_SIZES):
            rng = np.random.default_rng(1000 + 10 * k + s)
            n = (257, 600, 1500)[(k + s) % 3]
            xyz, rgb = _cloud(rng, n, H, W, size)
            xyz[0] = (0.5 * W, 0.5 * H, 1.0)                                             # one sprite about the centre of the image
            poses = THREE_POSES if (k + s) % 2 else THREE_POSES[:1]
            reach = ["max_sprite", "every_border"] + [f"side={a}" for a in SIDES[size] if a <= min(H, W)]
            out.append(_case(f"{H}x{W} size {size:g}", f"cover() and the clip to [0, {W}) x [0, {H}) at point size {size:g}; the MAX_SPRITE clamp "
                             f"never binds; {poses.shape[0]} pose(s)", reach, H, W, size, xyz, rgb, poses))
    return out


def _cloud_size_cases():
    out = []
    for n in CLOUD_SIZES:
        rng = np.random.default_rng(2000 + n)
        xyz, rgb = _cloud(rng, n, 17, 65, 2.5)
        xyz[-1] = _pixels_to_points([30.5], [8.5], [0.25])[0]               # the last lane's point is nearest: it must show
        xyz[0] = _pixels_to_points([3.5], [3.5], [0.25])[0]
        last = {1: "holds one lane", 255: "lacks one lane", 256: "is full (no empty workgroup)", 257: "holds one lane (the second)"}[n]
        out.append(_case(f"{n} points", f"idx < n in splat_points_kernel: the last workgroup {last}", ["first_and_last_win", "max_sprite"],
                         17, 65, 2.5, xyz, rgb, THREE_POSES if n == 257 else THREE_POSES[:1]))
    return out


def _hand_case(size):
    """Points placed by hand on 17 x 65, z = 1 unless stated: image position = (x, y)."""
    H, W, h = 17, 65, size / 2
    znear, zfar = F(sr.ZNEAR), F(sr.ZFAR)
    up, down = lambda a: np.nextafter(F(a), F(np.inf)), lambda a: np.nextafter(F(a), F(-np.inf))
    pts, kept, culled, ties = [], [], [], []

    def add(u, v, z=1.0, keep=None):
        pts.append((F(u) * F(z), F(v) * F(z), F(z)))
        if keep is not None:
            (kept if keep else culled).append(len(pts) - 1)
        return len(pts) - 1

    for u, v in ((0.2, 8.3), (64.9, 8.3), (30.3, 0.1), (30.3, 16.9), (0.3, 0.3), (64.8, 0.2), (0.2, 16.8), (64.7, 16.9)):
        add(u, v, keep=True)                                                             # a sprite across each border and each corner
    # the home pixel outside the image and the sprite reaching in (size 1 reaches nothing from there: 0.25 inside instead)
    reach_in = 0.45 if size > 1 else -0.25
    for u, v in ((-reach_in, 5.2), (W + reach_in, 5.2), (20.2, -reach_in), (20.2, H + reach_in)):
        add(u, v, z=2.0, keep=True)
    for u, v in ((-size, 5.0), (W + size, 5.0), (20.0, -size), (20.0, H + size), (-h, 5.0), (W + h, 5.0), (20.0, -h), (20.0, H + h)):
        add(u, v, keep=False)                                                            # one sprite outside; exactly on the cull's bound
    for u, v in ((10.0, 5.0), (10.5, 5.5), (12.0, 11.5), (40.5, 3.0), (50.0, 12.0), (51.5, 12.5), (26.75, 11.25), (38.25, 2.75)):
        add(u, v, z=3.0, keep=True)                                                      # integers, halves (quarters for 2.5): lo <= i + 0.5 < hi on its bound
    for z, keep in ((znear, False), (zfar, False), (up(znear), True), (down(zfar), True), (down(znear), False), (up(zfar), False)):
        add(45.5, 8.5, z=z, keep=keep)
    add(22.5, 8.5, z=-1.0, keep=False)                                                   # behind the camera
    pts.append((F(22.5), F(8.5), F(0.0)))                                                # zc = 0
    culled.append(len(pts) - 1)
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            p = [F(22.5), F(8.5), F(1.0)]
            p[axis] = F(bad)
            pts.append(tuple(p))
            culled.append(len(pts) - 1)
    a = add(33.5, 13.5, z=0.5)                                                           # ties: bit-equal zc on the same pixels
    add(5.0, 5.0, z=0.75)
    b = add(33.5, 13.5, z=0.5)
    ties.append((a, b))
    c = add(58.5, 4.5, z=0.5)
    d = add(59.0, 4.5, z=0.5)                                                            # a partial overlap: the shared pixels go to c
    ties.append((c, d))
    xyz = np.array(pts, dtype=F)
    rng = np.random.default_rng(77)
    rgb = rng.integers(1, 256, (len(pts), 3)).astype(np.uint8)
    mats = np.stack([EYE, ZERO, shifted(1.0, 1.0, 0.0)])[:, None]                        # pose 1: the zero matrix, zc = 0 for every point
    return _case(f"hand-placed, size {size:g}", "splat_project: the depth range, the off-image cull, not-a-number; cover() on its bounds and at "
                 "every border; the key's index half on ties; a zero matrix", ["kept_and_culled", "ties", "zero_matrix", "on_the_bound",
                                                                                 "every_border", "max_sprite"],
                 H, W, size, xyz, rgb, mats, kept=tuple(kept), culled=tuple(culled), ties=tuple(ties), empty_poses=(1,))


def _id_cases():
    rng = np.random.default_rng(31)
    H, W, n = 17, 65, 300
    xyz, rgb = _cloud(rng, n, H, W, 4.0)
    ids = rng.integers(0, 3, n)
    ids[:8] = (-1, 3, INT32_MIN, INT32_MAX, -7, 1000, 0, 2)
    xyz[:8] = _pixels_to_points(8.5 + 6.0 * np.arange(8), np.full(8, 8.5), np.full(8, 0.3))     # in view and nearest at every matrix
    table = np.stack([np.stack([EYE, shifted(2.0, 0.0, 0.0), shifted(0.0, 3.0, 0.0)]),
                      np.stack([shifted(-1.0, 1.0, 0.5), shifted(4.0, -2.0, 0.0), shifted(0.0, 0.0, 2.0)])])
    three = _case("ids over three matrices", "the id clamp of splat_points_kernel<true, .>: id < 0 -> 0, id >= nmat -> nmat - 1",
                  ["ids_clamped", "max_sprite"], H, W, 4.0, xyz, rgb, table, ids=ids, out_of_range=(0, 1, 2, 3, 4, 5))
    wild = ids.copy()
    wild[8:] = rng.integers(INT32_MIN, INT32_MAX, n - 8)
    one = _case("any ids over one matrix", "the id clamp with nmat = 1: every id takes matrix 0, the image is the id-less launch's",
                ["ids_do_not_matter", "max_sprite"], H, W, 4.0, xyz, rgb, table[:, :1], ids=wild)
    return [three, one]


@functools.lru_cache(maxsize=None)
def points_cases():
    return tuple(_sized_cases() + _cloud_size_cases() + [_hand_case(s) for s in SPRITE_SIZES] + _id_cases())


@functools.lru_cache(maxsize=None)
def points_keys(name):
    """The definition's key images (poses, H, W) uint64 and its count of (point, pose, pixel) covers for one case."""
    c = {c["name"]: c for c in points_cases()}[name]
    args = (CAM, c["size"], c["H"], c["W"], c["znear"], c["zfar"])
    keys = np.stack([sr.splat_keys(c["xyz"], m[0] if c["ids"] is None else m, *args, ids=c["ids"]) for m in c["mats"]])
    covered = sum(sr.covers(c["xyz"], m[0] if c["ids"] is None else m, *args, ids=c["ids"]) for m in c["mats"])
    keys.setflags(write=False)
    return keys, covered


def seeded_keys(case, seed=5):
    """A key image to draw on top of: a third empty, the rest keys of some earlier cloud (any depth in range, any index)."""
    rng = np.random.default_rng(seed)
    shape = (case["mats"].shape[0], case["H"], case["W"])
    z = rng.uniform(0.4, 160.0, shape).astype(F)
    keys = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | rng.integers(0, 4000, shape).astype(np.uint64)
    return np.where(rng.random(shape) < 0.33, sr.EMPTY, keys)


# ------------------------------------------------------------------------------------------------ resolve
# (name, clause, pixels, offsets in elements of keys / depth / colour, the form the entry point chooses)
RESOLVE_CASES = (
    ("4 wide", "splat_resolve_kernel<4>: one lane", 4, (0, 0, 0), 4),
    ("1024 wide", "splat_resolve_kernel<4>: one full workgroup", 1024, (0, 0, 0), 4),
    ("1028 wide", "splat_resolve_kernel<4>: i >= total in a second workgroup of one lane", 1028, (0, 0, 0), 4),
    ("1 narrow", "splat_resolve_kernel<1>: pixels & 3", 1, (0, 0, 0), 1),
    ("1961 narrow", "splat_resolve_kernel<1>: 37 x 53 pixels, i >= total in the eighth workgroup", 1961, (0, 0, 0), 1),
    ("1024 keys off", "the dispatch's aligned16(keys): keys 8 bytes off a 16-byte address", 1024, (1, 0, 0), 1),
    ("1024 depth off", "the dispatch's aligned16(depth): depth one float off", 1024, (0, 1, 0), 1),
    ("1024 colour off", "the dispatch's aligned16(colour): colour one word off", 1024, (0, 0, 1), 1),
)
RESOLVE_POINTS, RESOLVE_BUFFER = 500, 1000                     # n as passed, and the points the buffer holds: foreign indices stay inside it


@functools.lru_cache(maxsize=None)
def resolve_points():
    rng = np.random.default_rng(404)
    xyz = rng.uniform(-50, 50, (RESOLVE_BUFFER, 3))
    packed = sr.pack(xyz, rng.integers(0, 256, (RESOLVE_BUFFER, 3)).astype(np.uint8), top=rng.integers(1, 256, RESOLVE_BUFFER))
    packed.setflags(write=False)
    return packed


@functools.lru_cache(maxsize=None)
def resolve_keys(pixels):
    """Winners, empty pixels and indices >= n (inside the buffer) in equal parts, in an order of their own for every size."""
    rng = np.random.default_rng(pixels)
    z = rng.uniform(1e-3, 199.0, pixels).astype(F)
    kind = np.arange(pixels) % 3 if pixels < 8 else rng.integers(0, 3, pixels)
    if pixels == 1:
        kind = np.array([0])
    index = np.where(kind == 2, rng.integers(RESOLVE_POINTS, RESOLVE_BUFFER, pixels), rng.integers(0, RESOLVE_POINTS, pixels))
    keys = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | index.astype(np.uint64)
    keys = np.where(kind == 1, sr.EMPTY, keys)
    keys.setflags(write=False)
    return keys


# ------------------------------------------------------------------------------------------------ compose
COMPOSE_SIZES = ((1, 1), (5, 3), (16, 64), (17, 65), (37, 53), (33, 130))
SET = 0x00070180                                               # every channel above zero
HOLES = (0x00FFFF00, 0x00FF00FF, 0x0000FFFF)                   # red, green or blue zero: coloured, yet not in the mask

# object pixels placed by hand: (row, column) set, and probes (row, column, in the dilated mask?)
PLACED = {
    (1, 1): dict(set=(), hole=(0, 0), probes=((0, 0, False),)),
    (5, 3): dict(set=((0, 0),), hole=(4, 2), probes=((4, 2, True), (0, 2, True))),                    # clipped on all four sides at once
    (16, 64): dict(set=((0, 0), (15, 63), (8, 30)), hole=(15, 10),
                   probes=((6, 6, True), (7, 6, False), (6, 7, False), (9, 57, True), (8, 57, False), (9, 56, False),
                           (8, 24, True), (8, 23, False), (8, 36, True), (8, 37, False), (2, 30, True), (1, 30, False), (14, 30, True), (15, 30, False))),
    (17, 65): dict(set=((8, 57), (16, 64), (12, 20), (16, 40), (0, 0)), hole=(1, 30),
                   probes=((8, 63, True), (8, 64, False),                                             # 6 away at the seam's left, 7 across it
                           (10, 58, True), (10, 64, True), (9, 64, False),                           # the corner's box from the ragged tiles into tile (0, 0)
                           (16, 20, True), (16, 14, True), (16, 13, False),                          # down across y = 15 | 16
                           (10, 40, True), (9, 40, False), (15, 46, True), (15, 47, False),          # up across it
                           (6, 6, True), (7, 0, False), (0, 7, False), (1, 30, False))),
    (37, 53): dict(set=((0, 0), (0, 52), (36, 0), (36, 52), (18, 26)), hole=(18, 45),
                   probes=((6, 6, True), (7, 6, False), (6, 46, True), (6, 45, False), (30, 6, True), (29, 6, False), (30, 46, True), (30, 45, False),
                           (12, 26, True), (11, 26, False), (24, 32, True), (25, 32, False), (15, 20, True), (16, 19, False), (18, 45, False))),
    (33, 130): dict(set=((5, 58), (22, 67), (12, 110), (19, 30), (32, 129), (0, 0), (32, 0), (0, 129), (0, 90), (32, 50), (16, 0), (16, 129)),
                    hole=(28, 100),
                    probes=((5, 64, True), (5, 65, False), (11, 64, True), (12, 64, False),          # rightwards across x = 63 | 64
                            (22, 61, True), (22, 60, False), (16, 61, True), (15, 61, False),        # leftwards across it; 7 up is across y = 15 | 16
                            (18, 110, True), (19, 110, False), (16, 104, True), (16, 103, False),    # down across y = 15 | 16
                            (13, 30, True), (12, 30, False), (15, 36, True), (15, 37, False),        # up across it
                            (26, 123, True), (25, 123, False), (26, 122, False), (32, 123, True),    # the four corners, clipped
                            (6, 6, True), (7, 6, False), (26, 6, True), (25, 6, False), (6, 123, True), (7, 123, False),
                            (6, 84, True), (6, 97, False), (26, 56, True), (26, 57, False),          # the top and the bottom border
                            (10, 6, True), (22, 7, False), (10, 123, True), (16, 122, False),        # the left and the right border
                            (28, 100, False))),
}


@functools.lru_cache(maxsize=None)
def compose_layers(hw, poses=2):
    """(bg_colour, bg_depth, obj_colour, obj_depth), each (poses, H, W): colour words uint32 and float32 depths such as resolve gives
    them — 0 with colour 0 where nothing landed, else a depth in (1e-4, 200), a quarter of them above 100.  Pose 0 carries the
    hand-placed object pixels of PLACED, every further pose the same pixels moved by one row and column plus a few at random; at `hole`
    and beside it lie pixels with one channel zero, the blue one at `hole` itself in pose 0."""
    H, W = hw
    rng = np.random.default_rng(H * 1000 + W)
    shape = (poses, H, W)

    def depths():
        d = np.exp(rng.uniform(np.log(2e-4), np.log(100.0), shape))
        return np.where(rng.random(shape) < 0.25, rng.uniform(100.0, 199.0, shape), d).astype(F)

    bg_d = depths()
    bg_c = rng.integers(0, 1 << 24, shape).astype(np.uint32)
    empty = rng.random(shape) < 0.3
    bg_d[empty], bg_c[empty] = 0, 0
    if H * W == 1:
        bg_d[0, 0, 0], bg_c[0, 0, 0] = 150.0, 0x00C86432
    ob_d, ob_c = np.zeros(shape, F), np.zeros(shape, np.uint32)
    placed = PLACED[hw]
    for p in range(poses):
        spots = [((r + p) % H, (c + p) % W) for r, c in placed["set"]]
        if p and H * W > 1000:
            spots += [(int(r), int(c)) for r, c in zip(rng.integers(0, H, 3), rng.integers(0, W, 3))]
        for k, (r, c) in enumerate(spots):
            ob_c[p, r, c] = SET + k
            ob_d[p, r, c] = (3.5, 120.0, 0.004, 61.25)[k % 4]
        r, c = placed["hole"]
        for k in range(3):                                                               # three coloured pixels side by side, another channel zero in each
            x = c + k - 1
            if 0 <= x < W and not ob_c[p, r, x]:
                ob_c[p, r, x], ob_d[p, r, x] = HOLES[(k + 1 + p) % 3], 9.0
    for a in (bg_c, bg_d, ob_c, ob_d):
        a.setflags(write=False)
    return bg_c, bg_d, ob_c, ob_d


def compose_clause(hw):
    H, W = hw
    tx, ty = -(-W // TW), -(-H // TH)
    ragged = sum(1 for x in range(tx) for y in range(ty) if (x + 1) * TW > W or (y + 1) * TH > H)
    return f"splat_compose_kernel at {H} x {W}: {tx * ty} tile(s), {ragged} ragged (y >= H || x >= W), the halo clipped at every border"


# ------------------------------------------------------------------------------------------------ refusals
# (entry point, what is wrong, the argument(s) changed, a piece of the message).  The GPU test starts from a valid call each time.
REFUSALS = (
    ("points", "point size 0", dict(point_size=0.0), "point size"),
    ("points", "point size above 7", dict(point_size=7.5), "point size"),
    ("points", "negative point size", dict(point_size=-1.0), "point size"),
    ("points", "point size not a number", dict(point_size=float("nan")), "point size"),
    ("points", "znear = 0", dict(znear=0.0), "znear"),
    ("points", "znear < 0", dict(znear=-1.0), "znear"),
    ("points", "zfar = znear", dict(znear=2.0, zfar=2.0), "znear"),
    ("points", "zfar < znear", dict(znear=2.0, zfar=1.0), "znear"),
    ("points", "points 8 bytes off", dict(points=+8), "unaligned"),
    ("points", "keys 4 bytes off", dict(keys=+4), "unaligned"),
    ("points", "no points", dict(points=None), "bad arguments"),
    ("points", "no matrices", dict(mats=None), "bad arguments"),
    ("points", "no keys", dict(keys=None), "bad arguments"),
    ("points", "n = 0", dict(n=0), "bad arguments"),
    ("points", "poses = 0", dict(poses=0), "bad arguments"),
    ("points", "nmat = 0", dict(nmat=0), "bad arguments"),
    ("points", "H = 0", dict(H=0), "bad arguments"),
    ("points", "W = -1", dict(W=-1), "bad arguments"),
    ("points", "2^32 + 1 points", dict(n=2 ** 32 + 1), "32-bit index"),
    ("points", "three matrices, no ids", dict(nmat=3), "per-point ids"),
    ("points", "2^23 rows", dict(H=1 << 23), "too large"),
    ("points", "2^31 pixels", dict(H=1 << 16, W=1 << 15), "too large"),
    ("resolve", "no keys", dict(keys=None), "bad arguments"),
    ("resolve", "no points", dict(points=None), "bad arguments"),
    ("resolve", "no depth", dict(depth=None), "bad arguments"),
    ("resolve", "no colour", dict(colour=None), "bad arguments"),
    ("resolve", "n = 0", dict(n=0), "bad arguments"),
    ("resolve", "pixels = 0", dict(pixels=0), "bad arguments"),
    ("resolve", "2^40 + 1 pixels", dict(pixels=2 ** 40 + 1), "too large"),
    ("compose", "no background colour", dict(bg_colour=None), "bad arguments"),
    ("compose", "no background depth", dict(bg_depth=None), "bad arguments"),
    ("compose", "no sparse_frames", dict(sparse=None), "bad arguments"),
    ("compose", "no sparse_depth", dict(sdepth=None), "bad arguments"),
    ("compose", "poses = 0", dict(poses=0), "bad arguments"),
    ("compose", "H = 0", dict(H=0), "bad arguments"),
    ("compose", "W = 0", dict(W=0), "bad arguments"),
    ("compose", "object colour without depth", dict(obj_depth=None), "come together"),
    ("compose", "object depth without colour", dict(obj_colour=None), "come together"),
    ("compose", "T = 0", dict(T=0, t=0), "frame"),
    ("compose", "t = -1", dict(t=-1), "frame"),
    ("compose", "t = T", dict(t=3), "frame"),
    ("compose", "poses overlap by one element", dict(pose_stride_delta=-1), "overlap"),
    ("compose", "65536 poses", dict(poses=65536), "grid too large"),
    ("compose", "65535 * 16 + 1 rows", dict(H=65535 * 16 + 1, pose_stride=2 ** 40), "grid too large"),
)
