"""TEST INFRASTRUCTURE: the inputs that the CPU and the GPU tests of the scene kernels share (csrc/cloud.hip, neighbours.hip, depth.hip,
consistency.hip, metrics.hip; tests/test_scene_cpu.py, tests/test_scene_kernels_gpu.py).  Every case is a dict of numpy arrays that
names the clause it aims at (`clause`); test_scene_cpu.py asserts with the definitions alone that it reaches that clause, so that a case
which stops reaching it fails on the CPU.  Nothing here runs a kernel; every case is made once per process and is read-only.

Spoiled table entries are chosen so that a kernel which used them unchecked would still address inside the allocation the GPU test
makes: at most one element, row or view past either end of a buffer (sentinel_buffers.Flat keeps 256 elements in front and 264 behind)."""
import functools

import numpy as np

import cloud_reference as cr
import consistency_reference as vr
import neighbours_reference as nr
import scene_raw_reference as raw

F, D = np.float32, np.float64
FRAMES = 2                                                     # two frames or views throughout: the second one's base is exercised
SKY = 10
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
WG = 256                                                       # lanes of a workgroup in every kernel but depth_align_solve (64)


def _frozen(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


# ------------------------------------------------------------------------------------------------ the four-pixel / one-pixel kernels
PIXEL_SIZES = ((3, 4), (43, 24), (5, 7), (37, 53))
PIXEL_CLAUSE = {(3, 4): "the wide form, three lanes", (43, 24): "the wide form, 258 lanes: two lanes in a second workgroup",
                (5, 7): "W % 4 != 0: the one-pixel form, 35 lanes", (37, 53): "W % 4 != 0: the one-pixel form, the eighth workgroup partial"}
ALIGNED_SIZE = (43, 24)                                        # the size at which every pointer of the wide predicate is moved in turn
LIDAR_SPECIAL = (np.nan, -1.0, 256.0, 300.0, 2.0 ** -21, 3 * 2.0 ** -21, np.inf)       # not counted ...; halves of the 2^-20 grid; not counted
DEPTH_SPECIAL = (np.nan, 0.0, -3.0, np.inf, 100.0, 2.0 ** -7, 255.5)
LABEL_SPECIAL = (SKY + 2 ** 32, 2 ** 40, -1, -2 ** 40, SKY, 12, 63, 64)                # the low word alone is sky's; ...; dynamic; in and out of the mask
DYNAMIC_MASK = vr.DYNAMIC_MASK | (1 << 63)


def lanes(hw, wide):
    """(lanes of a frame, lanes in the last workgroup) of a per-pixel kernel."""
    n = hw[0] * hw[1] // 4 if wide else hw[0] * hw[1]
    return n, n - (n - 1) // WG * WG


@functools.lru_cache(maxsize=None)
def pixel_case(hw):
    """What the six per-pixel kernels read at H x W: a depth stream and a second picture, LiDAR depths, generated depths, labels, the
    fitted lines and the lifting tables of two frames.  The first and the last pixel of each frame count in every sum."""
    H, W = hw
    n = H * W
    rng = np.random.default_rng(100 * H + W)
    frames = rng.integers(0, 256, (FRAMES, n, 3)).astype(np.uint8)
    frames[rng.random((FRAMES, n)) < 0.1] = 0                                           # k = 0: not counted
    other = np.clip(frames.astype(np.int64) + rng.integers(-40, 41, frames.shape), 0, 255).astype(np.uint8)
    lidar = rng.uniform(0.5, 90.0, (FRAMES, n)).astype(F)
    lidar[rng.random((FRAMES, n)) < 0.2] = 0
    depth = rng.uniform(0.2, 120.0, (FRAMES, n)).astype(F)
    labels = rng.integers(0, 19, (FRAMES, n)).astype(np.int64)
    for f in range(FRAMES):
        lidar[f, 1:1 + len(LIDAR_SPECIAL)] = LIDAR_SPECIAL
        depth[f, 2:2 + len(DEPTH_SPECIAL)] = DEPTH_SPECIAL
        labels[f, 3:3 + len(LABEL_SPECIAL)] = LABEL_SPECIAL
        for at in (0, n - 1):
            frames[f, at], other[f, at] = (200, 7 + f, 90), (3, 250, 91 + f)
            lidar[f, at], depth[f, at], labels[f, at] = 17.25 + f, 20.5 - f, 12
    coef = np.array([[80.5, 1.25], [-130.0, 40.0]], dtype=D)                             # frame 1 falls: clipped at 0 where k is large
    a = 0.1
    c2w = np.array([[np.cos(a), 0, np.sin(a), 1.5], [0, 1, 0, -0.25], [-np.sin(a), 0, np.cos(a), 3.0]])
    table = np.stack([np.r_[c2w.reshape(-1), 0.8 * W, 0.9 * W, 0.5 * W, 0.5 * H], np.r_[np.eye(4)[:3].reshape(-1), 1.0 * W, 1.0 * W, 0.25 * W, 0.75 * H]]).astype(D)
    shape = (FRAMES, H, W)
    return _frozen(dict(name=f"{H}x{W}", clause=PIXEL_CLAUSE[hw], H=H, W=W, frames=frames.reshape(*shape, 3), other=other.reshape(*shape, 3),
                        lidar=lidar.reshape(shape), depth=depth.reshape(shape), labels=labels.reshape(shape), coef=coef, table=table))


def start_sums(shape, seed):
    """A non-zero pattern that accumulating outputs start from: words below 2^40, no two alike."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    return ((rng.integers(1, 1 << 20, n).astype(np.uint64) << np.uint64(20)) + np.arange(1, n + 1, dtype=np.uint64)).reshape(shape)


# ------------------------------------------------------------------------------------------------ mudg_depth_align_solve
SOLVE_FRAMES = (1, 64, 65)
HEADROOM_ROW = (2 ** 24, 2 ** 23 * 766, 2 ** 23 * (765 * 765 + 1), 2 ** 23 * 2 ** 28, 2 ** 23 * (765 * (2 ** 28 - 1) + 1))
# 2^24 pixels (the most a frame holds), half of them white at the largest q below 256 m, half at k = 1, q = 1


@functools.lru_cache(maxsize=None)
def solve_case(frames):
    """(frames, 5) uint64 sums of pixel sets: row 0 at the headroom the header states; then, where there is room, an empty frame, one
    pixel, five pixels of one k (no spread), two pixels; the rest 2 .. 30 pixels at random; the last row at the headroom again."""
    rng = np.random.default_rng(frames)
    rows, kinds = [], []
    for f in range(frames):
        if f == 0 or (f == frames - 1 and frames > 1):
            rows.append(HEADROOM_ROW), kinds.append("headroom")
            continue
        m = {1: 0, 2: 1, 3: 5, 4: 2}.get(f, int(rng.integers(2, 31)))
        k = rng.integers(1, 766, m)
        if f == 3:
            k[:] = 100
        q = rng.integers(1, 1 << 28, m)
        rows.append((m, int(k.sum()), int((k * k).sum()), int(q.sum()), int((k * q).sum())))
        kinds.append({1: "empty", 2: "one pixel", 3: "no spread"}.get(f, "fitted"))
    return _frozen(dict(name=f"{frames} frames", clause="a lane owns a frame, 64 lanes a workgroup: f >= frames, n < 2, den <= 0, the sums' headroom",
                        sums=np.array(rows, dtype=np.uint64), kinds=tuple(kinds)))


# ------------------------------------------------------------------------------------------------ mudg_colormap_spectral
COLORMAP_SIZES = (1, 257)
COLORMAP_RANGES = ((0.0, 1.0), (2.0, 50.0))


def knot_values():
    """For each of the ten knots k / 10 (k = 0 .. 9) and for 1.0 an fp32 x with fp32(x 10) == k exactly."""
    out = []
    for k in range(11):
        x = F(k / 10)
        for cand in (x, np.nextafter(x, F(2)), np.nextafter(x, F(-1))):
            if F(cand) * F(10) == F(k):
                out.append(F(cand))
                break
    return np.array(out, dtype=F)


@functools.lru_cache(maxsize=None)
def colormap_case(n, value_range):
    lo, hi = value_range
    rng = np.random.default_rng(n)
    x = rng.uniform(-0.2, 1.2, n).astype(F)
    if n > 1:
        special = np.r_[knot_values(), F([np.nan, np.inf, -np.inf, -0.5, 1.5, 0.35])]
        x[:len(special)] = special
        x[-1] = F(0.55)
    else:
        x[0] = F(0.35)
    values = x if value_range == (0.0, 1.0) else (F(lo) + x * F(hi - lo)).astype(F)
    return _frozen(dict(name=f"{n} values in ({lo:g}, {hi:g})", clause="i >= n in the second workgroup; the clamp, the knots, what is not a number; the rescale",
                        values=values, unit=x, val_min=lo, val_max=hi))


# ------------------------------------------------------------------------------------------------ mudg_metric_ssim
SSIM_SIZES = ((11, 11), (12, 43), (42, 42), (43, 75))
SSIM_TILES = {(11, 11): (1, 1, 1), (12, 43): (1, 2, 1), (42, 42): (1, 1, 32), (43, 75): (2, 3, 1)}     # tile rows, tile columns, columns of the last tile


@functools.lru_cache(maxsize=None)
def ssim_case(hw):
    H, W = hw
    rng = np.random.default_rng(7 * H + W)
    a = rng.integers(0, 256, (FRAMES, H, W, 3)).astype(np.uint8)
    a[1, :, :, 1] = 255                                                                 # a flat white channel: the variance is zero
    b = np.clip(a.astype(np.int64) + rng.integers(-60, 61, a.shape), 0, 255).astype(np.uint8)
    b[1, :, :, 2] = a[1, :, :, 2]                                                       # an equal channel: s = 1 everywhere
    ty, tx, last = SSIM_TILES[hw]
    return _frozen(dict(name=f"{H}x{W}", clause=f"{ty} x {tx} tiles of 32 x 32 outputs, the last one {last} column(s) wide; gy < H && gx < W in the apron", H=H, W=W, a=a, b=b))


# ------------------------------------------------------------------------------------------------ mudg_metric_confusion
CONFUSION_SIZES = ((1, 1), (64, 64), (17, 241))                # 1, 4096 and 4097 pixels: a workgroup owns 4096
CONFUSION_CLASSES = (1, 19, 32)


@functools.lru_cache(maxsize=None)
def confusion_case(hw, classes):
    H, W = hw
    n = H * W
    rng = np.random.default_rng(1000 * classes + n)
    pred = rng.integers(-1, classes + 1, (FRAMES, n)).astype(np.int64)
    gt = rng.integers(-1, classes + 1, (FRAMES, n)).astype(np.int64)
    wild = (2 ** 40, -2 ** 40, -1, classes)
    if n > 1:
        for f in range(FRAMES):
            for k, v in enumerate(wild):
                pred[f, 1 + k], gt[f, 1 + k] = v, 0                                     # a counted pixel with a prediction outside: bad
                gt[f, 5 + k], pred[f, 5 + k] = v, 0                                     # a pixel that is not counted
            pred[f, 0], gt[f, 0], pred[f, n - 1], gt[f, n - 1] = 0, classes - 1, classes - 1, 0
    else:
        pred[:, 0], gt[:, 0] = (0, 2 ** 40), (0, 0)
    return _frozen(dict(name=f"{H}x{W}, {classes} classes", clause="p < end in the last workgroup; g and q tested as 64-bit values before they index the histogram",
                        H=H, W=W, classes=classes, pred=pred, gt=gt))


# ------------------------------------------------------------------------------------------------ mudg_metric_cloud
CLOUD_METRIC_SIZES = (1, 2047, 2048, 2049)                     # a workgroup owns 2048 values, eight to a lane
CLOUD_R2 = 0.25
CLOUD_T2 = tuple(float(t) for t in (0.0009765625, 0.00390625, 0.015625, 0.03125, 0.0625, 0.125, 0.1875, 0.25))


@functools.lru_cache(maxsize=None)
def cloud_metric_case(n):
    rng = np.random.default_rng(n)
    d2 = rng.uniform(0.0, CLOUD_R2, n)
    if n > 1:
        special = list(CLOUD_T2) + [CLOUD_R2, np.nan, np.inf, -np.inf, 0.0]
        d2[1:1 + len(special)] = special
        d2[-1] = CLOUD_T2[2]                                                            # the last lane's value is found and on a threshold
    else:
        d2[0] = CLOUD_R2
    return _frozen(dict(name=f"{n} values", clause="i >= n inside a lane's eight values; d2 on a threshold and on r2; not finite: not found", d2=d2.astype(D)))


# ------------------------------------------------------------------------------------------------ mudg_cloud_nearest / mudg_cloud_count
SEARCH_R = nr.LATTICE_RADIUS
SEARCH_QUERIES = (1, 256, 257)
VISITS = ("none", "permutation", "spoiled")
BIG_CAP = 1000


@functools.lru_cache(maxsize=None)
def search_case(nq, one_point=False):
    """The lattice clouds of neighbours_reference (every d2 exact), sorted the way the search takes them."""
    ref, queries, _ = nr.lattice_case(seed=3, n=300, nq=257)
    if one_point:
        ref = ref[:1]
        queries[:3] = ref[0] + F([[0, 0, 0], [SEARCH_R, 0, 0], [SEARCH_R, nr.STEP, 0]])   # on it, at exactly r, one step beyond
    queries = queries[:nq].copy()
    ref_sorted, keys, order, cell = raw.sorted_reference(ref, SEARCH_R)
    rng = np.random.default_rng(nq)
    perm = rng.permutation(nq).astype(np.int64)
    spoiled = perm.copy()
    if nq > 1:
        spoiled[0], spoiled[5], spoiled[nq - 1] = -1, nq, spoiled[7]                     # below, beyond, a duplicate: three queries lose their lane
    else:
        spoiled[0] = 1
    foreign = order.copy()                                                               # values that are no index of this cloud: only returned
    foreign[::3] = -5
    foreign[1::3] += len(ref) + 3
    foreign[2::7] = 2 ** 40
    name = f"{len(ref)} points, {nq} queries"
    return _frozen(dict(name=name, clause="j >= nq in the last workgroup; qi outside [0, nq): no slot is written; order[s] is returned, never an address",
                        ref=ref, ref_sorted=ref_sorted, keys=keys, order=order, foreign=foreign, cell=cell, queries=queries, nq=nq,
                        visit={"none": None, "permutation": perm, "spoiled": spoiled}))


# ------------------------------------------------------------------------------------------------ mudg_cloud_sweep
SWEEP_VARIANTS = ("whole", "spoiled offsets", "spoiled cameras", "no cameras", "no objects")


def _cam(h, w, base, f=2.0, shift=0.0):
    w2c = np.eye(4)[:3].astype(D)
    w2c[0, 3] = shift
    return (w2c, np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]], dtype=D), h, w, base)


def _box(centre, size, visible=True):
    w2l = np.eye(4)[:3].astype(D)
    w2l[:, 3] = [-c for c in centre]
    return (w2l, np.array(size, dtype=D), visible)


@functools.lru_cache(maxsize=None)
def sweep_case(variant):
    """Three frames of 300, 257 and 1 returns that look down +z at two small cameras (3 x 4 and 2 x 5 pixels: every pixel is hit many
    times, and many returns fall outside) and two overlapping boxes.  The spoiled variants change the tables only."""
    counts = (300, 257, 1)
    total = sum(counts)
    rng = np.random.default_rng(12)
    d = np.stack([rng.uniform(-1.6, 1.6, total), rng.uniform(-1.6, 1.6, total), np.where(rng.random(total) < 0.1, -1.0, 1.0)], axis=1).astype(F)
    o = rng.uniform(-0.01, 0.01, (total, 3)).astype(F)
    ranges = rng.uniform(1.0, 30.0, total).astype(F)
    d[[0, 299, 300, 556, 557]] = F([[-1.2, -0.7, 1], [0.9, 0.4, 1], [-1.2, -0.7, 1], [0.9, 0.4, 1], [0.1, 0.1, 1]])   # the first and last return of each frame: seen
    o[[0, 299, 300, 556, 557]] = 0
    l2w = np.stack([np.eye(4)[:3], np.eye(4)[:3], np.eye(4)[:3]]).astype(D)
    l2w[1, :, 3], l2w[2, :, 3] = (0.5, 0.0, 0.25), (0.0, 0.0, 1.0)
    sizes = ((3, 4), (2, 5))
    image_bytes = 3 * sum(3 * h * w for h, w in sizes)                                 # three frames of both cameras
    images = rng.integers(1, 256, image_bytes).astype(np.uint8)
    cams, at = [], 0
    for f in range(3):
        row = []
        for c, (h, w) in enumerate(sizes):
            row.append(_cam(h, w, at, shift=0.1 * c))
            at += 3 * h * w
        cams.append(row)
    objs = [[_box((0, 0, 15), (20, 20, 20)), _box((2, 0, 12), (10, 30, 10))], [_box((0, 0, 15), (20, 20, 20), False), _box((2, 0, 12), (10, 30, 10))],
            [_box((0, 0, 15), (20, 20, 20)), _box((2, 0, 12), (10, 30, 10))]]
    offsets = np.array([0, 300, 557, 558], dtype=np.int64)
    clause = "i >= count in the last workgroup of each frame; a frame of one return"
    if variant == "spoiled offsets":
        # frame 0 starts below 0 (return -1 is dropped), frame 1 ends beyond total (return 558 is dropped), frame 2 has a negative count
        offsets = np.array([-1, 300, total + 1, total - 5], dtype=np.int64)
        clause = "idx < 0 || idx >= total: an offset table that does not describe the buffers; a count that is not positive"
    if variant == "spoiled cameras":
        h, w = sizes[1]
        cams[0][1] = _cam(h, w, -3, shift=0.1)                                          # pixel (0, 0) would lie three bytes in front of the buffer
        cams[1][1] = _cam(h, w, image_bytes - 3 * h * w + 1, shift=0.1)                 # the last pixel would end one byte beyond it
        cams[1][0] = _cam(0, 4, 0)                                                      # no rows: sees nothing
        cams[2][0] = _cam(3, 0, 0)                                                      # no columns
        cams[2][1] = _cam(h, w, image_bytes - 3 * h * w)                                # the buffer's last pixel, and image_bytes is one short of it
        image_bytes -= 1
        clause = "at < 0 || at + 3 > image_bytes: a camera table that does not describe the image buffer; h = 0, w = 0"
    if variant == "no cameras":
        cams, clause = [[], [], []], "ncam = 0 with null tables: every return unseen, label -1, colour 0"
    if variant == "no objects":
        objs, clause = [[], [], []], "nobj = 0 with a null table: every seen return is background"
    return _frozen(dict(name=variant, clause=clause, rays_o=o, rays_d=d, ranges=ranges, offsets=offsets, total=total, max_rays=int(np.diff(offsets).max()), l2w=l2w,
                        cams=cams, objs=objs, images=images, image_bytes=image_bytes, buffer_bytes=len(images)))


def sweep_tables(case):
    """The camera and object tables as the entry point takes them: (frames, ncam, 24) eight-byte words as int64 (21 doubles, then h, w and
    the byte offset) and (frames, nobj, 16) doubles."""
    frames = len(case["cams"])
    ncam, nobj = len(case["cams"][0]), len(case["objs"][0])
    cam = np.zeros((frames, ncam, 24), dtype=np.int64)
    obj = np.zeros((frames, nobj, 16), dtype=D)
    for f in range(frames):
        for c, (w2c, K, h, w, base) in enumerate(case["cams"][f]):
            cam[f, c, :21] = np.r_[w2c.reshape(-1), K.reshape(-1)].astype(D).view(np.int64)
            cam[f, c, 21:] = (h, w, base)
        for k, (w2l, box, visible) in enumerate(case["objs"][f]):
            obj[f, k] = np.r_[w2l.reshape(-1), box, 1.0 if visible else 0.0]
    return cam, obj


# ------------------------------------------------------------------------------------------------ mudg_cloud_voxel_keys / _reduce / _finish
VOXEL = 0.5
VOXEL_RUNS = {1: (1,), 65: (1, 60, 4), 257: (1, 2, 59, 70, 1, 100, 17, 7)}     # runs of equal rank in sorted order: 61 .. 64 crosses a wave,
VOXEL_SPOILS = ("none", "order", "segments")                                   # 62 .. 131 two waves, 250 .. 256 a workgroup


@functools.lru_cache(maxsize=None)
def voxel_case(n, spoil="none"):
    """n points in len(runs) voxels whose keys rise with the run, shuffled; `order` and `segments` as a stable sort by key and the rank of
    each key give them, and (n > 1) one more voxel than there are runs: no entry names the last one.  The run of two holds colours whose mean is
    exactly on .5 in every channel."""
    runs = VOXEL_RUNS[n]
    rng = np.random.default_rng(n)
    idx = np.concatenate([np.tile([[k - 3, 5 - k, 2 * k]], (m, 1)) for k, m in enumerate(runs)])
    xyz = ((idx + rng.integers(0, 1 << 12, (n, 3)) / 4096.0) * VOXEL).astype(F)                # exact in fp32: the index is what was meant
    rgb = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    if len(runs) > 1 and runs[1] == 2:
        rgb[1:3] = [[10, 0, 255], [11, 1, 254]]
    shuffle = rng.permutation(n)
    xyz, rgb = xyz[shuffle], rgb[shuffle]
    packed = cr.pack(xyz, rgb)
    keys = raw.voxel_keys(xyz, VOXEL)
    order = np.argsort(keys, kind="stable").astype(np.int64)
    segments = np.cumsum(np.r_[0, np.diff(keys[order]) != 0]).astype(np.int64)
    voxels = len(runs) + 1 if n > 1 else 1                                                     # the entry point takes voxels <= n
    spoiled = ()
    if spoil != "none" and n > 1:
        # inside the long run (its lanes on either side still count once), at a run's head, at the cloud's last entry
        spoiled = {65: (30, 61, 64), 257: (100, 132, 256)}[n]
        bad = (-1, n, -1) if spoil == "order" else (-1, voxels, voxels)
        target = order if spoil == "order" else segments
        for at, v in zip(spoiled, bad):
            target[at] = v
    elif spoil != "none":
        (order if spoil == "order" else segments)[0] = n if spoil == "order" else voxels
        spoiled = (0,)
    return _frozen(dict(name=f"{n} points, spoiled {spoil}", clause="runs of equal rank across a wave and a workgroup; an order or a ranking that is not this cloud's: dropped",
                        n=n, runs=runs, xyz=xyz, rgb=rgb, packed=packed, keys=keys, order=order, segments=segments, voxels=voxels, spoiled=tuple(spoiled)))


@functools.lru_cache(maxsize=None)
def voxel_wrap_points():
    """65 points of which the first six have a voxel index outside [-2^20, 2^20) on some axis."""
    xyz = voxel_case(65)["xyz"].copy()
    xyz[:6] = F([[600000.0, 0, 0], [0, -600000.25, 0], [0, 0, 524288.0], [-524288.25, 1, 1], [1048576.0, -1048576.0, 3], [524287.75, -524288.0, 0]])
    xyz.setflags(write=False)
    return xyz


# ------------------------------------------------------------------------------------------------ mudg_view_consistency
VIEW_SIZES = ((1, 1), (16, 16), (1, 257))
VIEW_WITNESSES = (1, 64)
# "near": ids -1, V and the view itself: a view, a table row and a time one past the end at the most.  "wild": those and INT32_MIN,
# INT32_MAX, the only spoiled values here that an unchecked kernel would not survive; they have cases of their own, so that the near
# ones alone show a missing check by its bits.
VIEW_IDS = ("near", "wild")
VIEW_PARAMS = dict(r=2, min_agree=1, max_violate=0, rel_tol=0.02, abs_tol=0.05)


def _view_tables(V, H, W, shifts):
    f = float(max(H, W))
    src, wit = np.zeros((V, 16)), np.zeros((V, 16))
    for v in range(V):
        c2w = np.eye(4)
        c2w[0, 3] = shifts[v]
        src[v] = np.r_[c2w[:3].reshape(-1), f, f, W / 2, H / 2]
        wit[v] = np.r_[np.linalg.inv(c2w)[:3].reshape(-1), f, f, W / 2, H / 2]
    return src.astype(D), wit.astype(D)


@functools.lru_cache(maxsize=None)
def view_case(hw, N, ids="near"):
    """Five views of a wall about 10 m ahead, each a little to the side of the last: projections land within a pixel or two.  View 3's
    witness row holds NaN, view 4's a translation of 1e300: neither gives evidence.  The witness lists cycle through the spoiled ids,
    the view itself and the other views (a view may stand in a list more than once: each entry is a verdict of its own)."""
    H, W = hw
    V = 5
    rng = np.random.default_rng(H * 1000 + W + N)
    depth = (10.0 + rng.uniform(-0.08, 0.08, (V, H, W))).astype(F)
    depth[rng.random(depth.shape) < 0.1] = 3.0                                          # something nearer: a witness sees through it
    labels = rng.integers(0, 19, (V, H, W)).astype(np.int64)
    flags = vr.flags(depth, labels, SKY, vr.DYNAMIC_MASK, 0.0, 100.0)
    src, wit = _view_tables(V, H, W, (0.0, 0.4, -0.3, 0.7, -0.6))
    wit[3, 0], wit[4, 3] = np.nan, 1e300
    times = np.array([0, 0, 1, 1, 0], dtype=np.int32)
    spoiled = (-1, V) if ids == "near" else (-1, V, INT32_MIN, INT32_MAX)
    witnesses = np.zeros((V, N), dtype=np.int32)
    for s in range(V):
        cycle = [(s + 1) % V, *spoiled, s, (s + 2) % V, (s + 3) % V, (s + 4) % V]
        row = [cycle[k % len(cycle)] for k in range(N)]
        if N == 1 and s == 1:
            row = [spoiled[-1]]
        if N == 1 and s == 2:
            row = [s]
        witnesses[s] = row
    return _frozen(dict(name=f"{H}x{W}, {N} witnesses, {ids} ids", clause="w < 0 || w >= V || w == s; the window clipped at the image's corners; p >= hw in the last workgroup",
                        H=H, W=W, V=V, N=N, depth=depth, flags=flags, src=src, wit=wit, times=times, witnesses=witnesses, **VIEW_PARAMS))


@functools.lru_cache(maxsize=None)
def view_exact_case():
    """2 x 4, two views, every number exact: the source pixel (j, i) at depth 1 is the world point (i, j, 1); witness 1 projects it to
    u = i + 1, v = j, so that column 3 lands on u = W exactly (outside) and column 2 on the last column."""
    H, W, V = 2, 4, 2
    depth = np.ones((V, H, W), dtype=F)
    flags = np.ones((V, H, W), dtype=np.uint8)
    eye = np.eye(4)[:3].reshape(-1)
    src = np.stack([np.r_[eye, 1.0, 1.0, 0.5, 0.5]] * V).astype(D)
    wit = np.stack([np.r_[eye, 1.0, 1.0, 0.0, 0.0], np.r_[eye, 1.0, 1.0, 1.0, 0.0]]).astype(D)
    return _frozen(dict(name="2x4 exact", clause="u < (double)W: u == W is outside", H=H, W=W, V=V, N=1, depth=depth, flags=flags, src=src, wit=wit,
                        times=np.zeros(V, dtype=np.int32), witnesses=np.array([[1], [0]], dtype=np.int32), r=0, min_agree=1, max_violate=0,
                        rel_tol=0.0, abs_tol=0.0))


# ------------------------------------------------------------------------------------------------ refusals
# (entry point, what is wrong, the arguments changed — a buffer's name with None (a null pointer) or a number of bytes to move it by, or
# a scalar's name with its value —, a piece of the message).  The GPU test starts from the small valid call of each entry point.
BIG = 1 << 40
_SHAPE = (("no frames", dict(frames=0)), ("65536 frames", dict(frames=65536)), ("H = 0", dict(H=0)), ("W = -1", dict(W=-1)), ("2^24 + 4096 pixels", dict(H=4097, W=4096)))
REFUSALS = tuple(
    [("depth_align_sums", w, ch, "frames of") for w, ch in _SHAPE]
    + [("depth_align_sums", f"no {b}", {b: None}, "null") for b in ("frames_u8", "lidar", "sums")]
    + [("depth_align_solve", f"no {b}", {b: None}, "null") for b in ("sums", "coef", "fitted")]
    + [("depth_align_solve", "no frames", dict(frames=0), "frames"), ("depth_align_solve", "65536 frames", dict(frames=65536), "frames")]
    + [("depth_finish", w, ch, "frames of") for w, ch in _SHAPE]
    + [("depth_finish", f"no {b}", {b: None}, "null") for b in ("frames_u8", "coef", "depth")]
    + [("colormap_spectral", "no values", dict(values=None), "null"), ("colormap_spectral", "neither output", dict(bytes=None, colours=None), "null"),
       ("colormap_spectral", "n = 0", dict(n=0), "values"), ("colormap_spectral", "2^40 values", dict(n=256 * (1 << 31)), "values"),
       ("colormap_spectral", "an empty range", dict(val_min=1.0, val_max=1.0), "range"), ("colormap_spectral", "a reversed range", dict(val_min=1.0, val_max=0.0), "range"),
       ("colormap_spectral", "a range that is not a number", dict(val_max=float("nan")), "range")]
    + [("depth_unproject", w, ch, "frames of") for w, ch in _SHAPE]
    + [("depth_unproject", f"no {b}", {b: None}, "null") for b in ("depth", "rgb", "table", "points", "valid")]
    + [("depth_unproject", "points 8 bytes off", dict(points=8), "unaligned")]
    + [("view_flags", w, ch, "views of") for w, ch in _SHAPE]
    + [("view_flags", f"no {b}", {b: None}, "null") for b in ("depth", "flags")]
    + [("view_consistency", w, ch, "views of") for w, ch in _SHAPE]
    + [("view_consistency", f"no {b}", {b: None}, "null") for b in ("depth", "flags", "src", "wit", "times", "witnesses", "agree", "violate", "keep", "stats")]
    + [("view_consistency", "N = 0", dict(N=0), "witnesses per view"), ("view_consistency", "N = 65", dict(N=65), "witnesses per view"),
       ("view_consistency", "r = -1", dict(r=-1), "radius"), ("view_consistency", "r = 3", dict(r=3), "radius"),
       ("view_consistency", "min_agree = -1", dict(min_agree=-1), "not negative"), ("view_consistency", "max_violate = -1", dict(max_violate=-1), "not negative"),
       ("view_consistency", "rel_tol < 0", dict(rel_tol=-0.5), "tolerances"), ("view_consistency", "abs_tol not a number", dict(abs_tol=float("nan")), "tolerances")]
    + [(e, w, ch, "frames of") for e in ("metric_sse", "metric_ssim", "metric_depth", "metric_confusion") for w, ch in _SHAPE]
    + [("metric_sse", f"no {b}", {b: None}, "null") for b in ("a", "b", "sums")]
    + [("metric_ssim", f"no {b}", {b: None}, "null") for b in ("a", "b", "sums")]
    + [("metric_ssim", "10 rows", dict(H=10), "11 x 11"), ("metric_ssim", "10 columns", dict(W=10), "11 x 11")]
    + [("metric_depth", f"no {b}", {b: None}, "null") for b in ("depth", "lidar", "sums")]
    + [("metric_depth", "min_depth below 2^-6", dict(min_depth=2.0 ** -7), "headroom"), ("metric_depth", "max_depth above 256", dict(max_depth=256.5), "headroom"),
       ("metric_depth", "an empty range", dict(min_depth=5.0, max_depth=5.0), "headroom"), ("metric_depth", "a range that is not a number", dict(min_depth=float("nan")), "headroom")]
    + [("metric_confusion", f"no {b}", {b: None}, "null") for b in ("pred", "gt", "confusion", "bad")]
    + [("metric_confusion", "no classes", dict(classes=0), "classes"), ("metric_confusion", "33 classes", dict(classes=33), "classes")]
    + [(e, f"no {b}", {b: None}, "null") for e in ("cloud_nearest", "cloud_count") for b in ("ref", "keys", "order", "queries")]
    + [(e, w, ch, piece) for e in ("cloud_nearest", "cloud_count") for w, ch, piece in (
        ("the reference 8 bytes off", dict(ref=8), "unaligned"), ("the queries 4 bytes off", dict(queries=4), "unaligned"), ("n = 0", dict(n=0), "reference points"),
        ("nq = 0", dict(nq=0), "reference points"), ("2^40 queries", dict(nq=256 * (1 << 31)), "reference points"), ("r2 = 0", dict(r2=0.0), "squared radius"),
        ("r2 above 4096", dict(r2=4097.0, cell=64.05), "squared radius"), ("r2 not a number", dict(r2=float("nan")), "squared radius"),
        ("a cell of r exactly", dict(cell=0.5), "cell edge"), ("a cell above 64 (1 + 2^-10)", dict(cell=64.07), "cell edge"))]
    + [("cloud_nearest", "no d2", dict(d2=None), "null"), ("cloud_nearest", "no index", dict(index=None), "null"),
       ("cloud_count", "no counts", dict(counts=None), "null"), ("cloud_count", "cap = 0", dict(cap=0), "cap"), ("cloud_count", "cap = -3", dict(cap=-3), "cap")]
    + [("metric_cloud", "no d2", dict(d2=None), "null"), ("metric_cloud", "no sums", dict(sums=None), "null"), ("metric_cloud", "thresholds without a table", dict(t2=None), "null"),
       ("metric_cloud", "n = 0", dict(n=0), "values"), ("metric_cloud", "2^31 values", dict(n=1 << 31), "values"), ("metric_cloud", "K = -1", dict(K=-1), "thresholds"),
       ("metric_cloud", "K = 9", dict(K=9), "thresholds"), ("metric_cloud", "r2 = 0", dict(r2=0.0), "squared radius"), ("metric_cloud", "r2 above 4096", dict(r2=4097.0), "squared radius"),
       ("metric_cloud", "a threshold of 0", dict(t2=(0.0, 0.1)), "squared threshold"), ("metric_cloud", "a threshold above r2", dict(t2=(0.1, 0.3)), "squared threshold"),
       ("metric_cloud", "a threshold that is not a number", dict(t2=(float("nan"), 0.1)), "squared threshold")]
    + [("cloud_sweep", f"no {b}", {b: None}, "bad arguments") for b in ("rays_o", "rays_d", "ranges", "offsets", "l2w", "points", "labels")]
    + [("cloud_sweep", "no frames", dict(frames=0), "frames of"), ("cloud_sweep", "65536 frames", dict(frames=65536), "frames of"),
       ("cloud_sweep", "max_rays = 0", dict(max_rays=0), "frames of"), ("cloud_sweep", "total = 0", dict(total=0), "frames of"),
       ("cloud_sweep", "2^40 rays a frame", dict(max_rays=256 * (1 << 31)), "frames of"), ("cloud_sweep", "ncam = -1", dict(ncam=-1), "cameras"),
       ("cloud_sweep", "nine cameras", dict(ncam=9), "cameras"), ("cloud_sweep", "cameras without a table", dict(cams=None), "cameras"),
       ("cloud_sweep", "cameras without images", dict(images=None), "cameras"), ("cloud_sweep", "image_bytes = 0", dict(image_bytes=0), "cameras"),
       ("cloud_sweep", "nobj = -1", dict(nobj=-1), "objects"), ("cloud_sweep", "objects without a table", dict(objs=None), "objects"),
       ("cloud_sweep", "points 8 bytes off", dict(points=8), "unaligned")]
    + [("cloud_voxel_keys", "no points", dict(points=None), "bad arguments"), ("cloud_voxel_keys", "no keys", dict(keys=None), "bad arguments"),
       ("cloud_voxel_keys", "n = 0", dict(n=0), "bad arguments"), ("cloud_voxel_keys", "2^40 points", dict(n=256 * (1 << 31)), "bad arguments"),
       ("cloud_voxel_keys", "points 4 bytes off", dict(points=4), "bad arguments")]
    + [("cloud_voxel_reduce", f"no {b}", {b: None}, "bad arguments") for b in ("points", "order", "segments", "sums")]
    + [("cloud_voxel_reduce", "n = 0", dict(n=0), "bad arguments"), ("cloud_voxel_reduce", "no voxels", dict(voxels=0), "bad arguments"),
       ("cloud_voxel_reduce", "more voxels than points", dict(voxels=9), "bad arguments"), ("cloud_voxel_reduce", "points 8 bytes off", dict(points=8), "bad arguments")]
    + [("cloud_voxel_finish", "no sums", dict(sums=None), "bad arguments"), ("cloud_voxel_finish", "no output", dict(out=None), "bad arguments"),
       ("cloud_voxel_finish", "no voxels", dict(voxels=0), "bad arguments"), ("cloud_voxel_finish", "output 8 bytes off", dict(out=8), "bad arguments")]
    + [(e, w, dict(voxel=v), "voxel size") for e in ("cloud_voxel_keys", "cloud_voxel_reduce", "cloud_voxel_finish")
       for w, v in (("a voxel of 0", 0.0), ("a negative voxel", -0.5), ("a voxel of 1e30", 1e30), ("a voxel that is not a number", float("nan")))])
ENTRY_POINTS = ("cloud_sweep", "cloud_voxel_keys", "cloud_voxel_reduce", "cloud_voxel_finish", "cloud_nearest", "cloud_count", "metric_cloud",
                "depth_align_sums", "depth_align_solve", "depth_finish", "colormap_spectral", "depth_unproject", "view_flags", "view_consistency",
                "metric_sse", "metric_ssim", "metric_depth", "metric_confusion")
SOURCES = ("cloud.hip", "neighbours.hip", "depth.hip", "consistency.hip", "metrics.hip")
