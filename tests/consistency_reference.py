"""TEST INFRASTRUCTURE: the CPU definition of the cross-view depth-consistency rule, in numpy float64, written from the
rule and not from the kernel.  Every floating-point operation is a single correctly rounded numpy operation in the stated order; the
statistics are Python integers.  Nothing in the product imports it."""
import numpy as np

F = np.float32
D = np.float64
ZNEAR = D(1e-4)
DYNAMIC_MASK = sum(1 << c for c in range(11, 19))
DEFAULTS = dict(r=1, min_agree=2, max_violate=0, rel_tol=0.02, abs_tol=0.2)


def row(m, x, y, z):
    """((m0 x + m1 y) + m2 z) + m3."""
    return ((m[0] * x + m[1] * y) + m[2] * z) + m[3]


def flags(depth, labels=None, sky_label=10, dynamic_mask=DYNAMIC_MASK, min_depth=0.0, max_depth=100.0):
    """(..., H, W) fp32 depths [, int64 labels] -> bytes: bit 0 usable, bit 1 dynamic."""
    z = np.asarray(depth, dtype=F).astype(D)
    with np.errstate(invalid="ignore"):
        usable = (z > D(min_depth)) & (z < D(max_depth))                   # what is not a number is not usable
    dynamic = np.zeros(z.shape, dtype=bool)
    if labels is not None:
        labels = np.asarray(labels, dtype=np.int64)
        usable &= labels != sky_label
        in_mask = (labels >= 0) & (labels < 64)
        bit = np.array([(int(dynamic_mask) >> c) & 1 for c in range(64)], dtype=bool)
        dynamic = in_mask & bit[np.where(in_mask, labels, 0)]
    return usable.astype(np.uint8) | (dynamic.astype(np.uint8) << 1)


def world_points(depth, table):
    """One view: depth (H, W) fp32 and the source row (16 doubles) -> the world point of every pixel, three (H, W) float64 arrays, formed
    as the lifting rule of §14 forms them and not rounded to fp32."""
    H, W = depth.shape
    t = np.asarray(table, dtype=D)
    fx, fy, cx, cy = t[12:]
    z = np.asarray(depth, dtype=F).astype(D)
    xn = ((np.arange(W, dtype=D)[None, :] + D(0.5)) - cx) / fx
    yn = ((np.arange(H, dtype=D)[:, None] + D(0.5)) - cy) / fy
    with np.errstate(invalid="ignore"):                                    # a depth that is not a number: its point is never used
        xc, yc = xn * z, yn * z
        return tuple(row(t[4 * a:4 * a + 4], xc, yc, z) for a in range(3))


def projections(P, active, wit_row, hw):
    """Where the points P land in a witness: (ok, jw, iw, qz) — whether there can be evidence, and the pixel that holds the projection."""
    H, W = hw
    m = np.asarray(wit_row, dtype=D)
    fx, fy, cx, cy = m[12:]
    with np.errstate(all="ignore"):
        qx, qy, qz = row(m[0:4], *P), row(m[4:8], *P), row(m[8:12], *P)
        ok = active & (qz > ZNEAR)
        u = fx * (qx / qz) + cx
        v = fy * (qy / qz) + cy
        ok = ok & (u >= 0) & (u < D(W)) & (v >= 0) & (v < D(H))            # on doubles, before any conversion
        iw = np.where(ok, u, D(0)).astype(np.int64)
        jw = np.where(ok, v, D(0)).astype(np.int64)
    return ok, jw, iw, qz


def verdicts(P, active, same_time, wit_row, depth_w, flags_w, r, rel_tol, abs_tol):
    """The source view's points P against one witness: (agree, violate, counting) — two boolean (H, W) arrays and the number of counting
    window pixels.  active: the source pixels that are tested against this witness."""
    H, W = depth_w.shape
    ok, jw, iw, qz = projections(P, active, wit_row, (H, W))
    with np.errstate(all="ignore"):
        tol = D(abs_tol) + D(rel_tol) * qz
        usable_w = (flags_w & 1) != 0
        counts_w = usable_w if same_time else usable_w & ((flags_w & 2) == 0)
        zw = np.asarray(depth_w, dtype=F).astype(D)
        agrees = np.zeros(ok.shape, dtype=bool)
        counting = np.zeros(ok.shape, dtype=np.int64)
        through = np.zeros(ok.shape, dtype=np.int64)
        for dj in range(-r, r + 1):
            for di in range(-r, r + 1):
                jj, ii = jw + dj, iw + di
                inside = ok & (jj >= 0) & (jj < H) & (ii >= 0) & (ii < W)
                jc, ic = np.clip(jj, 0, H - 1), np.clip(ii, 0, W - 1)
                c = inside & counts_w[jc, ic]
                d = qz - zw[jc, ic]
                counting += c
                agrees |= c & (np.abs(d) <= tol)
                through += c & (d < -tol)
    violates = ~agrees & (counting > 0) & (through == counting)
    return agrees, violates, counting


def consistency(depth, labels, src_table, wit_table, times, witnesses, *, r=1, min_agree=2, max_violate=0, rel_tol=0.02, abs_tol=0.2,
                sky_label=10, dynamic_mask=DYNAMIC_MASK, min_depth=0.0, max_depth=100.0):
    """depth (V, H, W) fp32, labels (V, H, W) int64 or None, the two (V, 16) tables, times (V,), witnesses (V, N) -> dict of "flags",
    "agree", "violate", "keep" (V, H, W) uint8 and "stats" (V, 6) int64, as the product's consistent_views names them."""
    depth = np.asarray(depth, dtype=F)
    V = depth.shape[0]
    times, witnesses = np.asarray(times), np.asarray(witnesses)
    assert r in (0, 1, 2) and times.shape == (V,) and witnesses.shape[0] == V and witnesses.min() >= -1 and witnesses.max() < V
    fl = flags(depth, labels, sky_label, dynamic_mask, min_depth, max_depth)
    agree = np.zeros(depth.shape, dtype=np.int64)
    violate = np.zeros(depth.shape, dtype=np.int64)
    for s in range(V):
        usable, dynamic = (fl[s] & 1) != 0, (fl[s] & 2) != 0
        P = world_points(depth[s], src_table[s])
        for w in witnesses[s]:
            w = int(w)
            if w == -1 or w == s:
                continue
            same_time = bool(times[w] == times[s])
            active = usable if same_time else usable & ~dynamic
            a, b, _ = verdicts(P, active, same_time, wit_table[w], depth[w], fl[w], r, rel_tol, abs_tol)
            agree[s] += a
            violate[s] += b
    usable = (fl & 1) != 0
    keep = usable & (agree >= min_agree) & (violate <= max_violate)
    per_view = lambda a: [int(x) for x in a.reshape(V, -1).sum(axis=1)]
    stats = np.array([per_view(usable), per_view((agree + violate) > 0), per_view(keep), per_view(agree), per_view(violate), per_view(violate > 0)],
                     dtype=np.int64).T
    return {"flags": fl, "agree": agree.astype(np.uint8), "violate": violate.astype(np.uint8), "keep": keep.astype(np.uint8),
            "stats": np.ascontiguousarray(stats)}


def scores(stats):
    """(V, 6) integer sums -> the shares that metrics.view_consistency reports, per view and overall, as Python floats."""
    def one(s):
        usable, tested, kept, sum_agree, _, violated = (int(x) for x in s)
        share = lambda a, b: a / b if b else float("nan")
        return {"tested": share(tested, usable), "kept": share(kept, usable), "violated": share(violated, usable), "mean_agree": share(sum_agree, tested)}
    stats = np.asarray(stats)
    return [one(s) for s in stats], one(stats.sum(axis=0))


# ------------------------------------------------------------------------------------------------ an analytic scene for the tests
GROUND_Y, WALL_Z = 3.0, 12.0                   # world = OpenCV axes (x right, y down, z forward): the ground 3 m below, a wall 12 m ahead
SCENE_INTR = np.array([[64.0, 0, 16.0], [0, 64.0, 0.0], [0, 0, 1]])        # at 24 x 32: the principal point on the top row, the ground in view


def scene_camera(frame, pose):
    """Frame f stands 0.5 f m further forward; pose 0 is 1 m to the left, pose 1 is 1 m to the right and turned 0.05 rad towards the middle."""
    a = 0.0 if pose == 0 else -0.05
    c2w = np.eye(4)
    c2w[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    c2w[:3, 3] = [-1.0 if pose == 0 else 1.0, 0.0, 0.5 * frame]
    return c2w


def scene_depth(c2w, hw, intr=SCENE_INTR):
    """The depth map of the ground and the wall by ray-plane intersection, float64 (H, W): camera-space z of the nearer hit."""
    H, W = hw
    xn = ((np.arange(W) + 0.5) - intr[0, 2]) / intr[0, 0]
    yn = ((np.arange(H) + 0.5) - intr[1, 2]) / intr[1, 1]
    rays = np.stack(np.broadcast_arrays(xn[None, :], yn[:, None], np.ones((H, W))), axis=-1) @ c2w[:3, :3].T        # world directions, per unit depth
    origin = c2w[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        ground = np.where(rays[..., 1] > 0, (GROUND_Y - origin[1]) / rays[..., 1], np.inf)
        wall = np.where(rays[..., 2] > 0, (WALL_Z - origin[2]) / rays[..., 2], np.inf)
    return np.minimum(ground, wall)


def scene_views(hw=(24, 32), frames=3, poses=2):
    """frames x poses views, pose-major as fuse_window_outputs stacks them: (depth (V, H, W) fp32, c2w (V, 4, 4), times (V,), pose ids (V,))."""
    order = [(f, p) for p in range(poses) for f in range(frames)]
    c2w = np.stack([scene_camera(f, p) for f, p in order])
    depth = np.stack([scene_depth(m, hw) for m in c2w]).astype(F)
    return depth, c2w, np.array([f for f, _ in order], dtype=np.int32), np.array([p for _, p in order], dtype=np.int32)
