"""Hand-made inputs for the seven core entry points of the Gaussian splat renderer (csrc/gaussians.hip; csrc/gaussians_bwd.hip,
§24), each naming the clause of the rule it reaches, and the two raw definitions that were missing: `keys_raw` and `ranges_raw` follow
gauss_keys_kernel and gauss_ranges_kernel line by line, spoiled tables included (gr.bin_entries assumes clean ones).  numpy only:
tests/test_gaussians_core_cases_cpu.py asserts, without a GPU, that every case reaches its clause and that the cases tell mutated
definitions apart; tests/test_gaussians_core_kernels_gpu.py runs the kernels on the cases and compares the bits.

  A  full covariances R diag(s^2) R^T (every one of the six entries non-zero), a needle and a pancake among them
  B  one Gaussian per reason the projection drops or keeps it
  C  rect, count and offsets that falsify the guards of gauss_keys_kernel, one owner per copy
  D  sorted keys for gauss_ranges_kernel, also with tiles outside [0, tiles)
  E  uv, conic and depth made by hand for the blends: every branch of blend_step, the batch edges, spoiled values and ranges
  F  count, offsets and partial rows that falsify the guards of with_partials and of gauss_view's depth range
No table holds a NaN where the rule would read one in arithmetic (B's NaN inputs are dropped before any is stored)."""
import functools
from types import SimpleNamespace

import numpy as np

import gaussians_bwd_reference as gb
import gaussians_reference as gr

F = np.float32
NAN = F(np.nan)
IDS = np.array([-3, 0, 1, 2, 7], dtype=np.int32)                                      # -3 -> 0, 7 -> nmat - 1
FULL_N = 300
FULL_SHAPES = (((17, 33), 1), ((17, 33), 3), ((40, 56), 1), ((40, 56), 3))             # (hw, views) of case A
FULL_SEED = 31
NEEDLE, PANCAKE = (0.01, 0.01, 1.5), (0.6, 0.6, 0.004)
TILE_SIZES = (255, 256, 257, 513)


def up(a):
    return np.nextafter(F(a), F(np.inf))


def down(a):
    return np.nextafter(F(a), F(-np.inf))


def upstream(V, hw, seed):
    """Seeded gradients of rgb, depth and alpha, as tests/test_gaussians_bwd_gpu.py draws them."""
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(V, 3) + tuple(hw)).astype(F), (rng.normal(size=(V,) + tuple(hw)) * 0.05).astype(F), rng.normal(size=(V,) + tuple(hw)).astype(F))


def exclusive(count):
    """offsets (V, n) int64 and E of count (V, n)."""
    ends = np.cumsum(count.reshape(-1).astype(np.int64))
    return (ends - count.reshape(-1)).reshape(count.shape), int(ends[-1])


def guarded(ranges, E):
    """ranges with gauss_tile's guard applied: [0, 0) where a tile's range is not one of E entries."""
    ranges = np.asarray(ranges, dtype=np.int32).reshape(-1, 2)
    bad = (ranges[:, 0] < 0) | (ranges[:, 1] > E) | (ranges[:, 0] > ranges[:, 1])
    return np.where(bad[:, None], 0, ranges).astype(np.int32)


# ------------------------------------------------------------------------------------------------ the two raw definitions
def keys_raw(depth, rect, count, offsets, n, V, hw, E):
    """gauss_keys_kernel: keys (E,) int64, values (E,) int32 and the mask of the entries written (the others are not touched)."""
    TX, TY = gr.tiles(hw)
    bits = np.ascontiguousarray(depth, dtype=F).reshape(-1).view(np.uint32).astype(np.int64)
    rect, count, offsets = np.asarray(rect).reshape(-1, 4).astype(np.int32), np.asarray(count).reshape(-1), np.asarray(offsets).reshape(-1)
    keys, values, written = np.zeros(E, np.int64), np.zeros(E, np.int32), np.zeros(E, bool)
    for o in range(V * n):
        c = int(count[o])
        if c <= 0: continue
        x0, x1, y0, y1 = (int(t) for t in rect[o])                                     # the words read as signed
        if x0 < 0: continue
        if x1 > TX: continue
        if x0 >= x1: continue
        if y0 < 0: continue
        if y1 > TY: continue
        if y0 >= y1: continue
        if (x1 - x0) * (y1 - y0) != c: continue
        at = int(offsets[o])
        if at < 0: continue
        if at > E - c: continue
        view, index = divmod(o, n)
        e = at
        for ty in range(y0, y1):
            for tx in range(x0, x1):
                keys[e] = ((view * TX * TY + ty * TX + tx) << 32) | int(bits[o])
                values[e] = index
                written[e] = True
                e += 1
    return keys, values, written


def ranges_raw(keys, E, tiles):
    """mudg_gauss_ranges: zeros, then gauss_ranges_kernel's two stores per entry whose tile lies in [0, tiles).  (tiles, 2) int32."""
    out = np.zeros(2 * tiles, np.int32)
    tile = np.asarray(keys, dtype=np.int64) >> 32                                      # arithmetic, as the kernel's shift of a long long
    for e in range(E):
        t = int(tile[e])
        if t < 0: continue
        if t >= tiles: continue
        if e == 0 or tile[e - 1] != t:
            out[2 * t] = e
        if e == E - 1 or tile[e + 1] != t:
            out[2 * t + 1] = e + 1
    return out.reshape(tiles, 2)


def blend_bytes(proj, words, values, ranges, hw):
    """gr.blend behind gauss_tile's range guard and stage_batch's value guard (a sorted value outside the cloud is an entry of zeros):
    rgb, depth, alpha and walked (V NT,) int32, the entries each workgroup staged (whole batches until every pixel is done)."""
    V, n = proj["count"].shape
    E = len(values)
    padded = {k: np.concatenate([proj[k], np.zeros((V, 1) + proj[k].shape[2:], proj[k].dtype)], axis=1) for k in ("uv", "conic", "depth", "count")}
    values = np.where((values < 0) | (values >= n), n, values)
    ranges = guarded(ranges, E)
    rgb, depth, alpha, looked = gr.blend(padded, np.concatenate([words, np.zeros(1, words.dtype)]), values, ranges, hw)
    walked = np.minimum(ranges[:, 1] - ranges[:, 0], 256 * ((looked + 255) // 256)).astype(np.int32)
    return rgb, depth, alpha, walked


# ------------------------------------------------------------------------------------------------ A: full covariances
def rotations(rng, n):
    q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    return q


def full_covariances(rot, s):
    """R diag(s^2) R^T in float64, rounded once: (n, 6) fp32."""
    m = rot * np.asarray(s, dtype=np.float64)[:, None, :]
    full = m @ m.transpose(0, 2, 1)
    return np.stack([full[:, 0, 0], full[:, 0, 1], full[:, 0, 2], full[:, 1, 1], full[:, 1, 2], full[:, 2, 2]], axis=1).astype(F)


def _more_views(mats, views, seed):
    rng = np.random.default_rng(seed + 100)
    more = [mats[0]]
    for _ in range(views - 1):
        a, b = rng.uniform(-0.2, 0.2, 2)
        more.append(np.array([[np.cos(a), 0, np.sin(a), b, 0, 1, 0, 0.1, -np.sin(a), 0, np.cos(a), 1.0 + b]], dtype=F))
    return np.stack(more)


@functools.lru_cache(maxsize=None)
def full_case(hw, views, with_ids=True, seed=FULL_SEED, n=FULL_N):
    """gr.seeded_scene's positions, colours, opacities and camera; covariances R diag(s^2) R^T with seeded rotations and s uniform in
    (0.03, 0.5) metres (the scene's unit; its own isotropic scales are 0.05 .. 0.4), Gaussian 0 a needle and Gaussian 1 a pancake in the
    middle of the view; with_ids: three matrices a view as test_gaussians_gpu.py's _ids_case builds them (the scene's, one shifted by
    0.5 m, the views reversed; view 0 does not show id 1) and ids from {-3, 0, 1, 2, 7}."""
    xyz, rgb, _, op, mats, cam = gr.seeded_scene(n, hw, seed)
    rng = np.random.default_rng(seed + 200)
    s = rng.uniform(0.03, 0.5, (n, 3))
    s[0], s[1] = NEEDLE, PANCAKE
    xyz[0], xyz[1] = (0.1, 0.05, 6.0), (-0.3, 0.1, 9.0)
    c = SimpleNamespace(hw=hw, V=views, n=n, clause="full covariances", scales=s)
    c.xyz, c.rgb, c.opacity, c.cam = xyz, rgb, op, cam
    c.cov = full_covariances(rotations(rng, n), s)
    mats = _more_views(mats, views, seed)
    if with_ids:
        c.ids = rng.choice(IDS, n).astype(np.int32)
        c.ids[0], c.ids[1] = 0, 7
        shifted = mats.copy()
        shifted[:, 0, 3] += F(0.5)
        c.mats = np.ascontiguousarray(np.stack([mats[:, 0], shifted[:, 0], mats[::-1, 0]], axis=1))
        c.mats[0, 1] = 0
    else:
        c.ids, c.mats = None, mats
    c.nmat = c.mats.shape[1]
    c.pts = gr.pack(xyz, rgb)
    c.colour = rng.uniform(0.0, 255.0, (n, 3)).astype(F)
    c.ups = upstream(views, hw, seed + 300)
    return c


@functools.lru_cache(maxsize=None)
def flat_full_case(n=257, seed=41):
    """n anisotropic Gaussians in front of the flat camera whose centres lie on tile 0 of a 17 x 33 image: the blends' batch edge."""
    rng = np.random.default_rng(seed)
    pts, _, _ = gr.flat_case(rng.uniform(5.0, 11.0, (n, 2)), 0.5, z=rng.uniform(60.0, 180.0, n).astype(F), seed=seed)
    c = SimpleNamespace(hw=(17, 33), V=1, n=n, clause=f"{n} anisotropic Gaussians on one tile", ids=None, mats=gr.FLAT[None].copy(), nmat=1, cam=gr.FLAT_CAM)
    c.pts = pts
    c.xyz, _ = gr.unpack(pts)
    c.scales = rng.uniform(0.1, 0.9, (n, 3))
    c.cov = full_covariances(rotations(rng, n), c.scales)
    c.opacity = rng.uniform(0.01, 0.05, n).astype(F)
    c.colour = rng.uniform(0.0, 255.0, (n, 3)).astype(F)
    c.ups = upstream(1, c.hw, seed + 300)
    return c


@functools.lru_cache(maxsize=None)
def full_definition(c_key):
    """The definition's answer on a case of A (c_key: the arguments of full_case, or "flat"): gb.render_backward's dict with the byte
    render's keys, images and walked added as keys, rgb8, depth8, alpha8, walked8."""
    c = flat_full_case() if c_key == "flat" else full_case(*c_key)
    want = gb.render_backward(c.xyz, c.colour, c.cov, c.opacity, c.ids, c.mats, c.cam, c.hw, *c.ups)
    proj = {k: want[k] for k in ("uv", "conic", "depth", "rect", "count")}
    keys, values, ranges = gr.bin_entries(proj, c.hw)
    assert np.array_equal(values, want["values"]) and np.array_equal(ranges, want["ranges"])
    rgb8, depth8, alpha8, walked8 = blend_bytes(proj, gr.unpack(c.pts)[1], values, ranges, c.hw)
    want.update(keys=keys, rgb8=rgb8, depth8=depth8, alpha8=alpha8, walked8=walked8, proj=proj, E=want["entries"])
    return want


# ------------------------------------------------------------------------------------------------ B: what the projection drops
def largest_kept_scale():
    """The largest fp32 scale s for which gr.project keeps gr.isotropic(s) at (8.5, 8.5), z = FOCAL, on a 16 x 16 image, by bisection on
    the bits between 1000 (kept) and 2000 (dropped); its rad, the next scale up and that one's rad (`radius`)."""
    pts = gr.flat_case([[8.5, 8.5]], 0.5)[0]
    kept = lambda s: gr.project(gr.unpack(pts)[0], gr.isotropic(s, 1), np.ones(1, F), None, gr.FLAT[None], gr.FLAT_CAM, (16, 16))["count"][0, 0] > 0
    lo, hi = int(F(1000.0).view(np.uint32)), int(F(2000.0).view(np.uint32))
    assert kept(F(1000.0)) and not kept(F(2000.0))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if kept(np.uint32(mid).view(F)):
            lo = mid
        else:
            hi = mid
    lo, hi = np.uint32(lo).view(F), np.uint32(hi).view(F)
    return lo, radius(lo), hi, radius(hi)


def radius(scale, centre=(8.5, 8.5)):
    """rad of one isotropic Gaussian at `centre`, z = FOCAL, in front of the flat camera: gr.project does not return it, so §23's steps
    6 - 9 are repeated here in its arithmetic (the qx the Jacobian sees is inside the limit for this centre on every image of B)."""
    with np.errstate(all="ignore"):
        fx = F(gr.FOCAL)
        z = F(gr.FOCAL)
        x, y = F(centre[0]) * z / fx, F(centre[1]) * z / fx
        zz = z * z
        s2 = F(scale) * F(scale)
        j00, j02, j12 = fx / z, -((fx * ((x / z) * z)) / zz), -((fx * ((y / z) * z)) / zz)
        t0, t1 = (j00, F(0), j02), (F(0), j00, j12)
        v0, v1 = [t * s2 for t in t0], [t * s2 for t in t1]
        a = ((v0[0] * t0[0] + v0[1] * t0[1]) + v0[2] * t0[2]) + gr.BLUR
        b = (v0[0] * t1[0] + v0[1] * t1[1]) + v0[2] * t1[2]
        c = ((v1[0] * t1[0] + v1[1] * t1[1]) + v1[2] * t1[2]) + gr.BLUR
        det = a * c - b * b
        mid = F(0.5) * (a + c)
        lam = mid + np.sqrt(np.fmax(F(0.1), mid * mid - det))
        return np.ceil(F(3.0) * np.sqrt(lam))


largest_kept_scale = functools.lru_cache(maxsize=None)(largest_kept_scale)


@functools.lru_cache(maxsize=None)
def drop_case(hw):
    """One Gaussian per clause in front of the flat camera (matrix 0 the identity, 1 the zero matrix, 2 the identity moved 2 m along x;
    znear 0.2, zfar 200).  Unless its clause says otherwise a Gaussian is isotropic with scale 0.5 (rad 3) at (8.5, 8.5), z = FOCAL, opaque,
    id 0.  c.clauses[i] names Gaussian i, c.drawn[i] is whether the rule keeps it, c.tiles[i] its count where the clause fixes one."""
    H, W = hw
    TX, TY = gr.tiles(hw)
    kept, _, dropped, _ = largest_kept_scale()
    rows = []

    def add(clause, drawn, tiles=None, centre=(8.5, 8.5), z=gr.FOCAL, cov=None, scale=0.5, op=1.0, gid=0, xyz=None):
        rows.append(SimpleNamespace(clause=clause, drawn=drawn, tiles=tiles, centre=centre, z=z, cov=cov, scale=scale, op=op, gid=gid, xyz=xyz))

    add("plain", True, 1)
    add("zc == znear", False, z=F(gr.ZNEAR))
    add("zc one ulp above znear", True, z=up(gr.ZNEAR))
    add("zc == zfar", False, z=F(gr.ZFAR))
    add("zc one ulp below zfar", True, z=down(gr.ZFAR))
    add("z is not a number", False, xyz=(8.5, 8.5, np.nan))
    add("x is not a number, zc finite: u is not a number and both ends of the rectangle clamp to 0", False, xyz=(np.nan, 8.5, gr.FOCAL))
    add("x = +inf: 0 x inf makes zc not a number", False, xyz=(np.inf, 8.5, gr.FOCAL))
    add("det <= 0", False, cov=[1.0, 0.0, 0.0, -1.0, 0.0, 1.0])
    add("an infinite covariance entry", False, cov=[np.inf, 0.0, 0.0, 0.25, 0.0, 0.25])
    add("a covariance entry that is not a number", False, cov=[0.25, np.nan, 0.0, 0.25, 0.0, 0.25])
    add("the largest rad <= 4096", True, TX * TY, scale=kept)
    add("the next scale up: rad > 4096", False, scale=dropped)
    add("opacity one ulp below 1 / 255", False, op=down(gr.MIN_ALPHA))
    add("opacity exactly 1 / 255", True, 1, op=gr.MIN_ALPHA)
    add("opacity not a number", False, op=np.nan)
    add("opacity +inf", False, op=np.inf)
    add("opacity -1", False, op=-1.0)
    add("opacity 0", False, op=0.0)
    add("opacity 1", True, 1, op=1.0)
    for k, centre in enumerate(((1e30, 8.0), (-1e30, 8.0), (8.0, 1e30), (8.0, -1e30))):
        add(f"centre at {'+-'[k % 2]}1e30 along {'xy'[k // 2]}", False, centre=centre)
    add("left of the image by less than rad", True, 1, centre=(-2.0, 8.0))
    add("left of the image by more than rad", False, centre=(-4.0, 8.0))
    add("right of the tile grid by less than rad", True, 1, centre=(16.0 * TX + 2.0, 8.0))
    add("right of the tile grid by more than rad", False, centre=(16.0 * TX + 3.5, 8.0))
    add("above the image by less than rad", True, 1, centre=(8.0, -2.0))
    add("above the image by more than rad", False, centre=(8.0, -4.0))
    add("below the tile grid by less than rad", True, 1, centre=(8.0, 16.0 * TY + 2.0))
    add("below the tile grid by more than rad", False, centre=(8.0, 16.0 * TY + 3.5))
    add("a centre on a tile corner", True, min(2, TX) * min(2, TY), centre=(16.0, 16.0))
    add("one Gaussian over every tile", True, TX * TY, centre=(W / 2.0, H / 2.0), scale=60.0)
    add("mid^2 - det below the 0.1 floor", True, cov=[0.8, 0.0, 0.0, 0.2, 0.0, 0.25])
    add("mid^2 - det above the 0.1 floor", True, cov=[0.85, 0.0, 0.0, 0.2, 0.0, 0.25])
    add("id -3 is matrix 0", True, 1, gid=-3)
    add("id 1: the zero matrix, zc = 0", False, gid=1)
    add("id nmat + 4 is matrix nmat - 1", True, 1, gid=7)
    n = len(rows)
    c = SimpleNamespace(hw=hw, V=1, n=n, nmat=3, cam=gr.FLAT_CAM, clauses=[r.clause for r in rows], drawn=np.array([r.drawn for r in rows]),
                        tiles=[r.tiles for r in rows], clause="one Gaussian per drop clause")
    z = np.array([r.z for r in rows], dtype=F)
    centres = np.array([r.centre for r in rows], dtype=F)
    with np.errstate(all="ignore"):
        c.xyz = np.stack([centres[:, 0] * z / F(gr.FOCAL), centres[:, 1] * z / F(gr.FOCAL), z], axis=1).astype(F)
    c.cov = np.concatenate([gr.isotropic(r.scale, 1) if r.cov is None else np.array([r.cov], dtype=F) for r in rows])
    for i, r in enumerate(rows):
        if r.xyz is not None:
            c.xyz[i] = r.xyz
    c.opacity = np.array([r.op for r in rows], dtype=F)
    c.ids = np.array([r.gid for r in rows], dtype=np.int32)
    moved = gr.FLAT[0].copy()
    moved[3] = 2.0
    c.mats = np.stack([gr.FLAT[0], np.zeros(12, F), moved])[None]
    c.pts = gr.pack(c.xyz, np.random.default_rng(n).integers(0, 256, (n, 3), dtype=np.uint8))
    return c


def project_case(c):
    return gr.project(c.xyz, c.cov, c.opacity, c.ids, c.mats, c.cam, c.hw)


# ------------------------------------------------------------------------------------------------ C: tables that gauss_keys_kernel refuses
KEY_HW, KEY_VIEWS = (40, 56), 3
KEY_TERMS = ("c <= 0", "x0 < 0", "x1 > TX", "x0 >= x1", "y0 < 0", "y1 > TY", "y0 >= y1", "area != c", "at < 0", "at > E - c")


def key_terms(rect, count, offsets, o, hw, E):
    """The guard terms of gauss_keys_kernel that owner o falsifies."""
    TX, TY = gr.tiles(hw)
    x0, x1, y0, y1 = (int(t) for t in rect.reshape(-1, 4)[o])
    c, at = int(count.reshape(-1)[o]), int(offsets.reshape(-1)[o])
    checks = (c <= 0, x0 < 0, x1 > TX, x0 >= x1, y0 < 0, y1 > TY, y0 >= y1, (x1 - x0) * (y1 - y0) != c, at < 0, at > E - c)
    return {t for t, hit in zip(KEY_TERMS, checks) if hit}


@functools.lru_cache(maxsize=None)
def key_cases():
    """The clean tables of case A at 40 x 56 with three views, and one copy per guard term with one owner spoiled: a dict name ->
    (case, owner).  A case: depth, rect (int32, the word 0x80000000 as -2^31), count, offsets, n, V, hw, E, clause, terms (what the owner
    falsifies).  The owners are drawn pairs away from the last entries, so a definition without a guard stays inside [0, E) on the CPU."""
    a = full_case(KEY_HW, KEY_VIEWS)
    proj = full_definition((KEY_HW, KEY_VIEWS))["proj"]
    TX, TY = gr.tiles(KEY_HW)
    offsets, E = exclusive(proj["count"])
    clean = SimpleNamespace(depth=proj["depth"], rect=proj["rect"].astype(np.int32), count=proj["count"], offsets=offsets, n=a.n, V=a.V, hw=KEY_HW,
                            E=E, clause="clean", terms=set())
    flat_count, flat_rect, flat_off = clean.count.reshape(-1), clean.rect.reshape(-1, 4), offsets.reshape(-1)
    last = int(np.nonzero(flat_count)[0][-1])
    inner = [o for o in np.nonzero(flat_count)[0] if flat_off[o] + 4 * TX * TY < E]   # room for any rectangle a mutant would follow
    narrow = [o for o in inner if flat_rect[o, 1] < TX and flat_rect[o, 3] < TY]      # a rectangle that may grow by a column or a row
    cases = {}

    def spoil(name, o, terms, rect=None, count=None, offset=None):
        c = SimpleNamespace(**vars(clean))
        c.rect, c.count, c.offsets = clean.rect.copy(), clean.count.copy(), clean.offsets.copy()
        if rect is not None:
            c.rect.reshape(-1, 4)[o] = rect
        if count is not None:
            c.count.reshape(-1)[o] = count
        if offset is not None:
            c.offsets.reshape(-1)[o] = offset
        c.clause, c.terms = name, set(terms)
        cases[name] = (c, int(o))

    x0, x1, y0, y1 = (int(t) for t in flat_rect[narrow[0]])
    area = lambda r: (r[1] - r[0]) * (r[3] - r[2])
    spoil("count 0 with a valid rectangle", inner[3], ("c <= 0", "area != c"), count=0)
    spoil("count -2 with a valid rectangle", inner[5], ("c <= 0", "area != c"), count=-2)
    o = inner[7]
    r = flat_rect[o].tolist()
    spoil("x0 >= x1", o, ("x0 >= x1", "area != c"), rect=[r[1], r[1], r[2], r[3]])
    spoil("both ends swapped: the area is the count", inner[9], ("x0 >= x1", "y0 >= y1"), rect=flat_rect[inner[9]][[1, 0, 3, 2]].tolist())
    o = narrow[0]
    grown = [x0, TX + 1, y0, y1]
    spoil("x1 = TX + 1, the count the larger rectangle's", o, ("x1 > TX",), rect=grown, count=area(grown))
    spoil("x1 = 0x80000000 as a word", inner[11], ("x0 >= x1", "area != c"), rect=[flat_rect[inner[11], 0], -2 ** 31, flat_rect[inner[11], 2], flat_rect[inner[11], 3]])
    o = inner[13]
    r = flat_rect[o].tolist()
    spoil("y0 >= y1", o, ("y0 >= y1", "area != c"), rect=[r[0], r[1], r[3], r[3]])
    grown = [x0, x1, y0, TY + 1]
    spoil("y1 = TY + 1, the count the larger rectangle's", narrow[0], ("y1 > TY",), rect=grown, count=area(grown))
    grown = [-1, x1, y0, y1]
    spoil("x0 = -1, the count the larger rectangle's", narrow[0], ("x0 < 0",), rect=grown, count=area(grown))
    grown = [x0, x1, -1, y1]
    spoil("y0 = -1, the count the larger rectangle's", narrow[0], ("y0 < 0",), rect=grown, count=area(grown))
    spoil("count off by one from the rectangle's area", inner[15], ("area != c",), count=int(flat_count[inner[15]]) + 1)
    spoil("offset -1", next(o for o in inner[17:] if flat_count[o] >= 2), ("at < 0",), offset=-1)
    spoil("offset E - count + 1", last, ("at > E - c",), offset=E - int(flat_count[last]) + 1)
    spoil("offset exactly E - count: accepted", last, (), offset=E - int(flat_count[last]))             # where the last owner already is
    return clean, cases


def keys_definition(c):
    return keys_raw(c.depth, c.rect, c.count, c.offsets, c.n, c.V, c.hw, c.E)


# ------------------------------------------------------------------------------------------------ D: sorted keys for gauss_ranges_kernel
def _keys_of(tiles_of_entries, seed):
    """Sorted keys whose entries lie on the given (non-decreasing) tiles, the depth bits seeded and ascending inside a tile."""
    rng = np.random.default_rng(seed)
    tile = np.asarray(tiles_of_entries, dtype=np.int64)
    assert (np.diff(tile) >= 0).all()
    bits = rng.uniform(0.5, 100.0, len(tile)).astype(F).view(np.uint32).astype(np.int64)
    keys = (tile << 32) | bits
    keys = np.sort(keys, kind="stable")
    assert np.array_equal(keys >> 32, tile)
    return keys


@functools.lru_cache(maxsize=None)
def range_cases():
    """name -> (keys, E, tiles, clause)."""
    out = {}
    out["one entry"] = (_keys_of([3], 1), 1, 6)
    out["one tile holds everything"] = (_keys_of([2] * 300, 2), 300, 6)
    out["the first and the last tile, nothing between"] = (_keys_of([0] * 255 + [11] * 3, 3), 258, 12)
    rng = np.random.default_rng(4)
    inside = np.sort(rng.choice([0, 1, 2, 3, 4, 6, 7, 9, 10], 560))                  # tiles 5, 8 and 11 stay [0, 0)
    tile = np.concatenate([[-7] * 3, [-1] * 4, inside, [12] * 5, [40] * 2, [2 ** 31 - 1]])
    out["tiles below 0 in front and tiles >= tiles behind"] = (_keys_of(tile, 4), len(tile), 12)
    return out


# ------------------------------------------------------------------------------------------------ E: hand-made tables for the blends
# clause, u, v, A, B, C, opacity on a 16 x 16 tile whose first pixel centre is (0.5, 0.5)
SPECIAL = (
    ("A, C < 0: p > 0 at every pixel", 8.25, 7.75, -0.05, 0.0, -0.05, 0.9),
    ("p crosses MIN_POWER inside the tile", 6.5, 9.5, 0.2, 0.05, 0.2, 0.6),
    ("opacity E(p) crosses 1 / 255", 8.5, 8.5, 0.02, 0.0, 0.02, 0.01),
    ("raw > 0.99 near the centre: capped", 4.5, 4.5, 0.01, 0.0, 0.02, 1.0),
    ("the centre on a pixel centre: p = 0, E = 1", 10.5, 5.5, 0.3, 0.1, 0.3, 0.5),
    ("only the rows of wave 0 blend it", 8.0, 1.5, 0.001, 0.0, 3.0, 0.5),
) + tuple((f"opaque {k}: T (1 - alpha) < 1e-4 ends pixels at different entries", 7.0 + 0.5 * k, 9.0 - 0.5 * k, 0.05, 0.01, 0.05, 0.95) for k in range(6))


@functools.lru_cache(maxsize=None)
def table_case(hw, n, seed=51):
    """n hand-made entries of one view on a 16 x 16 or a 17 x 33 image, every entry listed on every tile in depth order: SPECIAL in front
    (on the first tile), then seeded faint entries with positive definite conics.  proj (uv, conic, depth and a count that only carries
    the shape), colour (n, 3), packed points with colour words, values, order (a seeded permutation: where each partial lands), ranges,
    upstream gradients; spoiled: values with -5 and n, ranges with start < 0, end = E + 1 and start > end on three tiles (on a single tile:
    ranges left clean, or nothing would run)."""
    H, W = hw
    TX, TY = gr.tiles(hw)
    NT = TX * TY
    rng = np.random.default_rng(seed + n)
    k = len(SPECIAL)
    assert n > k
    A, C = rng.uniform(0.02, 0.3, n), rng.uniform(0.02, 0.3, n)
    B = rng.uniform(-0.5, 0.5, n) * np.sqrt(A * C)
    u, v, op = rng.uniform(0.0, W, n), rng.uniform(0.0, H, n), rng.uniform(0.01, 0.05, n)
    depth = np.sort(rng.uniform(20.0, 100.0, n))
    for i, (_, su, sv, sA, sB, sC, sop) in enumerate(SPECIAL):
        u[i], v[i], A[i], B[i], C[i], op[i], depth[i] = su, sv, sA, sB, sC, sop, 1.0 + i
    t = SimpleNamespace(hw=hw, V=1, n=n, E=NT * n, clause=f"{n} hand-made entries on each of {NT} tiles", clauses=[s[0] for s in SPECIAL])
    t.proj = dict(uv=np.stack([u, v], axis=1).astype(F)[None], conic=np.stack([A, B, C, op], axis=1).astype(F)[None], depth=depth.astype(F)[None],
                  count=np.full((1, n), NT, np.int32))
    t.colour = rng.uniform(0.0, 255.0, (n, 3)).astype(F)
    t.pts = gr.pack(rng.normal(size=(n, 3)).astype(F), rng.integers(0, 256, (n, 3), dtype=np.uint8))
    t.words = gr.unpack(t.pts)[1]
    t.values = np.tile(np.arange(n, dtype=np.int32), NT)                              # depth ascends with the index
    t.ranges = np.stack([np.arange(NT) * n, (np.arange(NT) + 1) * n], axis=1).astype(np.int32)
    t.order = rng.permutation(t.E).astype(np.int64)
    t.ups = upstream(1, hw, seed + 300 + n)
    values = t.values.copy()
    values[k::7], values[k + 3::11] = -5, n                                           # the specials of the first tile stay
    ranges = t.ranges.copy()
    if NT >= 6:
        ranges[1], ranges[2], ranges[4] = (-4, 3), (0, t.E + 1), (5 * n, 4 * n)
    t.spoiled = (values, t.order, ranges)
    return t


@functools.lru_cache(maxsize=None)
def table_definition(hw, n, spoiled=False):
    """rgb, depth, alpha, state, partial of the float blends and rgb8, depth8, alpha8, walked8 of the byte blend on a table."""
    t = table_case(hw, n)
    values, order, ranges = t.spoiled if spoiled else (t.values, t.order, t.ranges)
    rgb, depth, alpha, state = gb.blend_train(t.proj, t.colour, values, guarded(ranges, t.E), hw)
    partial = gb.blend_bwd(t.proj, t.colour, values, order, ranges, hw, state, *t.ups)
    rgb8, depth8, alpha8, walked8 = blend_bytes(t.proj, t.words, values, ranges, hw)
    return SimpleNamespace(rgb=rgb, depth=depth, alpha=alpha, state=state, partial=partial, rgb8=rgb8, depth8=depth8, alpha8=alpha8, walked8=walked8)


BRANCHES = ("p > 0", "p < MIN_POWER", "alpha < 1 / 255", "ends", "blends capped", "blends free")


def blend_trace(t, tile=0):
    """What each entry of `tile` does at each of the tile's live pixels, from the definition's step: (entries, len(BRANCHES)) pixel counts,
    and per entry the set of waves with a pixel that blends it."""
    H, W = t.hw
    TX, _ = gr.tiles(t.hw)
    _, _, inside, px, py = gb._lanes(tile, TX, H, W)
    T, done = np.ones(256, F), ~inside
    lo, hi = (int(x) for x in t.ranges[tile])
    counts, waves = np.zeros((hi - lo, len(BRANCHES)), np.int64), []
    with np.errstate(all="ignore"):
        for row, e in enumerate(range(lo, hi)):
            ent = gb._entry(t.proj, t.colour, 0, int(t.values[e]), t.n)
            dx, dy = ent[0] - px, ent[1] - py
            p = (F(-0.5) * ((ent[2] * dx) * dx + (ent[4] * dy) * dy)) - (ent[3] * dx) * dy
            _, _, _, raw, al, _, Tn, skip = gb._step(ent, px, py, T)
            live = ~done
            first = live & (p > 0)
            second = live & ~first & (p < gr.MIN_POWER)
            third = live & skip & ~first & ~second
            ends = live & ~skip & (Tn < gr.MIN_T)
            add = live & ~skip & ~ends
            capped = add & (raw > gr.MAX_ALPHA)
            counts[row] = [first.sum(), second.sum(), third.sum(), ends.sum(), capped.sum(), (add & ~capped).sum()]
            waves.append(set((np.nonzero(add)[0] // 64).tolist()))
            done = done | ends
            T = np.where(add, Tn, T)
    return counts, waves


# ------------------------------------------------------------------------------------------------ F: tables that with_partials refuses
@functools.lru_cache(maxsize=None)
def gather_cases():
    """Case A at 40 x 56 with three views and its definition's partial buffer; name -> (count, offsets, partial, clause's owner (view, g)).
    The clean tables are "clean"."""
    a = full_case(KEY_HW, KEY_VIEWS)
    want = full_definition((KEY_HW, KEY_VIEWS))
    count, offsets, partial, E = want["count"], want["offsets"], want["partial"], want["E"]
    proj = want["proj"]
    drawn = [(int(v), int(g)) for v, g in zip(*np.nonzero(count)) if offsets[v, g] + count[v, g] + 2 < E and partial[offsets[v, g]:offsets[v, g] + count[v, g] + 1].any()]
    hidden = [int(g) for g in np.nonzero((np.clip(a.ids, 0, a.nmat - 1) == 1) & (count[1] > 0))[0]]       # view 0: the zero matrix, zc = 0
    out = {"clean": (count, offsets, partial, None)}

    def spoil(name, owner, cnt=None, off=None, rows=None):
        c, o, p = count.copy(), offsets.copy(), partial
        if cnt is not None:
            c[owner] = cnt
        if off is not None:
            o[owner] = off
        if rows is not None:
            p = partial.copy()
            p[rows] = NAN
        out[name] = (c, o, p, owner)

    g = hidden[0]
    spoil("a count that says drawn where zc is out of range", (0, g), cnt=count[1, g], off=offsets[1, g])
    spoil("count 0 where it was drawn", drawn[10], cnt=0)
    # an owner for which a definition that followed offset -1 (on the CPU: the last row, then the first ones) would add something
    spoil("offset -1", next(o for o in drawn[20:] if count[o] >= 2 and partial[np.arange(-1, count[o] - 1)].any()), off=-1)
    spoil("offset E - count + 1", drawn[30], off=E - int(count[drawn[30]]) + 1)
    spoil("a count one larger: the neighbour's row is added", drawn[40], cnt=int(count[drawn[40]]) + 1)
    o = drawn[50]
    spoil("rows that are not a number where no valid (offset, count) reaches", o, cnt=0, rows=slice(int(offsets[o]), int(offsets[o]) + int(count[o])))
    return out


def gather_zfar():
    """A zfar for the backward alone that is exactly the zc of a Gaussian drawn in view 0, the median of that view's: the clean tables then
    say drawn for every pair at or beyond it, and gauss_view refuses them (zc == zfar included).  Returns (zfar, that Gaussian)."""
    want = full_definition((KEY_HW, KEY_VIEWS))
    seen = np.nonzero(want["count"][0])[0]
    g = int(seen[np.argsort(want["depth"][0, seen], kind="stable")[len(seen) // 2]])
    return F(want["depth"][0, g]), g


def gather_definition(name, zfar=gr.ZFAR):
    a = full_case(KEY_HW, KEY_VIEWS)
    count, offsets, partial, _ = gather_cases()[name]
    return gb.project_bwd(a.xyz, a.cov, a.ids, a.mats, a.cam, a.hw, count, offsets, partial, zfar=zfar)
