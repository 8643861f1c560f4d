"""TEST INFRASTRUCTURE: the inputs that the CPU and the GPU tests of the LiDAR depth maps share, each made once per process, with what
the definition (tests/lidar_depth_reference.py) gives for them."""
import functools

import numpy as np

import lidar_depth_reference as ld

F = np.float32
IDENTITY = np.eye(4)[:3].astype(F)

# ---- the plane lemma: 20 000 points of the camera-space plane through (0, 0, 10) with normal (0.5, 0.3, 1), seen at 160 x 240, f = 144
PLANE_HW, PLANE_F, PLANE_REL_TOL = (160, 240), 144.0, 0.05
PLANE_K = np.array([[PLANE_F, 0.0, PLANE_HW[1] / 2.0], [0.0, PLANE_F, PLANE_HW[0] / 2.0], [0.0, 0.0, 1.0]])
REACHES = (1, 4, 8, 16)


@functools.lru_cache(maxsize=None)
def plane_points():
    rng = np.random.default_rng(2020)
    H, W = PLANE_HW
    u, v = rng.uniform(-2.0, W + 2.0, 20000), rng.uniform(-2.0, H + 2.0, 20000)          # a little beyond every border
    xn, yn = (u - W / 2.0) / PLANE_F, (v - H / 2.0) / PLANE_F
    w = (1.0 + 0.5 * xn + 0.3 * yn) / 10.0                                               # inverse depth: affine in (u, v)
    step = (0.5 + 0.3) / 10.0 / PLANE_F                                                  # |dw/du| + |dw/dv|
    assert w.min() > 0 and step / w.min() <= 0.014 < PLANE_REL_TOL
    z = 1.0 / w
    return np.stack([xn * z, yn * z, z], axis=1).astype(F)


# ---- the leak scene: static boxes in front of the ground and the walls, six sweeps pooled at the last frame
LEAK_SCENE = dict(frames=6, beams=64, azimuths=1325, n_objects=0, n_static=4, n_other=0, seed=0)
LEAK_CAMERA, LEAK_FRAME, LEAK_HW = "camera_FRONT", 5, (320, 480)


@functools.lru_cache(maxsize=None)
def leak_scene():
    from mudg_amd.synthetic import street_sweeps
    return street_sweeps(**LEAK_SCENE)


@functools.lru_cache(maxsize=None)
def leak_sweeps():
    scenario, load_lidar, load_image = leak_scene()
    assert not [o for o in scenario["objects"].values() if ld.cr.is_object_motion(*ld.cr.object_tables(o, LEAK_SCENE["frames"])[::2])]
    return ld.frame_sweeps(scenario, load_lidar, load_image, [])


@functools.lru_cache(maxsize=None)
def leak_maps(frame=LEAK_FRAME):
    """(the analytic depth, the definition's map without the filter, with it) at the camera's own size."""
    scenario = leak_scene()[0]
    data = scenario["observers"][LEAK_CAMERA]["data"]
    xyz, mats = ld.candidates([s[0] for s in leak_sweeps()], None, None, None, data["c2w"][frame], frame)
    cam = ld.sr.scaled_camera(data["intr"][frame], LEAK_HW, LEAK_HW)
    return (ld.analytic_depth(scenario, LEAK_CAMERA, frame), ld.lidar_depth(xyz, mats, cam, *LEAK_HW, occlusion=False),
            ld.lidar_depth(xyz, mats, cam, *LEAK_HW))


def leak_conditions(g, off, on, say=print):
    """The three conditions of the filter, figures first."""
    before, after = int(ld.leaked(off, g).sum()), int(ld.leaked(on, g).sum())
    covered, kept = int((off > 0).sum()), int(((off > 0) & (on > 0)).sum())
    say(f"leaked pixels {before} -> {after}; covered {covered}, kept {kept} ({100.0 * kept / covered:.2f} %)")
    assert not ((on > 0) & (off == 0)).any()                                             # the filter only removes
    assert before >= 1000, before
    assert 3 * after <= before, (before, after)
    assert kept >= 0.95 * covered, (kept, covered)


# ---- a constant map: 3 % of the pixels at 12.5 m
@functools.lru_cache(maxsize=None)
def constant_map(hw=(70, 100)):
    rng = np.random.default_rng(7)
    return np.where(rng.random((2,) + hw) < 0.03, F(12.5), F(0)).astype(F)


# ---- a map wider than two 256-column segments of the 31 x 31 row pass: few returns, some of them within 15 columns of a seam
WIDE_SHAPE, WIDE_SEAMS = (2, 70, 600), (256, 512)


@functools.lru_cache(maxsize=None)
def wide_map():
    rng = np.random.default_rng(600)
    d = np.where(rng.random(WIDE_SHAPE) < 0.004, rng.uniform(2.0, 90.0, WIDE_SHAPE), 0.0).astype(F)
    d[0, 30:, :] = 0                                                                      # frame 0: nothing below row 30
    for seam in WIDE_SEAMS:                                                               # near returns a little to either side of a seam
        for row, off, z in ((5, -12, 3.0), (20, 11, 4.0), (44, -3, 2.5), (60, 2, 5.0), (33, -15, 6.0), (12, 14, 3.5)):
            d[1 if row >= 30 else 0, row, seam + off] = z
    return d


# ---- sparse maps for the completion: every edge value of step 1 among them
@functools.lru_cache(maxsize=None)
def sparse_map(shape, density, special=True):
    rng = np.random.default_rng(shape[0] * 1000003 + shape[1] * 1009 + shape[2] + (7 if density == "single" else int(density * 1000)))
    d = rng.uniform(1.0, 90.0, shape).astype(F)
    if density == "single":
        mask = np.zeros(shape, bool)
        mask.reshape(shape[0], -1)[:, (shape[1] * shape[2]) // 2] = True
    else:
        mask = rng.random(shape) < density
    d = np.where(mask, d, F(0)).astype(F)
    if special and d.size >= 64:
        flat = d.reshape(-1)
        at = rng.choice(flat.size, size=12, replace=False)
        flat[at] = np.array([0.1, np.nextafter(F(0.1), F(1)), 100.0 - 0.1, np.nextafter(F(99.9), F(0)), np.nextafter(F(99.9), F(200)), 100.0,
                             140.0, np.nan, np.inf, -np.inf, -3.0, 99.0], dtype=F)
    return d
