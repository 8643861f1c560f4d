"""Cross-view depth consistency on the GPU (csrc/consistency.hip through mudg_amd/depth.py, mudg_amd/metrics.py and
virtual_render/virtual_pose_render.py) against the CPU definition of the rule (tests/consistency_reference.py): torch.equal everywhere —
both sides perform the same correctly rounded fp64 operations in the same order and the statistics are integers, so there is no
tolerance."""
import numpy as np
import pytest
import torch

import consistency_reference as cr
import depth_reference as dr
from helpers import cfgs

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
SIZES = [(24, 32), (23, 29)]                     # the four-pixel flags form; the one-pixel form with a row tail
NAMES = ("flags", "agree", "violate", "keep", "stats")
WIDE_MASK = cr.DYNAMIC_MASK | (1 << 63)          # class 63 is dynamic too


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _views(hw, seed):
    """The analytic scene's six views (3 frames x 2 poses) with 3 % depth noise — so that all three verdicts occur — and the pixel
    values and labels the rule has a branch for."""
    from mudg_amd import depth
    rng = np.random.default_rng(seed)
    z, c2w, times, poses = cr.scene_views(hw)
    z = (z.astype(D) * (1 + rng.normal(0, 0.03, z.shape))).astype(F)
    z[0, 5:8, 9:12] *= F(0.5)                                                  # a floater
    z[1, 2, :6] = F([0.0, np.nan, 100.0, np.nextafter(F(100.0), F(0)), -4.0, np.inf])
    z[4, hw[0] - 1, hw[1] - 3:] = F([np.nan, 100.0, np.nextafter(F(100.0), F(0))])      # in the row tail of the last row
    labels = rng.integers(0, 10, z.shape).astype(np.int64)                     # static classes
    labels[:, :2, 3:9] = 10                                                    # sky
    labels[2, 10:16, 4:20] = 13                                                # a car in frame 2, pose 0: views of other frames do not judge it
    labels[5, 9:17, 2:18] = 13                                                 # and in frame 2, pose 1: they see each other
    labels[3, 4, :4] = [63, 64, -1, 18]
    labels[3, 5, :3] = [np.iinfo(np.int64).min, np.iinfo(np.int64).max, 10 + (1 << 32)]      # the whole 64 bits are compared
    source = depth.camera_table(cr.SCENE_INTR, c2w, hw, hw)
    return {"depth": z, "labels": labels, "c2w": c2w, "times": times, "poses": poses, "source": source, "witness": depth.witness_table(c2w, source),
            "lists": depth.default_witnesses(times, poses, reach=2)}


@pytest.fixture(scope="module")
def cases():
    """The inputs of every size with the definition's outputs for every radius, with and without labels; computed once, left unchanged."""
    out = {}
    for n, hw in enumerate(SIZES):
        c = _views(hw, 70 + n)
        for r in (0, 1, 2):
            for labelled in (True, False):
                c[(r, labelled)] = cr.consistency(c["depth"], c["labels"] if labelled else None, c["source"], c["witness"], c["times"], c["lists"],
                                                  **dict(cr.DEFAULTS, r=r, dynamic_mask=WIDE_MASK))
        hits = np.zeros(4, dtype=bool)                                         # projections into row 0, row H-1, column 0, column W-1
        for s in range(6):
            P = cr.world_points(c["depth"][s], c["source"][s])
            for w in c["lists"][s]:
                ok, jw, iw, _ = cr.projections(P, (c[(1, False)]["flags"][s] & 1) == 1, c["witness"][w], hw)
                hits |= [(jw[ok] == 0).any(), (jw[ok] == hw[0] - 1).any(), (iw[ok] == 0).any(), (iw[ok] == hw[1] - 1).any()]
        c["border_hits"] = hits
        out[hw] = c
    return out


def _assert_equal(got, want, what):
    for name in NAMES:
        w, g = _t(want[name]), got[name].cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        differ = int((g != w).sum())
        print(f"{what}: {name}: {differ} of {w.numel()} values differ")
        assert torch.equal(g, w), (what, name, differ)


def _run(cuda, c, labels, **kw):
    from mudg_amd import depth
    return depth.consistent_views(_t(c["depth"]).to(cuda), cr.SCENE_INTR, c["c2w"], c["depth"].shape[1:], None if labels is None else _t(labels).to(cuda),
                                  times=c["times"], witnesses=c.get("lists"), **kw)


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("r", [0, 1, 2])
@pytest.mark.parametrize("labelled", [True, False])
def test_consistent_views_is_bit_equal_to_the_cpu_definition(cuda, cases, hw, r, labelled):
    c = cases[hw]
    want = c[(r, labelled)]
    labels = c["labels"] if labelled else None
    got = _run(cuda, c, labels, r=r, dynamic_mask=WIDE_MASK)
    assert set(got) == set(NAMES)
    _assert_equal(got, want, f"{hw} r={r} labels={labelled}")
    again = _run(cuda, c, labels, r=r, dynamic_mask=WIDE_MASK)                 # two runs: the same bits
    for name in NAMES:
        assert torch.equal(got[name], again[name]), name
    # the fixture exercises what it is meant to: all three verdicts, kept and dropped pixels, what is not usable stores zeros
    a, b, k, f = (want[name] for name in ("agree", "violate", "keep", "flags"))
    usable = (f & 1) == 1
    assert a.max() >= 3 and b.max() >= 1 and 0 < k.sum() < k.size and ((a == 0) & (b == 0) & usable).any()
    assert not (a | b | k)[~usable].any() and (f[1, 2, :6] & 1).tolist() == [0, 0, 0, 1, 0, 0]
    assert b[0, 5:8, 9:12].min() >= 1 and not k[0, 5:8, 9:12].any()           # the floater is seen through
    assert c["border_hits"].all()                                              # windows are clipped at all four borders
    if labelled:
        assert f[3, 4, :4].tolist() == [3, 1, 1, 3] and not f[:, :2, 3:9].any() and (f[3, 5, :3] & 1).all()
        car = c["labels"][2] == 13
        assert (f[2][car] & 2).all() and a[2][car].max() <= 1                  # only view 5 shows frame 2 as well
    else:
        assert f.max() == 1 and (f[:, :2, 3:9] == 1).all()


def test_the_default_mask_leaves_class_63_static(cuda, cases):
    c = cases[(24, 32)]
    want = cr.consistency(c["depth"], c["labels"], c["source"], c["witness"], c["times"], c["lists"])
    got = _run(cuda, c, c["labels"])
    _assert_equal(got, want, "default mask")
    assert want["flags"][3, 4, :4].tolist() == [1, 1, 1, 3]


def test_unaligned_bases_take_the_one_pixel_form_and_give_the_same_bits(cuda, cases):
    from mudg_amd import ops
    c = cases[(24, 32)]
    want = c[(1, True)]
    shift = lambda a, pad: torch.cat([torch.zeros(pad, dtype=_t(a).dtype), _t(a).reshape(-1)]).to(cuda)[pad:].view(a.shape)
    z, labels = shift(c["depth"], 1), shift(c["labels"], 1)
    assert z.data_ptr() % 16 and labels.data_ptr() % 16 and z.is_contiguous()
    flags = ops.view_flags(z, labels, dynamic_mask=WIDE_MASK)
    assert torch.equal(flags.cpu(), _t(want["flags"]))
    flags = shift(want["flags"], 3)
    assert flags.data_ptr() % 4
    tables = _t(np.stack([c["source"], c["witness"]])).to(cuda)
    agree, violate, keep, stats = ops.view_consistency(z, flags, tables[0], tables[1], c["times"], c["lists"])
    _assert_equal({"flags": flags, "agree": agree, "violate": violate, "keep": keep, "stats": stats}, want, "unaligned")
    again = ops.view_consistency(z, flags, tables[0], tables[1], c["times"], c["lists"])                    # two runs: the same bits
    assert all(torch.equal(a, b) for a, b in zip(again, (agree, violate, keep, stats)))
    assert torch.equal(ops.view_flags(z, labels, dynamic_mask=WIDE_MASK).cpu(), _t(want["flags"]))


@pytest.mark.parametrize("hw", SIZES)
def test_witness_lists_with_padding_the_view_itself_and_strange_cameras(cuda, cases, hw):
    """Ten views: the six of the scene, a copy of view 0 (same pose, same depth, same time), a camera that looks away from the scene, one
    whose first world-to-camera row is 1e300 times too large (u beyond any integer, v as it should be) and one whose second row is not
    a number (v not a number, u as it should be).  N = 5 with -1 in the middle and at the end, lists that hold the view itself."""
    from mudg_amd import depth, hip, ops
    c = cases[hw]
    z = np.concatenate([c["depth"], c["depth"][:1], c["depth"][:3]])
    back = c["c2w"][0] @ np.diag([-1.0, 1.0, -1.0, 1.0])                       # turned half round about the vertical
    c2w = np.concatenate([c["c2w"], c["c2w"][:1], back[None], c["c2w"][1:2], c["c2w"][1:2]])
    times = np.concatenate([c["times"], c["times"][:1], [0, 1, 1]]).astype(np.int32)
    source = depth.camera_table(cr.SCENE_INTR, c2w, hw, hw)
    witness = depth.witness_table(c2w, source)
    witness[8, 0:4] *= 1e300                                                   # qx, and with it u, beyond any integer
    witness[9, 4:8] = np.nan                                                   # v not a number
    usable3 = (cr.flags(z[3]) & 1) == 1
    P3 = cr.world_points(z[3], source[3])
    assert cr.projections(P3, usable3, witness[1], hw)[0].sum() > 100          # view 1's camera sees view 3's points: only the broken row
    assert not cr.projections(P3, usable3, witness[8], hw)[0].any() and not cr.projections(P3, usable3, witness[9], hw)[0].any()      # stops them
    lists = np.array([[0, 6, -1, -1, -1], [1, -1, 0, 7, -1], [7, 8, -1, 2, 9], [8, 9, 0, -1, 3], [-1, -1, -1, -1, -1], [5, 5, 5, 5, 5],
                      [0, 1, 2, 3, 4], [0, 1, 2, 3, 4], [0, 1, 2, 3, 4], [0, 1, 2, 3, 4]], dtype=np.int32)
    tables = _t(np.stack([source, witness])).to(cuda)
    for r in (0, 1, 2):
        rule = dict(cr.DEFAULTS, r=r, min_agree=1)
        want = cr.consistency(z, None, source, witness, times, lists, **rule)
        flags = ops.view_flags(_t(z).to(cuda))
        out = ops.view_consistency(_t(z).to(cuda), flags, tables[0], tables[1], times, lists, **rule)
        _assert_equal(dict(zip(NAMES, (flags,) + out)), want, f"{hw} lists r={r}")
        again = ops.view_consistency(_t(z).to(cuda), flags, tables[0], tables[1], times, lists, **rule)     # two runs: the same bits
        assert all(torch.equal(a, b) for a, b in zip(again, out))
        usable = want["flags"][0] & 1
        # view 0 against itself (skipped) and its copy: every usable pixel lands in its own pixel and agrees — known without arithmetic
        assert np.array_equal(want["agree"][0], usable) and not want["violate"][0].any() and np.array_equal(want["keep"][0], usable)
        assert want["agree"][1].max() == 1 and not want["agree"][2].any() and not want["agree"][4].any() and not want["agree"][5].any() and not want["violate"][4:6].any()
        assert want["stats"][4].tolist() == [int((want["flags"][4] & 1).sum()), 0, 0, 0, 0, 0]
        assert want["agree"][3].max() == 1                                     # the two broken cameras never count
        for wrong in (np.where(lists == 6, 10, lists), np.where(lists == 6, -2, lists)):
            with pytest.raises(hip.MudgError, match="witness ids"):
                ops.view_consistency(_t(z).to(cuda), flags, tables[0], tables[1], times, wrong, **rule)
    # views 1, 2 and 3 against v = NaN, the camera that looks away and u = 1e300 alone: nothing lands anywhere
    alone = np.array([[-1], [9], [7], [8]] + [[-1]] * 6, dtype=np.int32)
    got = ops.view_consistency(_t(z).to(cuda), flags, tables[0], tables[1], times, alone)
    want = cr.consistency(z, None, source, witness, times, alone)
    _assert_equal(dict(zip(NAMES, (flags,) + got)), want, f"{hw} alone")
    assert not want["agree"].any() and not want["violate"].any() and want["stats"][:, 1:].max() == 0


def test_a_dynamic_pixel_and_differing_time_ids(cuda, cases):
    """Every view its own time (the default): a dynamic pixel has no witness at all, and no view counts a dynamic pixel."""
    c = cases[(24, 32)]
    free = {k: v for k, v in c.items() if k != "lists"}
    free["times"] = None
    from mudg_amd import depth
    lists = depth.default_witnesses(np.arange(6), np.zeros(6, int), reach=2)
    want = cr.consistency(c["depth"], c["labels"], c["source"], c["witness"], np.arange(6), lists)
    got = _run(cuda, free, c["labels"])
    _assert_equal(got, want, "own times")
    again = _run(cuda, free, c["labels"])                                      # two runs: the same bits
    assert all(torch.equal(got[n], again[n]) for n in NAMES)
    car = c["labels"][2] == 13
    assert not want["agree"][2][car].any() and not want["violate"][2][car].any() and want["agree"][2][~car].any()


def test_given_times_and_default_witnesses_list_the_views_of_the_same_frame(cuda, cases):
    """times given, witnesses left to the default: views that share a frame witness each other, so a dynamic pixel keeps a witness."""
    from mudg_amd import depth, hip
    c = cases[(24, 32)]
    free = {k: v for k, v in c.items() if k != "lists"}
    for reach in (None, 1):
        lists = depth.default_witnesses(c["times"], None, 2 if reach is None else reach)
        assert lists[:, 0].tolist() == [3, 4, 5, 0, 1, 2] and int((lists[0] >= 0).sum()) == (5 if reach is None else 3)
        want = cr.consistency(c["depth"], c["labels"], c["source"], c["witness"], c["times"], lists)
        got = _run(cuda, free, c["labels"], **({} if reach is None else {"reach": reach}))
        _assert_equal(got, want, f"default lists, reach {reach}")
        car = c["labels"][2] == 13
        assert want["agree"][2][car].max() == 1                                # view 5, the other pose of frame 2
    with pytest.raises(hip.MudgError, match="one of the two"):
        _run(cuda, c, c["labels"], reach=2)                                    # reach beside given lists would be ignored: refused


def test_the_counters_at_the_full_frame_size(cuda):
    """A 576 x 1024 pair, every pixel usable: a wall 10 m ahead seen from two cameras 0.5 m apart.  The columns that the other camera
    also sees agree once; the statistics equal the definition's Python integers."""
    from mudg_amd import depth, metrics
    H, W = 576, 1024
    z = np.full((2, H, W), 10.0, dtype=F)
    c2w = np.stack([np.eye(4), np.eye(4)])
    c2w[1, 0, 3] = 0.5
    intr = np.array([[800.0, 0, 512.0], [0, 800.0, 288.0], [0, 0, 1]])
    source = depth.camera_table(intr, c2w, (H, W), (H, W))
    lists = np.array([[1], [0]], dtype=np.int32)
    want = cr.consistency(z, None, source, depth.witness_table(c2w, source), [0, 0], lists, **dict(cr.DEFAULTS, min_agree=1))
    assert want["stats"].tolist() == [[H * W, H * (W - 40), H * (W - 40), H * (W - 40), 0, 0]] * 2          # 800 * 0.5 / 10 = 40 columns leave
    got = depth.consistent_views(_t(z).to(cuda), intr, c2w, (H, W), times=[0, 0], witnesses=lists, min_agree=1)
    _assert_equal(got, want, "full size")
    again = depth.consistent_views(_t(z).to(cuda), intr, c2w, (H, W), times=[0, 0], witnesses=lists, min_agree=1)
    assert all(torch.equal(got[n], again[n]) for n in NAMES)
    scores = metrics.view_consistency(got)
    per_view, overall = cr.scores(want["stats"])
    assert scores["overall"] == overall and [{k: scores[k][v] for k in per_view[v]} for v in range(2)] == per_view
    assert scores["kept"] == [(W - 40) / W] * 2 and scores["mean_agree"] == [1.0, 1.0] and scores["violated"] == [0.0, 0.0]


def test_fuse_views_is_lift_views_of_the_definitions_keep(cuda, cases):
    from mudg_amd import cloud, depth, render
    c = cases[(23, 29)]
    want = c[(1, True)]
    rng = np.random.default_rng(4)
    rgb = rng.integers(0, 256, c["depth"].shape + (3,), dtype=np.uint8)
    lifted = [dr.unproject(c["depth"][v], rgb[v], c["source"][v], c["labels"][v]) for v in range(6)]
    packed, valid = np.concatenate([l[0] for l in lifted]), np.concatenate([l[1] for l in lifted])
    assert np.array_equal(valid, want["flags"].reshape(-1) & 1)                # the same validity rule
    chosen = (valid == 1) & (want["keep"].reshape(-1) != 0)
    assert 0 < chosen.sum() < valid.sum()
    dev = lambda a: _t(a).to(cuda)
    args = (dev(c["depth"]), dev(rgb), cr.SCENE_INTR, c["c2w"], (23, 29), dev(c["labels"]))
    rule = dict(times=c["times"], witnesses=c["lists"], dynamic_mask=WIDE_MASK)
    points, result = depth.fuse_views(*args, **rule)
    assert isinstance(points, render.PointCloud) and torch.equal(points.points.cpu(), _t(packed[chosen]))
    _assert_equal(result, want, "fuse_views")
    with_keep = depth.lift_views(*args, keep=dev(want["keep"]))
    assert torch.equal(with_keep.points, points.points)
    assert torch.equal(depth.lift_views(*args, keep=dev(want["keep"] * np.uint8(255))).points, points.points)      # any non-zero byte keeps
    thinned, _ = depth.fuse_views(*args, voxel_size=0.5, **rule)
    assert torch.equal(thinned.points, cloud.voxel_downsample(with_keep, 0.5).points) and 0 < len(thinned) < len(points)
    again, _ = depth.fuse_views(*args, **rule)
    assert torch.equal(again.points, points.points)


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("sky", [True, False])
def test_lift_views_without_keep_is_unchanged(cuda, hw, sky):
    """The inputs of tests/test_depth_gpu.py's lifting test: keep=None (and no keep argument) gives the definition's points, as before."""
    from mudg_amd import depth
    from test_depth_gpu import _camera, _streams
    u8, lidar, labels = _streams(hw, 40 + SIZES.index(hw))
    z = dr.metric_depth(u8, lidar)["depth"].copy()
    z[0, 0, :3] = F([0.0, 100.0, 2.0 ** -30])
    labels = labels if sky else None
    c2w, intr = (np.stack(v) for v in zip(*(_camera(k) for k in range(3))))
    table = depth.camera_table(intr, c2w, (960, 1280), hw)
    want = [dr.unproject(z[t], u8[t], table[t], None if labels is None else labels[t]) for t in range(3)]
    want_p, want_v = np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want])
    dev = lambda a: None if a is None else _t(a).to(cuda)
    plain = depth.lift_views(dev(z), dev(u8), intr, c2w, (960, 1280), dev(labels))
    explicit = depth.lift_views(dev(z), dev(u8), intr, c2w, (960, 1280), dev(labels), keep=None)
    assert torch.equal(plain.points.cpu(), _t(want_p[want_v == 1])) and torch.equal(explicit.points, plain.points)
    everything = depth.lift_views(dev(z), dev(u8), intr, c2w, (960, 1280), dev(labels), keep=torch.ones(z.shape, dtype=torch.uint8, device=cuda))
    nothing = depth.lift_views(dev(z), dev(u8), intr, c2w, (960, 1280), dev(labels), keep=torch.zeros(z.shape, dtype=torch.uint8, device=cuda))
    assert torch.equal(everything.points, plain.points) and len(nothing) == 0


def test_wrappers_check_their_arguments(cuda):
    from mudg_amd import depth, hip, ops
    z = torch.ones(2, 8, 8, device=cuda)
    flags = ops.view_flags(z)
    table = torch.zeros(2, 16, dtype=torch.float64, device=cuda)
    with pytest.raises(hip.MudgError, match="labels"):
        ops.view_flags(z, torch.zeros(2, 8, 8, dtype=torch.int32, device=cuda))
    with pytest.raises(hip.MudgError, match="dynamic_mask"):
        ops.view_flags(z, dynamic_mask=1 << 64)
    with pytest.raises(hip.MudgError, match="wit_table"):
        ops.view_consistency(z, flags, table, table[:, :12].contiguous(), [0, 1], [[1], [0]])
    with pytest.raises(hip.MudgError, match="r 3"):
        ops.view_consistency(z, flags, table, table, [0, 1], [[1], [0]], r=3)
    with pytest.raises(hip.MudgError, match="abs_tol"):
        ops.view_consistency(z, flags, table, table, [0, 1], [[1], [0]], abs_tol=-0.1)
    with pytest.raises(hip.MudgError, match="cameras"):
        depth.consistent_views(z, np.eye(3), np.stack([np.eye(4)] * 3), (8, 8))
    with pytest.raises(hip.MudgError, match="keep"):
        depth.lift_views(z, torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=cuda), np.eye(3), np.stack([np.eye(4)] * 2), (8, 8),
                         keep=torch.ones(2, 8, 4, dtype=torch.uint8, device=cuda))


def test_a_window_generated_at_two_poses_becomes_one_filtered_cloud_that_renders_again(cuda):
    """render_windows -> synthesize_windows -> window_outputs at poses 1 and 2 -> fuse_window_outputs -> render_conditions on the fused
    cloud, on the tiny driver model (4 frames of 64 x 64, 2 DDIM steps).  The model is random: shapes, dtypes, that the kept points are a
    subset of the lifted ones, and the same bits from two runs — nothing about how many points survive."""
    from mudg_amd import depth, render
    from mudg_amd.synthetic import street_scene
    from test_splat_gpu import _driver_model, _upload
    from virtual_render.virtual_pose_render import fuse_window_outputs, render_windows, synthesize_windows, window_outputs
    small = street_scene(n_background=150_000, frames=4, seed=5, n_objects=3, object_points=3000)
    model, g = _driver_model(cuda)
    shp, px = g["shape"], g["driver"]["pixels"]
    L = shp["T"]
    bg, objects = _upload(small, cuda)
    scene = render.Scene(bg, objects, small["intr"], small["c2w"], small["hw_native"])
    dense = (torch.rand(3, 3, L, px, px, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(cuda)
    sm = cfgs.SAMPLER
    outputs, cams = [], []
    for pose in (1, 2):
        wins = list(render_windows(scene, dense, pose=pose, video_length=L))
        samples = synthesize_windows(model, wins, [3, 4, L, shp["H"], shp["W"]], video_length=L, ddim_steps=2, ddim_eta=1.0,
                                     unconditional_guidance_scale=sm["cfg_scale"], fs=sm["fs"], timestep_spacing=sm["spacing"],
                                     guidance_rescale=sm["guidance_rescale"])[0]
        cams.append(np.stack([render.virtual_poses(c, with_ori_pose=True)[pose] for c in small["c2w"]]))
        cond = render.render_conditions(bg, objects, small["intr"], small["c2w"], small["hw_native"], (px, px), poses=cams[-1][:, None], return_images=True)
        outputs.append(window_outputs(samples, cond))
    cloud, scores = fuse_window_outputs(outputs, scene, range(L), (1, 2))
    result = scores["result"]
    V = 2 * L
    for name in ("agree", "violate", "keep", "flags"):
        assert result[name].dtype == torch.uint8 and tuple(result[name].shape) == (V, px, px) and result[name].is_cuda, name
    assert result["stats"].dtype == torch.int64 and tuple(result["stats"].shape) == (V, 6)
    assert isinstance(cloud, render.PointCloud) and cloud.points.dtype == torch.int32 and len(cloud) == int(result["keep"].sum()) == int(result["stats"][:, 2].sum())
    for key in ("tested", "kept", "violated", "mean_agree"):
        assert len(scores[key]) == V and all(isinstance(v, float) for v in scores[key]) and isinstance(scores["overall"][key], float), key
    stack = lambda name: torch.cat([o[name] for o in outputs])
    intr = np.broadcast_to(np.asarray(small["intr"], dtype=D), (L, 3, 3))
    lifted = depth.lift_views(stack("depth"), stack("color"), np.concatenate([intr, intr]), np.concatenate(cams), small["hw_native"], stack("semantic_labels"))
    assert len(cloud) <= len(lifted) == int((result["flags"] & 1).sum())
    chosen = result["keep"].reshape(-1)[(result["flags"].reshape(-1) & 1).bool()].bool()
    assert torch.equal(lifted.points[chosen], cloud.points)                    # the kept points, in the lifted cloud's order
    again, scores2 = fuse_window_outputs(outputs, scene, range(L), (1, 2))
    assert torch.equal(again.points, cloud.points) and all(torch.equal(scores2["result"][n], result[n]) for n in NAMES)
    assert repr({k: v for k, v in scores2.items() if k != "result"}) == repr({k: v for k, v in scores.items() if k != "result"})
    if len(cloud):
        merged = render.PointCloud.concatenated(bg, cloud)
        seen = render.render_conditions(merged, None, small["intr"], small["c2w"], small["hw_native"], (px, px), poses=cams[0][:, None], return_images=True)
        assert seen["sparse_frames"].shape == (1, 3, L, px, px) and seen["sparse_frames"].dtype == torch.float32
        assert torch.isfinite(seen["sparse_frames"]).all() and torch.isfinite(seen["sparse_depth"]).all()
