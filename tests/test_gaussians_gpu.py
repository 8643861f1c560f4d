"""The Gaussian splat renderer on the GPU (csrc/gaussians.hip through mudg_amd/gaussians.py) against the CPU definition of the rule
(tests/gaussians_reference.py): torch.equal everywhere, for the images and for the intermediate counts, rectangles, sorted values and
ranges — both sides perform the same correctly rounded fp32 operations in the same order, so there is no tolerance."""
import numpy as np
import pytest
import torch

import gaussians_reference as gr
from sentinel_buffers import Flat

pytestmark = pytest.mark.gpu
F = np.float32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _gaussians(cuda, pts, cov, op, ids=None):
    from mudg_amd import gaussians, render
    return gaussians.Gaussians(render.PointCloud(_t(pts).to(cuda)), _t(cov).to(cuda), _t(op).to(cuda), None if ids is None else _t(ids).to(cuda))


def _render(cuda, case, **kw):
    """The product's render of a case (pts, cov, op, ids, mats, cam, hw), twice: the second call must give the same bits."""
    from mudg_amd import gaussians
    pts, cov, op, ids, mats, cam, hw = case
    g = _gaussians(cuda, pts, cov, op, ids)
    tx, ty = gr.tiles(hw)
    runs = []
    for _ in range(2):
        stats = {"walked": torch.full((mats.shape[0] * tx * ty,), -1, dtype=torch.int32, device=cuda)}
        out = gaussians.render(g, _t(mats).to(cuda), cam, hw, stats=stats, **kw)
        runs.append((out, stats))
    (out, stats), (again, stats2) = runs
    for k in ("rgb", "depth", "alpha"):
        assert torch.equal(out[k].view(torch.int32), again[k].view(torch.int32)), f"{k}: a repeat run differs"
    for k in ("count", "rect", "values", "ranges", "walked"):
        assert (stats[k] is None and stats2[k] is None) or torch.equal(stats[k], stats2[k]), f"{k}: a repeat run differs"
    return out, stats


def _assert_equal(out, stats, want, what):
    V = want["count"].shape[0]
    H, W = want["alpha"].shape[1:]
    assert out["rgb"].shape == (V, 3, H, W) and out["depth"].shape == out["alpha"].shape == (V, H, W)
    assert all(out[k].dtype == torch.float32 for k in out)
    bad = {k: int((out[k].cpu() != _t(want[w])).sum()) for k, w in (("rgb", "rgb"), ("depth", "depth_image"), ("alpha", "alpha"))}
    print(f"{what}: {want['entries']} entries, longest tile {want['longest_tile']}, {int((want['count'] > 0).sum())} of {want['count'].size} drawn, "
          f"coverage {float((want['alpha'] > 0.5).mean()):.3f}; elements that differ: {bad}")
    assert torch.equal(stats["count"].cpu(), _t(want["count"])), what
    assert torch.equal(stats["rect"].cpu(), _t(want["rect"])), what
    assert stats["entries"] == want["entries"] and stats["longest_tile"] == want["longest_tile"], what
    if want["entries"]:
        assert torch.equal(stats["values"].cpu(), _t(want["values"])), what
        assert torch.equal(stats["ranges"].cpu(), _t(want["ranges"])), what
        if stats.get("walked") is not None:
            walked = np.minimum(want["ranges"][:, 1] - want["ranges"][:, 0], 256 * ((want["looked"] + 255) // 256))      # whole batches until every pixel is done
            assert stats["walked"].cpu().tolist() == walked.tolist(), what
    else:
        assert stats["values"] is None and stats["ranges"] is None
    for k, w in (("rgb", "rgb"), ("depth", "depth_image"), ("alpha", "alpha")):
        assert torch.equal(out[k].cpu(), _t(want[w])), (what, k)


def _check(cuda, case, what, **kw):
    want = gr.render(*case, **kw)
    out, stats = _render(cuda, case, **kw)
    _assert_equal(out, stats, want, what)
    return out, stats, want


def _scene_case(n, hw, seed, views=1):
    xyz, rgb, cov, op, mats, cam = gr.seeded_scene(n, hw, seed)
    if views > 1:
        rng = np.random.default_rng(seed + 100)
        more = [mats[0]]
        for _ in range(views - 1):
            a, b = rng.uniform(-0.2, 0.2, 2)
            more.append(np.array([[np.cos(a), 0, np.sin(a), b, 0, 1, 0, 0.1, -np.sin(a), 0, np.cos(a), 1.0 + b]], dtype=F))
        mats = np.stack(more)
    return gr.pack(xyz, rgb), cov, op, None, mats, cam, hw


def _flat_case(centres, scale, hw, **kw):
    pts, cov, op = gr.flat_case(centres, scale, **kw)
    return pts, cov, op, None, gr.FLAT[None], gr.FLAT_CAM, hw


# ------------------------------------------------------------------------------------------------ image sizes, batch edges
@pytest.mark.parametrize("hw", [(1, 1), (16, 16), (17, 33), (40, 56)])
def test_images_that_are_and_are_not_whole_tiles(cuda, hw):
    out, stats, want = _check(cuda, _scene_case(150, hw, 11), f"{hw[0]} x {hw[1]}")
    assert want["entries"] > 0 and (want["alpha"] > 0).any()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_a_tile_with_entries_at_the_batch_edges(cuda, n):
    rng = np.random.default_rng(n)
    case = _flat_case(rng.uniform(5.0, 11.0, (n, 2)), 0.5, (17, 33), opacity=rng.uniform(0.004, 0.02, n).astype(F), z=rng.uniform(60.0, 180.0, n).astype(F), seed=n)
    out, stats, want = _check(cuda, case, f"{n} Gaussians on one tile")
    assert want["ranges"].tolist()[0] == [0, n] and want["entries"] == n and want["looked"][0] == n                  # no pixel finishes: every entry is blended
    assert not want["ranges"][1:].any()


def test_a_tile_that_finishes_in_its_first_batch_leaves_the_rest_alone(cuda):
    rng = np.random.default_rng(21)
    n = 556
    case = _flat_case(rng.uniform(2.0, 14.0, (n, 2)), 40.0, (16, 16), z=rng.uniform(60.0, 180.0, n).astype(F), seed=21)
    out, stats, want = _check(cuda, case, "opaque after three entries, 556 on the tile")
    assert want["looked"][0] < 10 and stats["walked"].tolist() == [256] and want["entries"] - 256 == 300
    assert float(out["alpha"].min()) > 0.98                                                                    # a finished pixel: T < 1e-4 / (1 - 0.99)


def test_a_tile_where_a_pixel_never_finishes_is_walked_to_its_end(cuda):
    rng = np.random.default_rng(22)
    n = 300
    case = _flat_case(np.full((n, 2), 5.5, F), 3.0, (16, 16), z=rng.uniform(120.0, 180.0, n).astype(F), seed=22)
    out, stats, want = _check(cuda, case, "300 entries, the far corner untouched")
    assert want["alpha"][0, 15, 15] == 0 and want["alpha"][0, 5, 5] > 0.98 and stats["walked"].tolist() == [300]


def test_one_gaussian_over_every_tile_and_known_answers(cuda):
    out, stats, want = _check(cuda, _flat_case([[28.0, 20.0]], 60.0, (40, 56)), "one Gaussian over twelve tiles")
    assert want["count"][0, 0] == 12 and want["ranges"].tolist() == [[k, k + 1] for k in range(12)] and float(out["alpha"].min()) > 0.5
    out, _, _ = _check(cuda, _flat_case([[8.5, 8.5], [8.5, 8.5]], 0.5, (16, 16), z=[128.0, 160.0]), "two opaque Gaussians on a pixel centre")
    assert float(out["alpha"][0, 8, 8]) == float(gr.MAX_ALPHA)


def test_equal_depths_resolve_to_the_lower_index(cuda):
    rng = np.random.default_rng(23)
    case = _flat_case(rng.uniform(0.0, 33.0, (60, 2)), 2.0, (17, 33), opacity=0.5, seed=23)
    out, stats, want = _check(cuda, case, "sixty Gaussians at one depth")
    assert len(set(want["depth"][0][want["count"][0] > 0].tolist())) == 1
    for lo, hi in want["ranges"].tolist():
        assert want["values"][lo:hi].tolist() == sorted(want["values"][lo:hi].tolist())


def test_everything_culled_gives_zeros_and_launches_nothing_more(cuda):
    case = _flat_case([[8.5, 8.5], [3.0, 4.0]], 0.5, (17, 33), z=[250.0, 300.0])
    out, stats, want = _check(cuda, case, "beyond zfar")
    assert stats["entries"] == 0 and not out["rgb"].any() and not out["depth"].any() and not out["alpha"].any()
    assert stats["walked"].tolist() == [-1] * 6                                                                # the blend never ran


def test_three_views_in_one_call_equal_three_calls(cuda):
    case = _scene_case(200, (40, 56), 13, views=3)
    out, stats, want = _check(cuda, case, "three views")
    pts, cov, op, ids, mats, cam, hw = case
    for v in range(3):
        one, one_stats = _render(cuda, (pts, cov, op, ids, mats[v:v + 1], cam, hw))
        for k in ("rgb", "depth", "alpha"):
            assert torch.equal(one[k][0], out[k][v]), (v, k)
        assert torch.equal(one_stats["count"][0], stats["count"][v]) and torch.equal(one_stats["rect"][0], stats["rect"][v])
    assert not torch.equal(out["rgb"][0], out["rgb"][1])


def _ids_case():
    pts, cov, op, _, mats, cam, hw = _scene_case(200, (40, 56), 17, views=2)
    rng = np.random.default_rng(17)
    ids = rng.choice(np.array([-3, 0, 1, 2, 7], dtype=np.int32), 200)                                        # -3 -> 0, 7 -> 2
    shifted = mats.copy()
    shifted[:, 0, 3] += F(0.5)
    table = np.stack([mats[:, 0], shifted[:, 0], mats[::-1, 0]], axis=1)                                       # (2, 3, 12)
    table[0, 1] = 0                                                                                            # view 0 does not show object 0
    return pts, cov, op, ids, np.ascontiguousarray(table), cam, hw


def test_object_ids_a_zero_matrix_and_ids_out_of_range(cuda):
    case = _ids_case()
    out, stats, want = _check(cuda, case, "three matrices a view")
    ids = case[3]
    assert not want["count"][0][ids == 1].any() and want["count"][1][ids == 1].any()
    clamped = case[:3] + (np.clip(ids, 0, 2),) + case[4:]
    again, _ = _render(cuda, clamped)
    assert all(torch.equal(again[k], out[k]) for k in out)


def test_more_entries_than_allowed_are_refused(cuda):
    from mudg_amd import hip
    case = _scene_case(150, (40, 56), 11)
    want = gr.render(*case)
    with pytest.raises(hip.MudgError, match=f"{want['entries']} .* max_entries = {want['entries'] - 1}"):
        _render(cuda, case, max_entries=want["entries"] - 1)
    out, stats = _render(cuda, case, max_entries=want["entries"])
    _assert_equal(out, stats, want, "exactly max_entries")


# ------------------------------------------------------------------------------------------------ the entry points, outputs inside sentinels
def test_no_entry_point_writes_outside_its_outputs(cuda):
    from mudg_amd import hip
    pts, cov, op, ids, mats, cam, hw = _ids_case()
    want = gr.render(pts, cov, op, ids, mats, cam, hw)
    lib = hip.lib()
    V, n, (H, W) = mats.shape[0], len(pts), hw
    tx, ty = gr.tiles(hw)
    tiles, E = V * tx * ty, want["entries"]
    d_pts, d_cov, d_op, d_ids, d_mats = (_t(a).to(cuda) for a in (pts, cov, op, ids, mats))
    uv, conic, depth = Flat(V * n * 2, torch.float32).blank(cuda), Flat(V * n * 4, torch.float32).blank(cuda), Flat(V * n, torch.float32).blank(cuda)
    rect, count = Flat(V * n * 4, torch.int32).blank(cuda), Flat(V * n, torch.int32).blank(cuda)
    hip.check(lib.mudg_gauss_project(d_pts.data_ptr(), d_cov.data_ptr(), d_op.data_ptr(), d_ids.data_ptr(), n, d_mats.data_ptr(), V, mats.shape[1], H, W,
                                     *[float(c) for c in cam], gr.ZNEAR, gr.ZFAR, uv.ptr, conic.ptr, depth.ptr, rect.ptr, count.ptr, None), "project")
    torch.cuda.synchronize()
    got = {k: b.read(k) for k, b in (("uv", uv), ("conic", conic), ("depth", depth), ("rect", rect), ("count", count))}
    for k in got:
        assert torch.equal(got[k], _t(want[k]).reshape(-1)), k
    offsets = (torch.cumsum(got["count"].to(torch.int64), 0) - got["count"]).to(cuda)
    keys, values = Flat(E, torch.int64).blank(cuda), Flat(E, torch.int32).blank(cuda)
    dev = {k: v.to(cuda) for k, v in got.items()}
    hip.check(lib.mudg_gauss_keys(dev["depth"].data_ptr(), dev["rect"].data_ptr(), dev["count"].data_ptr(), offsets.data_ptr(), n, V, H, W, E, keys.ptr,
                                  values.ptr, None), "keys")
    torch.cuda.synchronize()
    k_sorted, order = torch.sort(keys.read("keys"), stable=True)
    v_sorted = values.read("values")[order]
    assert torch.equal(k_sorted, _t(want["keys"])) and torch.equal(v_sorted, _t(want["values"]))
    k_sorted, v_sorted = k_sorted.to(cuda), v_sorted.to(cuda)
    ranges = Flat(tiles * 2, torch.int32).blank(cuda)
    hip.check(lib.mudg_gauss_ranges(k_sorted.data_ptr(), E, tiles, ranges.ptr, None), "ranges")
    torch.cuda.synchronize()
    r = ranges.read("ranges")
    assert torch.equal(r, _t(want["ranges"]).reshape(-1))
    r = r.to(cuda)
    rgb, dimg, alpha = Flat(V * 3 * H * W, torch.float32).blank(cuda), Flat(V * H * W, torch.float32).blank(cuda), Flat(V * H * W, torch.float32).blank(cuda)
    walked = Flat(tiles, torch.int32).blank(cuda)
    hip.check(lib.mudg_gauss_blend(d_pts.data_ptr(), dev["uv"].data_ptr(), dev["conic"].data_ptr(), dev["depth"].data_ptr(), v_sorted.data_ptr(),
                                   r.data_ptr(), n, E, V, H, W, rgb.ptr, dimg.ptr, alpha.ptr, walked.ptr, None), "blend")
    torch.cuda.synchronize()
    assert torch.equal(rgb.read("rgb"), _t(want["rgb"]).reshape(-1))
    assert torch.equal(dimg.read("depth"), _t(want["depth_image"]).reshape(-1)) and torch.equal(alpha.read("alpha"), _t(want["alpha"]).reshape(-1))
    assert int(walked.read("walked").min()) >= 0


# ------------------------------------------------------------------------------------------------ scenes
@pytest.fixture(scope="module")
def street(cuda):
    from mudg_amd import render, synthetic
    s = synthetic.street_scene(n_background=2500, frames=2, seed=3, n_objects=2, object_points=200)
    background = render.PointCloud.from_arrays(s["bg_xyz"], s["bg_rgb"], cuda)
    objects = render.ObjectSet(s["objects"], s["transform_obj"], s["visibility"], cuda)
    return s, background, objects


def test_render_scene_on_the_synthetic_street(cuda, street):
    from mudg_amd import gaussians, render
    s, background, objects = street
    hw = (64, 96)
    g = gaussians.Gaussians.from_scene(background, objects, 0.1, object_scale=0.05)
    assert len(g) == 2900 and g.ids.cpu().tolist() == [0] * 2500 + [1] * 200 + [2] * 200
    scales = np.concatenate([np.full(2500, 0.1), np.full(400, 0.05)])
    assert torch.equal(g.cov.cpu(), _t(gr.isotropic(scales, 2900))) and torch.equal(g.opacity.cpu(), torch.ones(2900))
    stats = []
    out = gaussians.render_scene(g, objects, s["intr"], s["c2w"], s["hw_native"], hw, stats=stats)
    assert out["rgb"].shape == (3, 2, 3, 64, 96) and out["depth"].shape == out["alpha"].shape == (3, 2, 64, 96)
    assert out["rgb_u8"].shape == (3, 2, 64, 96, 3) and out["rgb_u8"].dtype == torch.uint8 and len(stats) == 2
    pts, cov, op, ids = g.cloud.points.cpu().numpy(), g.cov.cpu().numpy(), g.opacity.cpu().numpy(), g.ids.cpu().numpy()
    assert s["visibility"][1, 1] == 0                                                                          # frame 1 does not show object 1
    for t in range(2):
        poses = np.stack(render.virtual_poses(s["c2w"][t], 2.0, with_ori_pose=True))
        mats = gaussians.scene_matrices(objects, np.linalg.inv(poses), t)
        assert mats.shape == (3, 3, 12) and mats.dtype == F and (not mats[:, 2].any()) == (t == 1)
        cam = render.scaled_intrinsics(s["intr"], s["hw_native"], hw).astype(F)
        want = gr.render(pts, cov, op, ids, mats, cam, hw)
        frame = {k: out[k][:, t] for k in ("rgb", "depth", "alpha")}
        _assert_equal(frame, stats[t], want, f"street frame {t}")
        assert torch.equal(out["rgb_u8"][:, t].cpu(), _t(gr.rgb_u8(want["rgb"])))
        assert (want["count"][:, ids > 0] > 0).any() and (want["alpha"] > 0.5).mean() > 0.2


def test_render_cloud_views_feeds_psnr_ssim(cuda, street):
    from mudg_amd import gaussians, metrics, render
    from virtual_render import virtual_pose_render as vpr
    s, background, objects = street
    scene = render.Scene(background, objects, s["intr"], s["c2w"], s["hw_native"])
    frames, alpha = vpr.render_cloud_views(background, scene, [0, 1], 0, (64, 96), 0.1)
    assert frames.shape == (2, 64, 96, 3) and frames.dtype == torch.uint8 and alpha.shape == (2, 64, 96) and alpha.dtype == torch.float32
    g = gaussians.Gaussians.from_cloud(background, 0.1)
    direct = gaussians.render_scene(g, None, s["intr"], s["c2w"], s["hw_native"], (64, 96), poses=s["c2w"][:, None])
    assert torch.equal(frames, direct["rgb_u8"][0]) and torch.equal(alpha, direct["alpha"][0])
    moved, _ = vpr.render_cloud_views(background, scene, [0, 1], 2, (64, 96), 0.1, opacity=0.8)
    scores = metrics.psnr_ssim(frames, moved)
    assert scores["psnr"].shape == (2,) and bool(torch.isfinite(scores["psnr"]).all()) and bool((scores["ssim"] < 1).all())
    assert bool(torch.isinf(metrics.psnr_ssim(frames, frames)["psnr"]).all())
