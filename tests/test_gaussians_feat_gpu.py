"""Semantic Gaussians on the GPU (csrc/gaussians_feat.hip through mudg_amd/ops.py and gaussians.py) against the CPU definition of the rule
(tests/gaussians_feat_reference.py): torch.equal for the images, both states, both partial buffers, the gathered gradient and the three
outputs of the class loss — both sides perform the same correctly rounded fp32 operations in the same order, so there is no tolerance."""
import numpy as np
import pytest
import torch

import gaussians_bwd_reference as gb
import gaussians_feat_reference as gf
import gaussians_reference as gr
from sentinel_buffers import Flat
from test_gaussians_gpu import _flat_case, _ids_case, _scene_case

pytestmark = pytest.mark.gpu
F = np.float32
IMAGES = ("rgb", "depth_image", "alpha", "state")
OUTPUTS = IMAGES + ("feat_out", "partial", "partial_feat", "d_feat_g")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _inputs(case, Fn, seed=5, per_view=False):
    """fp32 colours that are no whole bytes, feature rows of both signs, and seeded upstream gradients for the four outputs."""
    pts, cov, op, ids, mats, cam, hw = case
    xyz, _ = gr.unpack(pts)
    rng = np.random.default_rng(seed)
    V = mats.shape[0]
    colour = rng.uniform(0.0, 255.0, ((V,) if per_view else ()) + (len(xyz), 3)).astype(F)
    feat = rng.normal(size=(len(xyz), Fn)).astype(F) * F(3.0)
    up = (rng.normal(size=(V, 3) + tuple(hw)).astype(F), (rng.normal(size=(V,) + tuple(hw)) * 0.05).astype(F),
          rng.normal(size=(V,) + tuple(hw)).astype(F), rng.normal(size=(V, Fn) + tuple(hw)).astype(F))
    return xyz, colour, feat, up


def _direct(cuda, case, colour, feat, up, corrupt=None):
    """The entry points one after the other through mudg_amd.ops, each twice: a repeat must give the same bits.  Also the existing
    training blend on the same inputs: its four outputs are the feature blend's."""
    from mudg_amd import ops
    pts, cov, op, ids, mats, cam, hw = case
    d = lambda a: None if a is None else _t(a).to(cuda)
    d_pts, d_cov, d_op, d_ids, d_mats, d_col, d_feat = d(pts), d(cov), d(op), d(ids), d(mats), d(colour), d(feat)
    d_up = [d(u) for u in up]
    uv, conic, depth, rect, count = ops.gauss_project(d_pts, d_cov, d_op, d_mats, cam, hw, ids=d_ids)
    ends = torch.cumsum(count.reshape(-1), 0, dtype=torch.int64)
    offsets = (ends - count.reshape(-1)).reshape(count.shape)
    E = int(ends[-1])
    assert E > 0
    keys, values = ops.gauss_keys(depth, rect, count, offsets, E, hw)
    keys, order = torch.sort(keys, stable=True)
    values = values[order]
    tx, ty = gr.tiles(hw)
    ranges = ops.gauss_ranges(keys, mats.shape[0] * tx * ty)
    if corrupt is not None:
        values, order, ranges, offsets = corrupt(values, order, ranges, offsets)
    runs = []
    for _ in range(2):
        rgb, dimg, alpha, feat_out, state = ops.gauss_blend_feat(d_col, d_feat, uv, conic, depth, values, ranges, hw)
        partial, partial_feat = ops.gauss_blend_bwd_feat(d_col, d_feat, uv, conic, depth, values, order, ranges, hw, state, feat_out, *d_up)
        d_feat_g = ops.gauss_feat_bwd(count, offsets, partial_feat)
        runs.append(dict(rgb=rgb, depth_image=dimg, alpha=alpha, state=state, feat_out=feat_out, partial=partial, partial_feat=partial_feat,
                         d_feat_g=d_feat_g))
    for k in runs[0]:
        assert torch.equal(runs[0][k].view(torch.int32), runs[1][k].view(torch.int32)), f"{k}: a repeat run differs"
    train = ops.gauss_blend_train_views if colour.ndim == 3 else ops.gauss_blend_train
    for k, t in zip(IMAGES, train(d_col, uv, conic, depth, values, ranges, hw)):
        assert torch.equal(runs[0][k].view(torch.int32), t.view(torch.int32)), f"{k}: not the existing training blend's bits"
    no_state = ops.gauss_blend_feat(d_col, d_feat, uv, conic, depth, values, ranges, hw, with_state=False)
    assert no_state[4] is None and all(torch.equal(a, runs[0][k]) for a, k in zip(no_state[:4], ("rgb", "depth_image", "alpha", "feat_out")))
    return runs[0], dict(values=values, order=order, ranges=ranges, offsets=offsets, count=count, uv=uv, conic=conic, depth=depth)


def _check(cuda, case, Fn, what, per_view=False):
    xyz, colour, feat, up = _inputs(case, Fn, per_view=per_view)
    pts, cov, op, ids, mats, cam, hw = case
    want = gf.render_backward(xyz, colour, feat, cov, op, ids, mats, cam, hw, *up)
    got, mid = _direct(cuda, case, colour, feat, up)
    assert torch.equal(mid["order"].cpu(), _t(want["order"])) and torch.equal(mid["values"].cpu(), _t(want["values"])), what
    bad = {k: int((got[k].cpu() != _t(want[k])).sum()) for k in OUTPUTS}
    print(f"{what}: {want['entries']} entries, F = {Fn}; elements that differ: {bad}")
    for k in OUTPUTS:
        assert got[k].dtype == torch.float32 and torch.equal(got[k].cpu(), _t(want[k])), (what, k)
    assert all(np.isfinite(want[k]).all() for k in OUTPUTS)
    return got, want, mid


# ------------------------------------------------------------------------------------------------ widths, image sizes, batch edges
@pytest.mark.parametrize("Fn", [1, 3, 19, 32])
def test_every_template_bound_and_a_width_inside_one(cuda, Fn):
    got, want, _ = _check(cuda, _scene_case(150, (17, 33), 11), Fn, f"F = {Fn}")
    assert want["feat_out"].any() and want["partial_feat"].any() and want["d_feat_g"].any()


@pytest.mark.parametrize("hw", [(1, 1), (16, 16), (17, 33), (40, 56)])
def test_images_that_are_and_are_not_whole_tiles(cuda, hw):
    got, want, _ = _check(cuda, _scene_case(150, hw, 11), 19, f"{hw[0]} x {hw[1]}")
    assert want["d_feat_g"].any()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_a_tile_with_entries_at_the_batch_edges(cuda, n):
    rng = np.random.default_rng(n)
    case = _flat_case(rng.uniform(5.0, 11.0, (n, 2)), 0.5, (17, 33), opacity=rng.uniform(0.004, 0.02, n).astype(F), z=rng.uniform(60.0, 180.0, n).astype(F), seed=n)
    got, want, _ = _check(cuda, case, 19, f"{n} Gaussians on one tile")
    assert want["entries"] == n and want["partial_feat"].any(axis=1).sum() >= 0.8 * n


def test_a_tile_that_finishes_in_its_first_batch_leaves_the_rest_at_zero(cuda):
    rng = np.random.default_rng(21)
    n = 556
    case = _flat_case(rng.uniform(2.0, 14.0, (n, 2)), 40.0, (16, 16), z=rng.uniform(60.0, 180.0, n).astype(F), seed=21)
    got, want, _ = _check(cuda, case, 19, "opaque after a few entries, 556 on the tile")
    behind = _t(want["order"][256:]).to(cuda)
    assert want["entries"] - 256 == 300 and not got["partial"][behind].any() and not got["partial_feat"][behind].any()
    assert 0 < int(got["partial_feat"].any(dim=1).sum()) < 10


def test_a_tile_where_a_pixel_never_finishes_is_walked_to_its_end(cuda):
    rng = np.random.default_rng(22)
    n = 300
    case = _flat_case(np.full((n, 2), 5.5, F), 3.0, (16, 16), z=rng.uniform(120.0, 180.0, n).astype(F), seed=22)
    got, want, _ = _check(cuda, case, 19, "300 entries, the far corner untouched")
    assert want["alpha"][0, 15, 15] == 0 and not want["feat_out"][0, :, 15, 15].any()


def test_three_views_in_one_call_equal_three_calls(cuda):
    case = _scene_case(200, (40, 56), 13, views=3)
    got, want, _ = _check(cuda, case, 19, "three views")
    xyz, colour, feat, up = _inputs(case, 19)
    pts, cov, op, ids, mats, cam, hw = case
    total = None
    for v in range(3):
        one, _ = _direct(cuda, (pts, cov, op, ids, mats[v:v + 1], cam, hw), colour, feat, [u[v:v + 1] for u in up])
        assert torch.equal(one["state"][0], got["state"][v]) and torch.equal(one["feat_out"][0], got["feat_out"][v])
        total = one["d_feat_g"] if total is None else total + one["d_feat_g"]
    assert torch.equal(total, got["d_feat_g"])                                                         # the views are added in view order


def test_one_colour_per_view_and_gaussian(cuda):
    got, want, _ = _check(cuda, _scene_case(200, (40, 56), 13, views=3), 19, "colours (V, n, 3)", per_view=True)
    assert want["rgb"].any()


def test_object_ids(cuda):
    _check(cuda, _ids_case(), 3, "three matrices a view")


def test_no_upstream_for_the_features_leaves_the_existing_partials(cuda):
    from mudg_amd import ops
    case = _scene_case(200, (40, 56), 13, views=2)
    xyz, colour, feat, up = _inputs(case, 19)
    up = up[:3] + (np.zeros_like(up[3]),)
    got, mid = _direct(cuda, case, colour, feat, up)
    d = lambda a: _t(a).to(cuda)
    partial = ops.gauss_blend_bwd(d(colour), mid["uv"], mid["conic"], mid["depth"], mid["values"], mid["order"], mid["ranges"], case[6],
                                  got["state"], *[d(u) for u in up[:3]])
    assert torch.equal(got["partial"], partial) and partial.any() and not got["partial_feat"].any()


def test_one_opaque_gaussian_at_a_pixel_centre(cuda):
    case = _flat_case([[8.5, 8.5]], 0.5, (16, 16))
    xyz, colour, feat, up = _inputs(case, 19)
    got, _ = _direct(cuda, case, colour, feat, up)
    assert torch.equal(got["feat_out"][0, :, 8, 8].cpu(), _t(feat[0] * gr.MAX_ALPHA))                 # the cap: w = 0.99 exactly


# ------------------------------------------------------------------------------------------------ the entry points raw, inside sentinels
def test_no_entry_point_writes_outside_its_outputs_or_follows_an_unchecked_value(cuda):
    from mudg_amd import hip
    case = _ids_case()
    pts, cov, op, ids, mats, cam, hw = case
    Fn = 19
    xyz, colour, feat, up = _inputs(case, Fn)
    lib = hip.lib()
    V, n, (H, W) = mats.shape[0], len(pts), hw

    def spoil(values, order, ranges, offsets):       # values outside the cloud, positions outside [0, E), ranges outside [0, E], offsets outside [0, E - count]
        values, order, ranges, offsets = values.clone(), order.clone(), ranges.clone(), offsets.clone()
        E = values.numel()
        values[::7], values[3::11] = -5, n
        order[::5], order[2::9] = -1, E
        ranges[1], ranges[2] = torch.tensor([-4, 3], dtype=torch.int32), torch.tensor([0, E + 1], dtype=torch.int32)
        flat = offsets.reshape(-1)
        flat[::6], flat[1::13], flat[2::17] = -1, E, E - 1
        return values, order, ranges, offsets

    for corrupt in (None, spoil):
        _, mid = _direct(cuda, case, colour, feat, up, corrupt)
        values, order, ranges, offsets = (mid[k].cpu().numpy() for k in ("values", "order", "ranges", "offsets"))
        E = len(values)
        proj = gr.project(xyz, cov, op, ids, mats, cam, hw)
        w_rgb, w_depth, w_alpha, w_state, w_feat = gf.blend_feat(proj, colour, feat, values, ranges, hw)
        w_partial, w_pfeat = gf.blend_bwd_feat(proj, colour, feat, values, order, ranges, hw, w_state, w_feat, *up)
        w_dfeat = gf.feat_bwd(proj["count"], offsets, w_pfeat)
        ro = lambda a: Flat(a.size, torch.float32, nan=True).put(_t(a), cuda)                          # operands a kernel only reads
        d = lambda a: _t(a).to(cuda)
        uv, conic, depth = d(proj["uv"]), d(proj["conic"]), d(proj["depth"])
        f_col, f_feat = ro(colour), ro(feat)
        rgb, dimg, alpha, fout, state = (Flat(V * c * H * W, torch.float32).blank(cuda) for c in (3, 1, 1, Fn, 5))
        hip.check(lib.mudg_gauss_blend_feat(f_col.ptr, 0, f_feat.ptr, Fn, uv.data_ptr(), conic.data_ptr(), depth.data_ptr(), mid["values"].data_ptr(),
                                            mid["ranges"].data_ptr(), n, E, V, H, W, rgb.ptr, dimg.ptr, alpha.ptr, fout.ptr, state.ptr, None), "blend_feat")
        torch.cuda.synchronize()
        for buf, k, w in ((rgb, "rgb", w_rgb), (dimg, "depth", w_depth), (alpha, "alpha", w_alpha), (fout, "feat_out", w_feat), (state, "state", w_state)):
            assert torch.equal(buf.read(k), _t(w).reshape(-1)), k
        partial, pfeat = Flat(E * 10, torch.float32).blank(cuda), Flat(E * Fn, torch.float32).blank(cuda)
        f_state, f_fout = ro(w_state), ro(w_feat)
        f_up = [ro(u) for u in up]
        hip.check(lib.mudg_gauss_blend_bwd_feat(f_col.ptr, 0, f_feat.ptr, Fn, uv.data_ptr(), conic.data_ptr(), depth.data_ptr(), mid["values"].data_ptr(),
                                                mid["order"].data_ptr(), mid["ranges"].data_ptr(), n, E, V, H, W, f_state.ptr, f_fout.ptr,
                                                f_up[0].ptr, f_up[1].ptr, f_up[2].ptr, f_up[3].ptr, partial.ptr, pfeat.ptr, None), "blend_bwd_feat")
        torch.cuda.synchronize()
        assert torch.equal(partial.read("partial"), _t(w_partial).reshape(-1))
        got_pfeat = pfeat.read("partial_feat")
        assert torch.equal(got_pfeat, _t(w_pfeat).reshape(-1))
        f_pfeat, out = ro(w_pfeat), Flat(n * Fn, torch.float32).blank(cuda)
        hip.check(lib.mudg_gauss_feat_bwd(mid["count"].data_ptr(), mid["offsets"].data_ptr(), f_pfeat.ptr, E, n, V, Fn, out.ptr, None), "feat_bwd")
        torch.cuda.synchronize()
        assert torch.equal(out.read("d_feat_g"), _t(w_dfeat).reshape(-1))
        for f in (f_col, f_feat, f_state, f_fout, f_pfeat, *f_up):
            f.unchanged("an operand")


# ------------------------------------------------------------------------------------------------ the class loss
def _scores_and_labels(V, Fn, hw, seed, outlier=True):
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(V, Fn) + hw) * 4.0).astype(F)
    x[0, :, 0, 0] = 0.0                                                                                # a tie across all classes
    if outlier:
        x[0, 0, -1, -1] = 200.0                                                                        # the others fall below the floor of -80
    labels = rng.integers(0, Fn, (V,) + hw).astype(np.uint8)
    flat = labels.reshape(-1)
    flat[::5], flat[1::7], flat[2::11] = Fn - 1, Fn, 255
    return x, labels


def _loss_check(cuda, x, labels, weight, up=0.75):
    from mudg_amd import hip
    lib = hip.lib()
    V, Fn, H, W = x.shape
    tx, ty = gr.tiles((H, W))
    w_maps, w_partial, w_totals = gf.class_loss(x, labels, weight)
    w_dx = gf.class_loss_bwd(w_maps, w_totals, up, weight)
    f_x = Flat(x.size, torch.float32, nan=True).put(_t(x), cuda)
    f_labels = Flat(labels.size, torch.uint8, fill=0).put(_t(labels), cuda)                            # padding that would count as class 0
    for _ in range(2):                                                                                 # a repeat gives the same bits
        maps, partial, totals, dx = (Flat(k, torch.float32).blank(cuda) for k in (x.size, V * tx * ty * 2, 4, x.size))
        hip.check(lib.mudg_gauss_class_loss(f_x.ptr, f_labels.ptr, V, Fn, H, W, maps.ptr, partial.ptr, None), "class_loss")
        torch.cuda.synchronize()
        got_maps, got_partial = maps.read("maps"), partial.read("partial")
        assert torch.equal(got_maps, _t(w_maps).reshape(-1)) and torch.equal(got_partial.view(torch.int32), _t(w_partial).reshape(-1).view(torch.int32))
        f_partial = Flat(got_partial.numel(), torch.float32, nan=True).put(got_partial, cuda)
        hip.check(lib.mudg_gauss_class_loss_finish(f_partial.ptr, V, H, W, weight, totals.ptr, None), "finish")
        torch.cuda.synchronize()
        got_totals = totals.read("totals")
        assert torch.equal(got_totals.view(torch.int32), _t(w_totals).view(torch.int32)), (got_totals, w_totals)
        f_maps, f_totals = Flat(x.size, torch.float32, nan=True).put(got_maps, cuda), Flat(4, torch.float32, nan=True).put(got_totals, cuda)
        f_up = Flat(1, torch.float32, nan=True).put(torch.tensor([up], dtype=torch.float32), cuda)
        hip.check(lib.mudg_gauss_class_loss_bwd(f_maps.ptr, f_totals.ptr, f_up.ptr, weight, V, Fn, H, W, dx.ptr, None), "class_loss_bwd")
        torch.cuda.synchronize()
        assert torch.equal(dx.read("d_x"), _t(w_dx).reshape(-1))
    f_x.unchanged("x")
    f_labels.unchanged("labels")
    return w_maps, w_totals


@pytest.mark.parametrize("Fn", [1, 3, 19, 32])
@pytest.mark.parametrize("hw", [(1, 1), (17, 33), (40, 56)])
def test_the_class_loss_is_the_rule(cuda, Fn, hw):
    x, labels = _scores_and_labels(2, Fn, hw, 3 * Fn + hw[0])
    maps, totals = _loss_check(cuda, x, labels, 0.1)
    assert np.isfinite(maps).all() and np.isfinite(totals[[0, 2, 3]]).all()
    if Fn == 1:
        assert not maps.any() and totals[0] == 0                                                       # one class: softmax is 1, the map +0


def test_an_unlabelled_view_beside_a_labelled_one(cuda):
    x, labels = _scores_and_labels(2, 19, (17, 33), 9)
    labels[1] = 255
    maps, totals = _loss_check(cuda, x, labels, 1.0)
    assert not maps[1].any() and maps[0].any()
    labels[0] = 19                                                                                     # and nothing labelled at all
    maps, totals = _loss_check(cuda, x, labels, 1.0)
    assert not maps.any() and totals[0] == 0 and totals[3] == 0 and totals[2] == 1 and totals[1:2].view(np.int32)[0] == 0


def test_class_loss_through_autograd(cuda):
    from mudg_amd import gaussians
    x, labels = _scores_and_labels(2, 19, (17, 33), 4, outlier=False)                                  # the floor is not the textbook's
    w_maps, _, w_totals = gf.class_loss(x, labels, 0.3)
    leaf = _t(x).to(cuda).requires_grad_(True)
    loss = gaussians.class_loss(leaf, _t(labels).to(cuda), weight=0.3)
    (loss * 2.0).backward()
    assert loss.item() == w_totals[3] and torch.equal(leaf.grad.cpu(), _t(gf.class_loss_bwd(w_maps, w_totals, 2.0, 0.3)))
    wide = _t(labels.astype(np.int64))
    wide[0, 0, :3] = torch.tensor([-1, 255, 4000])                                                     # int64 labels: outside 0 .. 254 -> unlabelled
    narrow = _t(labels).clone()
    narrow[0, 0, :3] = 255
    assert gaussians.class_loss(leaf, wide.to(cuda)).item() == gaussians.class_loss(leaf, narrow.to(cuda)).item()
    terms = gaussians.class_loss.terms(leaf, _t(labels).to(cuda), weight=0.3)
    assert terms["loss"].item() == w_totals[3] and terms["count"].item() == int((labels < 19).sum())
    ref = torch.nn.functional.cross_entropy(_t(x).double(), _t(labels).long().clamp(max=19).where(_t(labels) < 19, torch.tensor(-100)),
                                            ignore_index=-100)
    assert abs(loss.item() / 0.3 - ref.item()) <= 1e-5 * ref.item()                                    # two polynomials of 2e-7 and an fp32 mean


# ------------------------------------------------------------------------------------------------ through Python
def _leaves(cuda, *arrays):
    return [_t(a).to(cuda).requires_grad_(True) for a in arrays]


def test_render_with_and_without_features(cuda):
    from mudg_amd import gaussians, render
    pts, cov, op, ids, mats, cam, hw = _scene_case(200, (40, 56), 13, views=3)
    xyz, _, feat, _ = _inputs((pts, cov, op, ids, mats, cam, hw), 19)
    d_mats = _t(mats).to(cuda)
    g = gaussians.Gaussians(render.PointCloud(_t(pts).to(cuda)), _t(cov).to(cuda), _t(op).to(cuda))
    before = gaussians.render(g, d_mats, cam, hw)
    assert sorted(before) == ["alpha", "depth", "rgb"]
    with_feat = gaussians.Gaussians(g.cloud, g.cov, g.opacity, features=_t(feat).to(cuda))
    out = gaussians.render(with_feat, d_mats, cam, hw)
    after = gaussians.render(g, d_mats, cam, hw)
    for k in before:
        assert torch.equal(before[k].view(torch.int32), after[k].view(torch.int32)), k                # the call without features is what it was
        assert torch.equal(before[k], out[k]), k                                                       # whole bytes: the same images
    proj = gr.project(xyz, cov, op, ids, mats, cam, hw)
    keys, values, ranges = gr.bin_entries(proj, hw)
    words = gr.unpack(pts)[1]
    whole = np.stack([(words >> (8 * k)) & 0xff for k in range(3)], axis=1).astype(F)
    want = gf.blend_feat(proj, whole, feat, values, ranges, hw)
    assert torch.equal(out["features"].cpu(), _t(want[4]))
    assert out["labels"].dtype == torch.uint8 and torch.equal(out["labels"].cpu(), _t(gf.labels_of(want[4], want[2])))
    assert (out["labels"] == 255).any() and (out["labels"] < 19).any()
    strict = gaussians.render(with_feat, d_mats, cam, hw, label_alpha=0.9)
    assert torch.equal(strict["labels"].cpu(), _t(gf.labels_of(want[4], want[2], 0.9)))
    far = gaussians.Gaussians(g.cloud, g.cov, g.opacity, features=_t(feat).to(cuda))
    nothing = gaussians.render(far, d_mats, cam, hw, zfar=0.3)                                         # everything culled
    assert not nothing["features"].any() and (nothing["labels"] == 255).all() and nothing["features"].shape == (3, 19, 40, 56)


def test_render_differentiable_with_features_harmonics_and_matrices(cuda):
    from mudg_amd import gaussians, ops
    case = _scene_case(200, (40, 56), 13, views=3)
    pts, cov, op, ids, mats, cam, hw = case
    xyz, colour, feat, up = _inputs(case, 19)
    sh = (np.random.default_rng(8).normal(size=(len(xyz), 3, 3)) * 20).astype(F)
    plain = _leaves(cuda, xyz, colour, cov, op)
    d_mats = _t(mats).to(cuda)
    base = gaussians.render_differentiable(*plain, d_mats, cam, hw)
    leaves = _leaves(cuda, xyz, colour, cov, op)
    d_feat = _t(feat).to(cuda).requires_grad_(True)
    out = gaussians.render_differentiable(*leaves, d_mats, cam, hw, features=d_feat)
    assert len(out) == 4 and all(torch.equal(a, b) for a, b in zip(base, out))
    torch.autograd.backward(out, [_t(u).to(cuda) for u in up])
    want = gf.render_backward(xyz, colour, feat, cov, op, ids, mats, cam, hw, *up)
    assert torch.equal(out[3].cpu(), _t(want["feat_out"])) and torch.equal(d_feat.grad.cpu(), _t(want["d_feat_g"]))
    for leaf, k in zip(leaves, ("d_xyz", "d_colour", "d_cov", "d_opacity")):
        assert torch.equal(leaf.grad.cpu(), _t(want[k])), k
    # harmonics and the matrices' gradient together: every gradient is the existing kernels' on the partials of the feature backward
    leaves = _leaves(cuda, xyz, colour, cov, op)
    d_sh, d_feat, m = _t(sh).to(cuda).requires_grad_(True), _t(feat).to(cuda).requires_grad_(True), _t(mats).to(cuda).requires_grad_(True)
    out = gaussians.render_differentiable(*leaves, m, cam, hw, sh=d_sh, features=d_feat)
    torch.autograd.backward(out, [_t(u).to(cuda) for u in up])
    with torch.no_grad():
        p = gaussians._pack_xyz(leaves[0])
        b = gaussians._bin("test", p, leaves[2], leaves[3], m, cam, hw, None, gaussians.ZNEAR, gaussians.ZFAR, gaussians.MAX_ENTRIES)
        colours = ops.gauss_sh_colour(p, m, b.count, leaves[1], d_sh)
    w = gf.blend_feat(dict(uv=b.uv.cpu().numpy(), conic=b.conic.cpu().numpy(), depth=b.depth.cpu().numpy(), count=b.count.cpu().numpy()),
                      colours.cpu().numpy(), feat, b.values.cpu().numpy(), b.ranges.cpu().numpy(), hw)
    proj = dict(uv=b.uv.cpu().numpy(), conic=b.conic.cpu().numpy(), depth=b.depth.cpu().numpy(), count=b.count.cpu().numpy())
    w_partial, w_pfeat = gf.blend_bwd_feat(proj, colours.cpu().numpy(), feat, b.values.cpu().numpy(), b.order.cpu().numpy(),
                                           b.ranges.cpu().numpy(), hw, w[3], w[4], *up)
    for a, k in zip(out, (0, 1, 2, 4)):
        assert torch.equal(a.cpu(), _t(w[k]))
    assert torch.equal(d_feat.grad.cpu(), _t(gf.feat_bwd(proj["count"], b.offsets.cpu().numpy(), w_pfeat)))
    partial = _t(w_partial).to(cuda)
    with torch.no_grad():
        g_xyz, g_cov, g_op, _ = ops.gauss_project_bwd(p, leaves[2], m, cam, hw, b.count, b.offsets, partial)
        g_col, g_sh, g_dir = ops.gauss_sh_bwd(p, m, b.count, b.offsets, partial, leaves[1], d_sh)
        g_mats = ops.gauss_pose_bwd(p, leaves[2], m, cam, hw, b.count, b.offsets, partial) + ops.gauss_sh_pose_bwd(p, m, b.count, b.offsets, partial,
                                                                                                                  leaves[1], d_sh)
    for got, wanted, k in ((leaves[0].grad, g_xyz + g_dir, "xyz"), (leaves[1].grad, g_col, "colour"), (leaves[2].grad, g_cov, "cov"),
                           (leaves[3].grad, g_op, "opacity"), (d_sh.grad, g_sh, "sh"), (m.grad, g_mats, "mats")):
        assert torch.equal(got, wanted) and wanted.any(), k


def test_everything_culled_gives_zero_gradients(cuda):
    from mudg_amd import gaussians
    pts, cov, op, ids, mats, cam, hw = _flat_case([[8.5, 8.5], [3.0, 4.0]], 0.5, (17, 33), z=[250.0, 300.0])
    xyz, colour, feat, up = _inputs((pts, cov, op, ids, mats, cam, hw), 19)
    leaves = _leaves(cuda, xyz, colour, cov, op, feat)
    out = gaussians.render_differentiable(*leaves[:4], _t(mats).to(cuda), cam, hw, features=leaves[4])
    assert len(out) == 4 and out[3].shape == (1, 19, 17, 33) and not any(o.any() for o in out)
    sum(o.sum() for o in out).backward()
    for leaf in leaves:
        assert leaf.grad is not None and leaf.grad.shape == leaf.shape and not leaf.grad.any()


def test_fit_with_density_control_and_classes(cuda):
    from mudg_amd import gaussians
    start, views, cam, targets = gb.fit_problem()
    hw = (40, 56)
    model = gaussians.GaussianModel(*[_t(start[k]).to(cuda) for k in gaussians.PARAMETERS])
    plain = gaussians.GaussianModel(*[_t(start[k]).to(cuda) for k in gaussians.PARAMETERS])
    d_views, d_targets = _t(views).to(cuda), targets.to(torch.float32).to(cuda)
    labels = (torch.arange(56, device=cuda)[None, None, :] * 3 // 56).expand(3, 40, 56).to(torch.uint8).contiguous()
    labels[:, :4] = 255                                                                                # a band nobody labelled
    control = gaussians.DensityControl(2, 12, 4, grad_threshold=1e-6, split_scale=0.2, max_scale=5.0)
    losses = gaussians.fit(model, d_targets, d_views, cam, hw, iters=12, density=control, label_targets=labels, class_weight=0.1, classes=3)
    assert len(control.history) == 2 and control.history[-1]["after"] != len(start["xyz"])            # the model grew or shrank
    assert model.class_logits.shape == (len(model), 3) and model.class_logits.requires_grad and model.class_logits.any()
    assert set(model.parameters()) == set(gaussians.PARAMETERS) | {"class_logits"}
    out = gaussians.render(model.gaussians(), d_views, cam, hw)
    assert out["labels"].shape == (3, 40, 56) and out["features"].shape == (3, 3, 40, 56)
    # with the defaults nothing changes: the same losses as a fit that was never given labels
    a = gaussians.fit(plain, d_targets, d_views, cam, hw, iters=3, label_targets=labels, class_weight=0.0)
    again = gaussians.GaussianModel(*[_t(start[k]).to(cuda) for k in gaussians.PARAMETERS])
    assert a == gaussians.fit(again, d_targets, d_views, cam, hw, iters=3) and plain.class_logits is None
    assert all(np.isfinite(losses))


# ------------------------------------------------------------------------------------------------ the fit against its float64 counterpart
# tests/gaussians_feat_fit64.py on the CPU: cross-entropy 1.09861 -> 0.04598 after 200 float64 Adam steps over the textbook renderer
R64_CLASSES = 0.04185


def test_the_fit_lowers_the_class_loss_as_the_float64_loop_does(cuda):
    """gb.fit_problem with labels that are the argmax of a hidden labelled model rendered in float64: the ratio of the final to the
    initial class loss after the reference's 200 iterations is within 10 % of the float64 CPU fit's, the margin the harmonics and
    density fits use."""
    import gaussians_feat_fit64 as f64
    from mudg_amd import gaussians
    assert f64.CLASS_RATE == gaussians.CLASS_LEARNING_RATE
    start, views, cam, targets, labels = f64.class_fit_problem()
    mats, tgt, d_labels = _t(views).to(cuda), targets.to(torch.float32).to(cuda), _t(labels).to(cuda)
    model = gaussians.GaussianModel(*[_t(start[k]).to(cuda) for k in gaussians.PARAMETERS]).enable_classes(f64.CLASSES)

    def cross_entropy():
        with torch.no_grad():
            feat = gaussians.render_differentiable(model.xyz, model.colour, model.covariance(), model.opacity(), mats, cam, f64.HW,
                                                   features=model.class_logits)[3]
            return float(gaussians.class_loss(feat, d_labels))

    first = cross_entropy()
    losses = gaussians.fit(model, tgt, mats, cam, f64.HW, iters=f64.ITERS, label_targets=d_labels, class_weight=f64.CLASS_WEIGHT, classes=f64.CLASSES)
    last = cross_entropy()
    ratio = last / first
    print(f"fp32 fit with classes, {f64.ITERS} steps: cross-entropy {first:.5f} -> {last:.5f}, ratio {ratio:.5f} (float64: {R64_CLASSES})")
    assert len(losses) == f64.ITERS and abs(first - np.log(f64.CLASSES)) <= 1e-6
    assert abs(ratio / R64_CLASSES - 1) <= 0.10, (ratio, R64_CLASSES)
