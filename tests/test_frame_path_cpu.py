"""What the GPU tests of the frame path (tests/test_frame_path_kernels_gpu.py) rest on, checked without a GPU: the entry-point level
definitions of tests/frame_path_raw_reference.py equal the existing definitions on well-formed input, their extra rules (a spoiled
table entry clamped, counts added to what hist held, a key the minimum of what it held and what lands, resolve leaving both key images
empty, stream placement by the header's formula, post.hip's fp32 operations) hold by hand, and every case of tests/frame_path_cases.py
reaches the clause it names — a branch of the definition (the result changes without the rule) or a launch shape (the lane and
workgroup counts come out as stated): a case that stops reaching it fails here, before any GPU run."""
import numpy as np

import frame_path_cases as fc
import frame_path_raw_reference as raw
import frames_reference as fr
import lidar_depth_reference as ld
import normals_reference as nm
import splat_cases as pc
import splat_reference as sr

F, D = np.float32, np.float64


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _zeros(*shape):
    return np.zeros(shape, dtype=np.uint64)


# ------------------------------------------------------------------------------------------------ raw definitions = the existing ones
def test_raw_resize_definitions_equal_the_existing_ones_on_well_formed_input():
    for width in fc.RESIZE_SHAPES:
        c = fc.resize_case(width)
        hw = (c["H"], c["W"])
        (xu, yu), (xn, yn), (xf, yf) = (c["tables"][k] for k in ("u8", "nearest", "f32"))
        for src in (c["u8_1"], c["u8_3"]):
            assert _same(raw.resize_u8(src, xu, yu), fr.resize_u8_linear(src, hw)) and _same(raw.resize_u8(src, xn, yn, raw.NEAREST), fr.resize_u8_nearest(src, hw))
        assert _same(raw.resize_u8(c["ids"], xu, yu, palette=True), fr.resize_u8_linear(fr.colourise(c["ids"]), hw))
        assert _same(raw.resize_f32(c["f32"], xf, yf), fr.resize_f32_linear(c["f32"], hw))
        for kind, src, whole in ((raw.COLOUR, c["u8_3"], fr.colour_stream), (raw.SEMANTIC, c["ids"], fr.semantic_stream)):
            planes, u8 = raw.dense_stream(kind, src, xu, yu, c["norm"])
            want_planes, want_u8 = whole(src, hw)
            assert _same(planes, want_planes) and _same(u8, want_u8)
        planes, u8 = raw.dense_stream(raw.DEPTH, c["metres"], xf, yf)
        assert u8 is None and _same(planes, fr.depth_stream(c["metres"], hw))
        assert _same(raw.normal_stream(c["normals"], xf, yf), nm.normal_stream(c["normals"], hw))
        assert (xu[:, 2] + xu[:, 3] == 2048).all() and (yu[:, 2] + yu[:, 3] == 2048).all()


def test_raw_normals_definitions_equal_the_existing_ones_on_well_formed_input():
    c = fc.normals_case((5, 7))
    for labels in (None, c["labels"]):
        for r in (-1.0, fc.REL_STEP):
            n, v = raw.depth_normals(c["depth"], c["table"], labels, fc.SKY, fc.MIN_DEPTH, fc.MAX_DEPTH, r)
            for f in range(2):
                wn, wv = nm.depth_normals(c["depth"][f], c["table"][f], None if labels is None else labels[f], fc.SKY, fc.MIN_DEPTH, fc.MAX_DEPTH, None if r < 0 else r)
                assert _same(n[f], wn) and _same(v[f], wv)
    s = fc.score_case((37, 53))
    hist = raw.metric_normals(s["pred"], s["gt"], s["valid"], _zeros(2, 720))
    for f in range(2):
        assert np.array_equal(hist[f].astype(np.int64), nm.normal_hist(s["pred"][f], s["gt"][f], s["valid"][f]))


def test_raw_lidar_definitions_equal_the_existing_ones_on_well_formed_input():
    """One segment, no ids, empty keys, the occluders drawn from the candidates: the key image resolves to lidar_depth_reference's map."""
    c = fc.visible_case(3)
    H, W, n = c["H"], c["W"], len(c["xyz"])
    empty = np.full((H, W), sr.EMPTY, dtype=np.uint64)
    keys, hid = raw.lidar_splat_visible(c["xyz"], None, c["segments"], c["mats"], c["occluders"], empty, fc.CAM, c["size"], 4, F(1.0 - 0.05))
    depth, after = raw.lidar_depth_resolve(keys)
    want, want_hidden = ld.lidar_depth(c["xyz"], c["mats"][0], fc.CAM, H, W, point_size=c["size"], reach=4, rel_tol=0.05, return_hidden=True)
    assert _same(depth, want) and np.array_equal(hid, want_hidden) and hid.any() and not hid.all() and (after == sr.EMPTY).all()
    keys, hid = raw.lidar_splat_visible(c["xyz"], None, c["segments"], c["mats"], None, empty, fc.CAM, c["size"])
    assert np.array_equal(keys, sr.splat_keys(c["xyz"], c["mats"][0], fc.CAM, c["size"], H, W)) and not hid.any()
    d = fc.complete_case((33, 65))
    for extrapolate in (0, 1):
        out, source = raw.depth_complete(d["depth"], d["labels"], fc.SKY, fc.COMPLETE_M, extrapolate)
        for f in range(2):
            wo, ws = ld.complete_depth(d["depth"][f], d["labels"][f], fc.COMPLETE_M, bool(extrapolate), fc.SKY)
            assert _same(out[f], wo) and _same(source[f], ws)


# ------------------------------------------------------------------------------------------------ the extra rules, by hand
def test_a_spoiled_table_entry_is_clamped_into_the_source():
    t = np.array([[-1, 3, 2048, 0], [1, 2, 1024, 1024], [-7, 9, 0, 2048]], dtype=np.int32)
    assert raw.clamped(t, 3).tolist() == [[0, 2, 2048, 0], [1, 2, 1024, 1024], [0, 2, 0, 2048]]
    assert raw.spoiled(raw.table_u8(5, 4), 5)[[0, 0, -1, -1], [0, 1, 0, 1]].tolist() == [-1, 5, -1, 5]
    src = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3, 1) * 10
    out = raw.resize_u8(src, t, t)
    assert out[0, :, :, 0].tolist() == [[0, 15, 20], [45, 60, 65], [60, 75, 80]]                      # rows 0, (1 + 2) / 2, 2 of columns 0, (1 + 2) / 2, 2
    f = np.array(t)
    f[:, 2:] = F([[1, 0], [0.5, 0.5], [0, 1]]).view(np.int32)
    assert raw.resize_f32(src[..., 0].astype(F), f, f)[1].tolist() == [[90, 105, 110], [135, 150, 155], [150, 165, 170]]


def test_stream_placement_follows_the_headers_address_formula():
    off = raw.stream_offsets(2, 2, 4, 100, 30, 8, 1, 1)
    assert off.shape == (3, 2, 2, 4) and off[0, 0, 0, 0] == 100 + 8 and off[2, 1, 1, 3] == 100 + 2 * 8 + 2 * 30 + 4 + 3
    before = np.full(200, 0xA5A5A5A5, dtype=np.uint32).view(np.int32)
    planes = np.arange(48, dtype=F).reshape(3, 2, 2, 4)
    after = raw.placed(before, planes, off)
    assert after.dtype == np.int32 and (after[off.reshape(-1)].view(F) == planes.reshape(-1)).all()
    rest = np.ones(200, dtype=bool)
    rest[off.reshape(-1)] = False
    assert (after[rest] == before[rest]).all() and rest.sum() == 200 - 48


def test_counts_are_added_to_what_hist_held():
    s = fc.score_case((5, 7))
    start = fc.start_sums((2, 720), 3)
    assert np.array_equal(raw.metric_normals(s["pred"], s["gt"], s["valid"], start) - start, raw.metric_normals(s["pred"], s["gt"], s["valid"], _zeros(2, 720)))
    assert raw.added(np.array([2 ** 64 - 1], dtype=np.uint64), [2]).tolist() == [1]


def test_a_key_is_the_minimum_of_what_it_held_and_what_lands_and_resolve_empties_both_images():
    xyz = pc._pixels_to_points([0.5], [0.5], [2.0])
    seg = np.array([[0, 1]], dtype=np.int64)
    landed = int(raw.make_keys(F(2.0), 0))
    for held, want in ((sr.EMPTY, landed), (raw.make_keys(F(1.0), 9), int(raw.make_keys(F(1.0), 9))), (raw.make_keys(F(3.0), 9), landed), (np.uint64(landed + 1), landed),
                       (np.uint64(landed - 1), landed - 1)):
        keys, _ = raw.lidar_splat_visible(xyz, None, seg, pc.EYE[None], None, np.full((1, 1), held, dtype=np.uint64), fc.CAM, 1.0)
        assert int(keys[0, 0]) == want
    keys, _ = raw.lidar_splat_visible(xyz, None, seg, pc.EYE[None], None, np.full((1, 1), sr.EMPTY, dtype=np.uint64), fc.CAM, 1.0, index_base=2 ** 32 - 1)
    assert int(keys[0, 0]) == landed + 2 ** 32 - 1                                                     # the last index a key holds: index_base + n = 2^32
    depth, after = raw.lidar_depth_resolve(np.array([sr.EMPTY, np.uint64(0x7FC0000100000005), raw.make_keys(F(2.5), 1)]))
    assert depth.view(np.uint32).tolist() == [0, 0x7FC00001, 0x40200000] and (after == sr.EMPTY).all() and after.shape == (3,)
    assert raw.candidate_points([[5, 2], [0, 3], [5, 1]]).tolist() == [5, 6, 0, 1, 2, 5]
    assert raw.complete_scratch(2, 3, 5) == 2 * 128 + 32 and raw.complete_scratch(1, 1, 1) == 48 and raw.complete_scratch(2, 2, 8) == 2 * 128 + 32


def test_post_definitions_by_hand():
    x = F([np.nan, -np.inf, -1.5, -1, 0, 2 / 255 - 1, 1, 7, np.inf])
    assert raw.clamp_unit(x).tolist() == [-1, -1, -1, -1, 0, F(2 / 255 - 1), 1, 1, 1]
    assert raw.frames_to_u8(x.reshape(1, 1, 1, 9)).reshape(-1).tolist() == [0, 0, 0, 0, 127, 0, 255, 255, 255]   # (2/255 - 1 + 1) / 2 * 255 = 0.99999..: truncated
    v = F([[0.0, 1.0, 0.5, 0.25]]).reshape(1, 1, 1, 1, 4)
    assert raw.log_sheet(v, 0, 0).reshape(-1).tolist() == [0, 0, 0, 255, 255, 255, 127, 127, 127, 63, 63, 63]
    assert raw.log_sheet(v * 2 - 1, 0, 1).reshape(-1).tolist() == raw.log_sheet(v, 0, 0).reshape(-1).tolist()
    two = np.arange(2 * 3 * 1 * 1 * 2, dtype=F).reshape(2, 3, 1, 1, 2) / 255                           # sample n, channel c, column w holds (6 n + 2 c + w) / 255
    assert raw.log_sheet(two, 0, 0).shape == (1, 2, 2, 3) and raw.log_sheet(two, 0, 0).reshape(-1).tolist() == [0, 2, 4, 1, 3, 5, 6, 8, 10, 7, 9, 11]
    assert _same(raw.depth_from_u8(np.uint8([[0, 0, 0], [0, 0, 1], [255, 255, 255]])), F([0, F(F(1) / F(3)) / F(255), 1]))
    img = np.uint8([[255, 255], [120, 0], [50, 0]])
    vis, labels = raw.semantic_nearest(img)
    assert labels.tolist() == [0, 6] and vis.T.tolist() == [[255, 120, 50], [255, 0, 0]]
    # video (B, C, T, HW) -> (B, T, HW, C)
    vid = fc.filled(F([-1, 1]), (2, 3, 2, 1), 0)
    assert raw.frames_to_u8(vid).shape == (2, 2, 1, 3)


# ------------------------------------------------------------------------------------------------ the cases reach their clauses
def test_resize_cases_have_the_row_shapes_they_name_and_reach_the_clamp():
    assert [fc.row_lanes(w) for w in (4, 5, 516, 513)] == [(1, 1, 4), (1, 2, 1), (2, 1, 4), (2, 1, 1)]
    grew, shrank = False, False
    for width in fc.RESIZE_SHAPES:
        c = fc.resize_case(width)
        assert c["W"] == width and c["H"] in (2, 3) and c["H0"] * c["W0"] * 3 <= 5 * 11 * 3 and (c["W0"] + 1) * 3 <= 36 and c["clause"]
        grew |= c["W"] > c["W0"]
        shrank |= c["W"] < c["W0"] and c["W0"] % c["W"] != 0
        for k in ("u8_1", "u8_3", "ids", "metres", "f32", "normals"):
            assert not _same(c[k][0], c[k][1])
        assert set(fc.PALETTE_IDS) <= set(c["ids"][0].reshape(-1).tolist()) and set(fc.PALETTE_IDS) <= set(c["ids"][1].reshape(-1).tolist())
        assert raw.resize_u8(c["ids"], *c["tables"]["u8"], palette=True).any()
        # the spoiled tables: one sample past either end; a definition that used them unclamped reads elsewhere and differs
        for kind, (xt, yt) in c["spoiled"].items():
            good = c["tables"][kind]
            assert xt[:, :2].min() == -1 and xt[:, :2].max() == c["W0"] and yt[:, :2].min() == -1 and yt[:, :2].max() == c["H0"]
            assert np.array_equal(xt[:, 2:], good[0][:, 2:]) and np.array_equal(raw.clamped(yt, c["H0"])[1:-1], good[1][1:-1])
            pad = lambda s: np.pad(s, [(0, 0), (1, 1), (1, 1)] + [(0, 0)] * (s.ndim - 3), constant_values=np.nan if s.dtype == F else 0xA5)
            shift = lambda t: np.concatenate([t[:, :2] + 1, t[:, 2:]], axis=1)
            if kind == "f32":
                unclamped = raw.resize_f32(pad(c["f32"]), shift(xt), shift(yt), clamp=False)
                assert not _same(unclamped, raw.resize_f32(c["f32"], xt, yt)) and np.isnan(unclamped).any()
            else:
                mode = raw.NEAREST if kind == "nearest" else raw.LINEAR
                assert not _same(raw.resize_u8(pad(c["u8_3"]), shift(xt), shift(yt), mode, clamp=False), raw.resize_u8(c["u8_3"], xt, yt, mode))
        # the last column's and the last row's second tap is min(s + 1, n - 1): s + 1 would read the (NaN) padding
        xf, yf = c["tables"]["f32"]
        assert xf[-1, 1] == c["W0"] - 1 and yf[-1, 1] == c["H0"] - 1 and (xf[-1, 0] == c["W0"] - 1) == (c["W"] > c["W0"])
        if c["W"] > c["W0"]:                                                             # an enlargement: the last sample is the last source, weight 0 on the tap after it
            wrong = np.array(xf)
            wrong[-1, 1] += 1
            assert xf[-1, 3] == 0 and np.isnan(raw.resize_f32(np.pad(c["f32"], [(0, 0), (0, 0), (0, 1)], constant_values=np.nan), wrong, yf, clamp=False)[:, :, -1]).all()
        if c["H"] > c["H0"]:
            wrong = np.array(yf)
            wrong[-1, 1] += 1
            assert yf[-1, 3] == 0 and np.isnan(raw.resize_f32(np.pad(c["f32"], [(0, 0), (0, 1), (0, 0)], constant_values=np.nan), xf, wrong, clamp=False)[:, -1]).all()
        # the depth stream: what is not a number stays so, both clamps bind, and values lie between
        planes, _ = raw.dense_stream(raw.DEPTH, c["metres"], xf, yf)
        p = planes[0]
        assert np.isnan(p).any() and (p == -1).any() and (p == 1).any() and ((p > -1) & (p < 1)).any() and (c["metres"] < 0).any() and (c["metres"] > 100).any()
    assert grew and shrank
    c = fc.resize_case(5)                                                                # both axes grow: the corner samples are the corner sources
    d = raw.resize_f32(c["metres"], *c["tables"]["f32"])
    assert d[0, 0, 0] == 100 and d[0, -1, -1] == 0 and np.isnan(d[1, 0, 0]) and d[1, -1, -1] == 150
    assert raw.depth_norm(F([np.nan, -5, 0, 100, 101, 50])).tolist()[1:] == [-1, -1, 1, 1, 0] and np.isnan(raw.depth_norm(F([np.nan]))[0])


def test_stream_layouts_falsify_each_term_alone():
    for width in (4, 516):
        c = fc.resize_case(width)
        falsified = []
        for name in fc.STREAM_LAYOUTS:
            lay = fc.stream_layout(name, c["H"], c["W"])
            off = raw.stream_offsets(2, c["H"], c["W"], lay["ss"], lay["cs"], lay["fs"], fc.SLAB, fc.FRAME0)
            assert off.min() == lay["ss"] + lay["fs"] and off.max() < lay["n"] and len(np.unique(off)) == off.size and lay["fs"] >= c["H"] * c["W"]
            wrong = [k for k, v in lay["terms"].items() if not v]
            assert len(wrong) <= 1, (name, wrong)
            falsified += wrong
        assert sorted(falsified) == ["cs", "dst", "fs", "u8"]                            # W % 4 is falsified by the widths 5 and 513
    lay = fc.stream_layout("frames outermost", 2, 4)
    assert (lay["cs"], lay["fs"]) == (8, 24) and all(lay["terms"].values())
    assert not fc.stream_layout("planar", 3, 5)["terms"]["W"]


def _neighbour_sets(c, f, r, lo=fc.MIN_DEPTH, hi=fc.MAX_DEPTH):
    """Per pixel of frame f which of left, right, up, down count (nm's rule restated on the usable mask)."""
    z = c["depth"][f].astype(D)
    with np.errstate(all="ignore"):
        usable = (z > lo) & (z < hi) & (c["labels"][f] != fc.SKY)
        out = {}
        for name, (dj, di) in (("left", (0, -1)), ("right", (0, 1)), ("up", (-1, 0)), ("down", (1, 0))):
            out[name] = nm._moved(usable, dj, di, False) & (np.abs(nm._moved(z, dj, di, D(0)) - z) <= D(r) * z)
    return usable, out


def test_normals_cases_reach_the_frame_boundary_and_their_special_pixels():
    assert [fc.lanes(hw, hw[1] % 4 == 0) for hw in fc.PIXEL_SIZES] == [(3, 3), (258, 2), (35, 35), (1961, 169)]
    args = (fc.SKY, fc.MIN_DEPTH, fc.MAX_DEPTH)
    for hw in fc.PIXEL_SIZES:
        c = fc.normals_case(hw)
        H, W = hw
        assert not _same(c["depth"][0], c["depth"][1]) and (c["labels"] == fc.SKY).any()
        for labels in (None, c["labels"]):
            for r in (-1.0, fc.REL_STEP):
                n, v = raw.depth_normals(c["depth"], c["table"], labels, *args, r)
                n2, v2 = raw.depth_normals(c["depth"], c["table"], labels, *args, r, across=True)
                assert 0 < v.sum() < v.size
                for f, j, i in c["special"]["boundary"]:
                    assert v[f, j, i] == 0 and not n[f, j, i].any() and v2[f, j, i] == 1, (hw, f, j, i)      # a neighbour across the boundary would validate it
        n, v = raw.depth_normals(c["depth"], c["table"], c["labels"], *args, fc.REL_STEP)
        assert not _same(v, raw.depth_normals(c["depth"], c["table"], None, *args, fc.REL_STEP)[1])          # the sky rule binds
        if "step" not in c["special"]:
            continue
        for k, z in enumerate(fc.NORMAL_DEPTHS):
            at = (0, 1 + k % (H - 2), 3 + k // (H - 2))
            assert _same(c["depth"][at], F(z)) and v[at] == 0
        usable = lambda lo, hi: _neighbour_sets(dict(c, depth=c["depth"]), 0, np.inf, lo, hi)[0]
        assert not usable(fc.MIN_DEPTH, fc.MAX_DEPTH)[[1, 2 if H > 3 else 1], 3].any()
        assert usable(fc.MIN_DEPTH - 0.01, fc.MAX_DEPTH)[1, 3] and usable(fc.MIN_DEPTH, fc.MAX_DEPTH + 0.01)[2, 3]    # on the bound is outside: a bound moved by 0.01 takes it in
        f, j, i = c["special"]["step"]
        assert c["depth"][f, j, i - 1:i + 2].tolist() == [6, 8, 10] and v[f, j, i] == 1
        tighter = raw.depth_normals(c["depth"], c["table"], c["labels"], *args, np.nextafter(fc.REL_STEP, 0))
        assert not _same(tighter[0][f, j, i], n[f, j, i])                                  # both horizontal neighbours sit exactly on r z
        f, j, i = c["special"]["low_word"]
        assert c["labels"][f, j, i] == fc.LOW_WORD_SKY and v[f, j, i] == 1
        low = (c["labels"] & 0xFFFFFFFF).astype(np.int64)
        assert raw.depth_normals(c["depth"], c["table"], low, *args, fc.REL_STEP)[1][f, j, i] == 0          # a test on the low word drops it
        if H * W > 1000:                                                                   # pixels with one neighbour only on an axis, each kind
            for f in range(2):
                _, nb = _neighbour_sets(c, f, fc.REL_STEP)
                ok = v[f] == 1
                for only, other in (("left", "right"), ("right", "left"), ("up", "down"), ("down", "up")):
                    assert (ok & nb[only] & ~nb[other]).any(), (hw, f, only)


def test_score_cases_have_the_launch_shapes_and_the_special_pixels_they_name():
    assert [fc.score_launch(hw) for hw in fc.SCORE_SIZES] == [(4, 1, 1), (4, 1, 2), (1, 1, 1), (1, 1, 8), (4, 1, 1), (4, 2, 5), (1, 2, 17)]
    assert 43 * 192 == 8256 > fc.SCORE_PIXELS and 91 * 91 == 8281 and (2 * 6) % 4 == 0 and 6 % 4 != 0
    for hw in fc.SCORE_SIZES:
        c = fc.score_case(hw)
        n = hw[0] * hw[1]
        whole = raw.metric_normals(c["pred"], c["gt"], c["valid"], _zeros(2, 720))
        assert set(fc.VALID_BYTES) <= set(c["valid"].reshape(-1).tolist()) or n < 35
        assert not np.array_equal(whole, raw.metric_normals(c["pred"], c["gt"], None, _zeros(2, 720))) or n < 35       # validity binds
        assert not np.array_equal(whole, raw.metric_normals(c["pred"], c["gt"], (c["valid"] == 1).astype(np.uint8), _zeros(2, 720))) or n < 35     # any nonzero byte counts
        for f in range(2):
            for at in (0, n - 1):                                                          # dropping the first or the last lane shows
                v = np.array(c["valid"][f]).reshape(-1)
                v[at] = 0
                assert not np.array_equal(nm.normal_hist(c["pred"][f], c["gt"][f], v.reshape(hw)), whole[f].astype(np.int64))
        if not c["special"]:
            continue
        s = c["special"]
        pred, gt = c["pred"][0].reshape(-1, 3), c["gt"][0].reshape(-1, 3)
        cos, gg = nm.cosines(pred, gt)
        assert gg[s["zero"]] == 0 and np.isnan(gg[s["nan"]]) and np.isinf(gg[s["inf"]]) and cos[s["above"]] > 1 and cos[s["below"]] < -1 and cos[s["right_angle"]] == 0
        assert cos[s["plus_one"]] == 1 and cos[s["minus_one"]] == -1
        one = lambda k: nm.normal_hist(pred[k:k + 1], gt[k:k + 1]).tolist()
        assert one(s["zero"]) == one(s["nan"]) == one(s["inf"]) == [0] * 720
        assert one(s["above"])[0] == 1 and one(s["plus_one"])[0] == 1 and one(s["below"])[719] == 1 and one(s["minus_one"])[719] == 1 and one(s["right_angle"])[360] == 1
    h = raw.metric_normals(*(fc.score_case((5, 7))[k] for k in ("pred", "gt", "valid")), _zeros(2, 720))
    assert h[1, 0] == (fc.score_case((5, 7))["valid"][1] != 0).sum() > 0 and not h[1, 1:].any() and (h[0] > 0).sum() > 3       # a frame in one bin


def _visible(c, Z="own", **kw):
    Z = c["occluders"] if isinstance(Z, str) else Z
    return raw.lidar_splat_visible(c["xyz"], c["ids"], c["segments"], c["mats"], Z, c["keys"], fc.CAM, c["size"], **kw)


def test_visible_cases_reach_the_minimum_the_segments_and_every_occluder_rule():
    assert fc.SPLAT_IMAGES == tuple(hw for hw in pc.IMAGE_SIZES if hw != (1, 7)) and fc.SPLAT_CLOUDS == pc.CLOUD_SIZES
    for k in range(4):
        c = fc.visible_case(k)
        keys, hid = _visible(c, reach=4, rel_keep=F(0.95))
        won = keys != c["keys"]
        kind = c["kind"]
        assert int(raw.candidate_points(c["segments"])[-1]) == fc.SPLAT_CLOUDS[k] - 1 and won.any()
        assert (keys <= c["keys"]).all() and not won[kind == 1].any()                     # a nearer key stays
        if k >= 2:
            assert won[kind == 0].any() and won[kind == 2].any() and (~won)[kind == 2].any() and hid.any() and not hid.all()
            assert not np.array_equal(keys, _visible(c, reach=4, rel_keep=F(0.95), minimum=False)[0])       # stored instead of minimised: differs
            results = [keys] + [_visible(c, **kw)[0] for kw in (dict(reach=1, rel_keep=F(0.95)), dict(reach=16, rel_keep=F(0.95)), dict(reach=4, rel_keep=F(1.0)))]
            results.append(_visible(c, Z=None)[0])
            assert all(not np.array_equal(a, b) for i, a in enumerate(results) for b in results[i + 1:])   # every variant is a result of its own
            last = fc.SPLAT_CLOUDS[k] - 1
            assert (keys & np.uint64(0xFFFFFFFF) == np.uint64(last)).any()                 # the last lane's point shows
    e = fc.segments_case("eight")
    starts = np.cumsum([0] + [n for _, n in fc.EIGHT_RUNS])
    assert len(fc.EIGHT_RUNS) == 8 and starts[-1] == 300 and any(a < 256 < b for a, b in zip(starts[:-1], starts[1:])) and 256 not in starts
    keys, hid = _visible(e, reach=4, rel_keep=F(0.95))
    at = raw.candidate_points(e["segments"])
    assert not np.array_equal(at, np.sort(at)) and {-1, 3, pc.INT32_MIN, pc.INT32_MAX} <= set(e["ids"][at].tolist())
    numbers = np.array(e["keys"] != keys) * (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert numbers.max() >= 256 and (numbers[e["keys"] != keys] < 8).any()                # both workgroups and the clamped ids land
    by_number = dict(e, ids=np.ascontiguousarray(e["ids"][:300]))                          # ids read at the candidate's number instead: differs
    shuffled = raw.lidar_splat_visible(e["xyz"][at], by_number["ids"], np.array([[0, 300]]), e["mats"], e["occluders"], e["keys"], fc.CAM, e["size"], 4, F(0.95))[0]
    assert not np.array_equal(shuffled, keys)
    t = fc.segments_case("twice")
    keys, _ = _visible(t, Z=None)
    won = keys != t["keys"]
    assert won.any() and ((keys[won] & np.uint64(0xFFFFFFFF)) < 50).all() and t["segments"].tolist() == [[400, 50], [400, 50]]
    p = fc.probe_case()
    keys, hid = _visible(p, reach=fc.PROBE_REACH, rel_keep=F(fc.PROBE_KEEP))
    assert hid.tolist() == p["want_hidden"].tolist() == [q[2] for q in fc.PROBES]
    shown = set((keys[keys != sr.EMPTY] & np.uint64(0xFFFFFFFF)).astype(np.int64).tolist())
    assert shown == {i for i, q in enumerate(fc.PROBES) if not q[2]} and fc.LIMIT == F(9.5)
    assert keys[30, 0] != sr.EMPTY and fc.PROBES[-1][0][1] == -1                           # the probe whose home is outside lands on column 0
    either = _visible(p, reach=fc.PROBE_REACH, rel_keep=F(fc.PROBE_KEEP), both_sides=False)[1]
    assert either.tolist() != hid.tolist() and either[2] and either[8]
    for d, probe in enumerate((3, 4, 5, 6)):                                               # each direction alone hides its probe and no other
        rest = tuple(x for k, x in enumerate(ld.DIRECTIONS) if k != d)
        assert not _visible(p, reach=fc.PROBE_REACH, rel_keep=F(fc.PROBE_KEEP), directions=rest)[1][probe]
        assert _visible(p, reach=fc.PROBE_REACH, rel_keep=F(fc.PROBE_KEEP), directions=(ld.DIRECTIONS[d],))[1][probe]
    assert not _visible(p, reach=3, rel_keep=F(fc.PROBE_KEEP))[1][0] and _visible(p, reach=5, rel_keep=F(fc.PROBE_KEEP))[1][1]
    assert _visible(p, reach=fc.PROBE_REACH, rel_keep=F(1.0))[1][7]                        # the depth on the limit is nearer under any larger limit


def test_resolve_cases_hold_empty_keys_and_odd_words():
    for pixels in fc.RESOLVE_PIXELS:
        for full in (False, True):
            c = fc.resolve_case(pixels, full)
            depth, _ = raw.lidar_depth_resolve(c["keys"])
            assert len(c["keys"]) == pixels and (c["keys"] == sr.EMPTY).any() != full and not (c["occluders"] == sr.EMPTY).all()
            if pixels > 1:
                assert depth.view(np.uint32)[1:7].tolist() == list(fc.ODD_WORDS) and depth[-1] == 17.25
                assert np.isnan(depth[1]) and depth.view(np.uint32)[2] == 0x80000000 and depth[2] == 0       # a copy made through arithmetic could lose either


def test_complete_cases_reach_the_seam_the_tiles_and_the_frame_boundary():
    assert [(-(-h // 32), -(-w // 32)) for h, w in fc.COMPLETE_SIZES] == [(1, 1), (1, 2), (2, 1), (1, 2), (2, 3), (1, 10)]
    for hw in fc.COMPLETE_SIZES:
        c = fc.complete_case(hw)
        assert not _same(c["depth"][0], c["depth"][1]) and (c["labels"] == fc.SKY).any()
        results = {(e, l): fc.complete_want(hw, e, l) for e in (0, 1) for l in (False, True)}
        assert not _same(results[0, True][0], results[0, False][0]) and (results[1, True][1] == 4).any()
        if hw[0] * hw[1] >= 40 and hw != (3, 300):
            x1 = ld.step1(c["depth"][0], fc.COMPLETE_M).reshape(-1)
            assert not x1[3:3 + len(fc.COMPLETE_SPECIAL)].any() and x1[-1] == 70 and ld.step1(c["depth"][1], fc.COMPLETE_M)[0, 0] == (0 if hw == (31, 33) else 40)
            assert not _same(results[0, False][0], results[1, False][0])                   # the extrapolation changes the map
            assert {1, 2} <= set(results[0, False][1].reshape(-1).tolist()) and 3 in results[1, False][1]
    # the seam: after step 4 the value has reached column 250, the 31-wide maximum carries it to 265 and no further
    c = fc.complete_case((3, 300))
    _, _, (x1, x4, x5, x6, x7) = ld.complete_depth(c["depth"][0], None, fc.COMPLETE_M, True, stages=True)
    cols = lambda x: np.nonzero((x >= ld.EMPTY_BELOW).any(axis=0))[0]
    assert cols(x1).tolist() == [fc.SEAM_COLUMN] and cols(x4).max() == 250 and cols(x5).max() == 265 and cols(x5).min() == 225
    out, source = fc.complete_want((3, 300), 1, False)
    assert (out[0, :, 256:266] > 0).all() and source[0, 1, 265] == 3 and not out[0, :, 268:].any() and 0 in source
    # the frame boundary: frame 0 is full at the bottom, frame 1 empty at the top; a halo across the boundary would fill
    c = fc.complete_case((31, 33))
    assert (c["depth"][0, -3:] > 0.1).all() and not c["depth"][1, :10].any()
    for e in (0, 1):
        out, _ = fc.complete_want((31, 33), e, False)
        across, _ = raw.depth_complete(c["depth"], None, fc.SKY, fc.COMPLETE_M, e, across=True)
        assert not _same(out[1, :4], across[1, :4]) and (e == 1 or not out[1, :3].any()) and across[1, 0].all()
    stale = np.full(4, fc.STALE, dtype=np.uint8)
    assert stale.view(F)[0] >= ld.EMPTY_BELOW and stale[0] != 0


def test_post_cases_hold_every_byte_boundary_and_the_ties():
    v = fc.unit_values()
    assert len(v) == 3 * 256 + 11 and np.isnan(v).sum() == 1 and np.isinf(v).sum() == 2 and (v < -1).sum() >= 4 and (v > 1).sum() >= 4
    inside = v[np.isfinite(v) & (np.abs(v) <= 1)]
    b = raw.frames_to_u8(inside.reshape(1, 1, 1, -1)).reshape(-1)
    assert set(b.tolist()) == set(range(256))
    k = np.arange(256)
    exact = raw.frames_to_u8(v[256:512].reshape(1, 1, 1, -1)).reshape(-1).astype(np.int64)
    below = raw.frames_to_u8(v[:256].reshape(1, 1, 1, -1)).reshape(-1).astype(np.int64)
    assert (np.abs(exact - k) <= 1).all() and (exact != below).any() and (exact == k).sum() > 128      # the neighbours straddle byte boundaries
    for C in (1, 3):
        for HW in fc.U8_HW:
            vid = fc.u8_video(C, HW)
            assert vid.shape == (2, C, 2, HW) and not _same(vid[0], vid[1]) and np.isnan(vid).any()
        assert set(raw.frames_to_u8(fc.u8_video(C, 257)).reshape(-1).tolist()) == set(range(256))
        for hw in fc.SHEET_SIZES:
            for clamp, rescale in fc.SHEET_SETTINGS:
                vid = fc.sheet_video(C, hw, clamp, rescale)
                sheet = raw.log_sheet(vid, clamp, rescale)                                  # asserts that every byte is defined
                assert sheet.shape == (2, 2 * hw[0], hw[1], 3) and not _same(vid[0], vid[1]) and np.isnan(vid).any() == bool(clamp and rescale)
                assert (vid > 1).any() == bool(clamp)
                assert len(set(sheet.reshape(-1).tolist())) > min(100, vid.size // 4)
    assert [2 * 2 * h * (w // 4 if w % 4 == 0 else w) for h, w in fc.SHEET_SIZES] == [12, 140, 1080]     # lanes: the last above 256
    assert raw.clamp_unit(F([np.nan]), nan_to_low=False).tolist() != [-1.0]
    for pixels in fc.POST_PIXELS:
        f = fc.u8_pixels(pixels)
        assert len(f) == pixels and (pixels < 3 or f[:3].tolist() == [list(t) for t in fc.TRIPLES])
    ties = fc.equidistant_colours()
    d = np.sort(raw.palette_distances(ties), axis=0)
    assert ties.shape[1] >= 5 and (d[0] == d[1]).all()
    first, last = raw.semantic_nearest(ties)[1], raw.semantic_nearest(ties, first=False)[1]
    assert (first < last).all()                                                            # the last minimum would be another label
    for hw in (255, 257):
        img = fc.semantic_image(hw)
        vis, labels = raw.semantic_nearest(img)
        assert labels[1:20].tolist() == list(range(19)) and _same(vis[:, 1:20], img[:, 1:20]) and not np.array_equal(labels, raw.semantic_nearest(img, first=False)[1])
    assert fc.semantic_image(1).shape == (3, 1) and len(fc.ENTRY_POINTS) == 13
