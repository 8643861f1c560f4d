"""The 18 entry points of csrc/cloud.hip, neighbours.hip, depth.hip, consistency.hip and metrics.hip called directly through hip.lib(),
with raw pointers into sentinel-filled buffers (sentinel_buffers.Flat), on the cases of tests/scene_cases.py: both forms of the
four-pixel / one-pixel kernels with every pointer of the dispatch's predicate moved off alignment in turn, sizes that do not fill their
last workgroup, sums that start from a non-zero pattern, slots that must stay unwritten, and table entries spoiled by one element
either way (a kernel that used them unchecked would still address inside the test's own allocation: a missing check shows as a wrong
result or a changed sentinel, never as a fault).  The definitions are tests/scene_raw_reference.py over the five *_reference modules;
every comparison is torch.equal on the bits, no tolerance and no element left out, and after every call every result is read with
read() (nothing outside the view was written) and every input checked with unchanged().  Float operands a kernel only reads lie in
NaN, everything else in the byte 0xA5; an operand whose rule ignores both lies in a value the rule counts (Flat's fill), so that a
read of padding changes the result.  tests/test_scene_cpu.py asserts that each case reaches the clause it names."""
import ctypes

import numpy as np
import pytest
import torch

import cloud_reference as cr
import scene_cases as sc
import scene_raw_reference as raw
from sentinel_buffers import Flat

pytestmark = pytest.mark.gpu
I64, I32, F32, U8 = torch.int64, torch.int32, torch.float32, torch.uint8
EINVAL = -1
NAN64 = 0x7FF8000000000000                                      # a float64 NaN as the int64 that carries it
QUARTER64 = int(np.float64(0.25).view(np.int64))                # a witness row of sixteen 0.25 projects every point to pixel (0, 0): evidence
SENT = {np.dtype(t): np.frombuffer(bytes([0xA5] * 8), dtype=t)[0] for t in (np.int64, np.int32, np.uint8)}
SKY = sc.SKY
MIN_DEPTH, MAX_DEPTH = 0.0, 100.0


def _t(a):
    """numpy -> a flat tensor of the same bits (unsigned words and doubles as the signed integer of their width)."""
    a = np.ascontiguousarray(a)
    a = a.view({np.dtype(np.uint64): np.int64, np.dtype(np.float64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype))
    return torch.from_numpy(a.copy()).reshape(-1)


def _bits(x):
    return x.view(I32) if x.dtype == F32 else x


def _same(got, want, what):
    got, want = _bits(got.reshape(-1)), _bits(_t(want))
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    differ = int((got != want).sum())
    print(f"{what}: {differ} of {want.numel()} values differ")
    assert torch.equal(got, want), (what, differ)


def _put(a, dev, **kw):
    """An operand: the array's bits inside its sentinels (doubles travel as int64 and lie in NaN)."""
    t = _t(a)
    if np.asarray(a).dtype == np.float64 and "fill" not in kw:
        kw["fill"] = NAN64
    return Flat(t.numel(), t.dtype, **kw).put(t, dev)


def _blank(n, dtype, dev, off=1):
    return Flat(n, dtype, off=off).blank(dev)


def _ptr(buf):
    return None if buf is None else buf.ptr


def _lib():
    from mudg_amd import hip
    return hip.lib()


def _ok(rc, what):
    msg = _lib().mudg_last_error()
    assert rc == 0, (what, rc, msg.decode() if msg else "")
    torch.cuda.synchronize()


def _unchanged(what, **bufs):
    for k, b in bufs.items():
        if b is not None:
            b.unchanged(f"{what}: {k}")


def _kept(want, written):
    """The definition's result where a slot is written, the sentinel where it must stay unwritten."""
    want = np.ascontiguousarray(want)
    want = want.view({np.dtype(np.float64): np.int64, np.dtype(np.uint64): np.int64}.get(want.dtype, want.dtype)).copy()
    want[~written] = SENT[want.dtype]
    return want


# ================================================================================================ the four-pixel / one-pixel kernels
# Each runner makes one call at the element offsets `offs` (by operand name; 0: the base is 256 elements into a fresh allocation, so
# aligned) and returns (the results' bits by name, the form the entry point chooses for these addresses).
def _form(W, *aligned):
    return 4 if W % 4 == 0 and all(b is None or b.ptr % a == 0 for b, a in aligned) else 1


def _run_align_sums(c, dev, offs):
    what = f"depth_align_sums {c['name']} {offs}"
    frames = _put(c["frames"], dev, off=offs.get("frames", 0))
    lidar = _put(c["lidar"], dev, off=offs.get("lidar", 0), fill=1.0)                      # padding that the rule would count
    start = sc.start_sums((2, 5), 11)
    sums = _put(start, dev, off=1)
    _ok(_lib().mudg_depth_align_sums(frames.ptr, lidar.ptr, 2, c["H"], c["W"], sums.ptr, None), what)
    got = sums.read(f"{what}: sums")
    _unchanged(what, frames=frames, lidar=lidar)
    _same(got, raw.align_sums(c["frames"], c["lidar"], start), f"{what}: sums")
    return {"sums": got}, _form(c["W"], (frames, 4), (lidar, 16))


def _run_finish(c, dev, offs, labels=True, vis=True):
    what = f"depth_finish {c['name']} {offs} [labels {labels}, vis {vis}]"
    n = 2 * c["H"] * c["W"]
    frames, coef = _put(c["frames"], dev, off=offs.get("frames", 0)), _put(c["coef"], dev, off=1)
    lab = _put(c["labels"], dev, off=offs.get("labels", 0), fill=SKY) if labels else None
    depth = _blank(n, F32, dev, off=offs.get("depth", 0))
    picture = _blank(3 * n, U8, dev, off=offs.get("vis", 0)) if vis else None
    _ok(_lib().mudg_depth_finish(frames.ptr, coef.ptr, _ptr(lab), SKY, 2, c["H"], c["W"], depth.ptr, _ptr(picture), None), what)
    got = {"depth": depth.read(f"{what}: depth")}
    if vis:
        got["vis"] = picture.read(f"{what}: vis")
    _unchanged(what, frames=frames, coef=coef, labels=lab)
    want_d, want_v = raw.finish(c["frames"], c["coef"], c["labels"] if labels else None, SKY)
    _same(got["depth"], want_d, f"{what}: depth")
    if vis:
        _same(got["vis"], want_v, f"{what}: vis")
    return got, _form(c["W"], (frames, 4), (depth, 16), (picture, 4), (lab, 16))


def _run_unproject(c, dev, offs, labels=True):
    what = f"depth_unproject {c['name']} {offs} [labels {labels}]"
    n = 2 * c["H"] * c["W"]
    depth = _put(c["depth"], dev, off=offs.get("depth", 0), fill=5.0)
    rgb, table = _put(c["frames"], dev, off=offs.get("rgb", 0)), _put(c["table"], dev, off=1)
    lab = _put(c["labels"], dev, off=offs.get("labels", 0), fill=SKY) if labels else None
    points, valid = _blank(4 * n, I32, dev, off=0), _blank(n, U8, dev, off=offs.get("valid", 0))
    _ok(_lib().mudg_depth_unproject(depth.ptr, rgb.ptr, _ptr(lab), SKY, table.ptr, 2, c["H"], c["W"], MIN_DEPTH, MAX_DEPTH, points.ptr, valid.ptr, None), what)
    got = {"points": points.read(f"{what}: points"), "valid": valid.read(f"{what}: valid")}
    _unchanged(what, depth=depth, rgb=rgb, table=table, labels=lab)
    want_p, want_v = raw.unproject(c["depth"], c["frames"], c["table"], c["labels"] if labels else None, SKY, MIN_DEPTH, MAX_DEPTH)
    _same(got["points"], want_p, f"{what}: points")
    _same(got["valid"], want_v, f"{what}: valid")
    return got, _form(c["W"], (depth, 16), (rgb, 4), (lab, 16), (valid, 4))


def _run_flags(c, dev, offs, labels=True):
    what = f"view_flags {c['name']} {offs} [labels {labels}]"
    n = 2 * c["H"] * c["W"]
    depth = _put(c["depth"], dev, off=offs.get("depth", 0), fill=5.0)
    lab = _put(c["labels"], dev, off=offs.get("labels", 0), fill=SKY) if labels else None
    flags = _blank(n, U8, dev, off=offs.get("flags", 0))
    _ok(_lib().mudg_view_flags(depth.ptr, _ptr(lab), SKY, sc.DYNAMIC_MASK, 2, c["H"], c["W"], MIN_DEPTH, MAX_DEPTH, flags.ptr, None), what)
    got = {"flags": flags.read(f"{what}: flags")}
    _unchanged(what, depth=depth, labels=lab)
    _same(got["flags"], raw.view_flags(c["depth"], c["labels"] if labels else None, SKY, sc.DYNAMIC_MASK, MIN_DEPTH, MAX_DEPTH), f"{what}: flags")
    return got, _form(c["W"], (depth, 16), (lab, 16), (flags, 4))


def _run_sse(c, dev, offs):
    what = f"metric_sse {c['name']} {offs}"
    a, b = _put(c["frames"], dev, off=offs.get("a", 0)), _put(c["other"], dev, off=offs.get("b", 0))
    start = sc.start_sums((2,), 12)
    sums = _put(start, dev, off=1)
    _ok(_lib().mudg_metric_sse(a.ptr, b.ptr, 2, c["H"], c["W"], sums.ptr, None), what)
    got = sums.read(f"{what}: sums")
    _unchanged(what, a=a, b=b)
    _same(got, raw.metric_sse(c["frames"], c["other"], start), f"{what}: sums")
    return {"sums": got}, _form(c["W"], (a, 4), (b, 4))


def _run_metric_depth(c, dev, offs):
    what = f"metric_depth {c['name']} {offs}"
    depth = _put(c["depth"], dev, off=offs.get("depth", 0), fill=2.0)
    lidar = _put(c["lidar"], dev, off=offs.get("lidar", 0), fill=1.0)
    start = sc.start_sums((2, 8), 13)
    sums = _put(start, dev, off=1)
    _ok(_lib().mudg_metric_depth(depth.ptr, lidar.ptr, 2, c["H"], c["W"], 0.1, 80.0, sums.ptr, None), what)
    got = sums.read(f"{what}: sums")
    _unchanged(what, depth=depth, lidar=lidar)
    _same(got, raw.metric_depth(c["depth"], c["lidar"], start, 0.1, 80.0), f"{what}: sums")
    return {"sums": got}, _form(c["W"], (depth, 16), (lidar, 16))


# (runner, the pointers of its wide predicate, its optional operands)
PIXEL_KERNELS = {
    "depth_align_sums": (_run_align_sums, ("frames", "lidar"), ()),
    "depth_finish": (_run_finish, ("frames", "depth", "vis", "labels"), ("labels", "vis")),
    "depth_unproject": (_run_unproject, ("depth", "rgb", "labels", "valid"), ("labels",)),
    "view_flags": (_run_flags, ("depth", "labels", "flags"), ("labels",)),
    "metric_sse": (_run_sse, ("a", "b"), ()),
    "metric_depth": (_run_metric_depth, ("depth", "lidar"), ()),
}


@pytest.mark.parametrize("kernel", list(PIXEL_KERNELS))
@pytest.mark.parametrize("hw", sc.PIXEL_SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_pixel_kernels_equal_the_definition_in_both_forms(cuda, hw, kernel):
    """Aligned bases: W % 4 alone chooses the form.  With and without each optional operand."""
    c = sc.pixel_case(hw)
    run, _, optional = PIXEL_KERNELS[kernel]
    print(f"{kernel} at {c['name']}: {c['clause']}")
    choices = [dict(zip(optional, v)) for v in np.ndindex(*(2,) * len(optional))]
    for choice in choices:
        _, form = run(c, cuda, {}, **{k: bool(v) for k, v in choice.items()})
        assert form == (4 if hw[1] % 4 == 0 else 1), (kernel, hw, choice, form)


@pytest.mark.parametrize("kernel", list(PIXEL_KERNELS))
def test_each_pointer_of_the_wide_predicate_off_alignment_gives_the_same_bits(cuda, kernel):
    """W % 4 == 0 and one base after another one element off: the entry point must choose the one-pixel form, whose bits are the
    aligned call's and the definition's.  A term missing from the conjunction runs the wide form on an address it was not written for."""
    c = sc.pixel_case(sc.ALIGNED_SIZE)
    run, pointers, _ = PIXEL_KERNELS[kernel]
    aligned, form = run(c, cuda, {})
    assert form == 4
    for name in pointers:
        moved, form = run(c, cuda, {name: 1})
        assert form == 1, (kernel, name)
        for k, v in aligned.items():
            assert torch.equal(_bits(v), _bits(moved[k])), (kernel, name, k)
    everything, form = run(c, cuda, {name: 1 for name in pointers})
    assert form == 1 and all(torch.equal(_bits(v), _bits(everything[k])) for k, v in aligned.items())


# ================================================================================================ the other depth entry points
@pytest.mark.parametrize("frames", sc.SOLVE_FRAMES)
def test_depth_align_solve_equals_the_definition(cuda, frames):
    c = sc.solve_case(frames)
    print(f"{c['name']}: {c['clause']}; rows {sorted(set(c['kinds']))}")
    sums = _put(c["sums"], cuda, off=1)
    coef, fitted = _blank(2 * frames, I64, cuda), _blank(frames, U8, cuda)
    _ok(_lib().mudg_depth_align_solve(sums.ptr, frames, coef.ptr, fitted.ptr, None), c["name"])
    want_coef, want_fitted = raw.align_solve(c["sums"])
    _same(coef.read("coef"), want_coef, f"{c['name']}: coef")
    _same(fitted.read("fitted"), want_fitted, f"{c['name']}: fitted")
    sums.unchanged("sums")


@pytest.mark.parametrize("value_range", sc.COLORMAP_RANGES, ids=lambda r: f"{r[0]:g}..{r[1]:g}")
@pytest.mark.parametrize("n", sc.COLORMAP_SIZES)
def test_colormap_spectral_equals_the_definition(cuda, n, value_range):
    c = sc.colormap_case(n, value_range)
    print(f"{c['name']}: {c['clause']}")
    for reversed_ in (0, 1):
        want_b, want_c = raw.colormap(c["values"], c["val_min"], c["val_max"], bool(reversed_))
        for outs in (("bytes",), ("colours",), ("bytes", "colours")):
            what = f"{c['name']} [reversed {reversed_}, {'+'.join(outs)}]"
            values = _put(c["values"], cuda, off=1, nan=True)
            b = _blank(3 * n, U8, cuda) if "bytes" in outs else None
            col = _blank(3 * n, F32, cuda) if "colours" in outs else None
            _ok(_lib().mudg_colormap_spectral(values.ptr, n, c["val_min"], c["val_max"], reversed_, _ptr(b), _ptr(col), None), what)
            if b is not None:
                _same(b.read(f"{what}: bytes"), want_b, f"{what}: bytes")
            if col is not None:
                _same(col.read(f"{what}: colours"), want_c, f"{what}: colours")
            values.unchanged(f"{what}: values")


# ================================================================================================ metrics.hip
@pytest.mark.parametrize("hw", sc.SSIM_SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_metric_ssim_equals_the_definition(cuda, hw):
    c = sc.ssim_case(hw)
    print(f"{c['name']}: {c['clause']}")
    a, b = _put(c["a"], cuda, off=1), _put(c["b"], cuda, off=3)
    start = sc.start_sums((2,), 14)
    start[1] = np.uint64(2 ** 64 - 12345)                                                  # a negative start: the sum is signed
    sums = _put(start, cuda, off=1)
    _ok(_lib().mudg_metric_ssim(a.ptr, b.ptr, 2, c["H"], c["W"], sums.ptr, None), c["name"])
    _same(sums.read("sums"), raw.metric_ssim(c["a"], c["b"], start), f"ssim {c['name']}: sums")
    _unchanged(c["name"], a=a, b=b)


@pytest.mark.parametrize("classes", sc.CONFUSION_CLASSES)
@pytest.mark.parametrize("hw", sc.CONFUSION_SIZES, ids=lambda hw: f"{hw[0] * hw[1]} pixels")
def test_metric_confusion_equals_the_definition(cuda, hw, classes):
    c = sc.confusion_case(hw, classes)
    print(f"{c['name']}: {c['clause']}")
    pred, gt = _put(c["pred"], cuda, off=1, fill=0), _put(c["gt"], cuda, off=1, fill=0)     # padding of a valid class: it would be counted
    start, start_bad = sc.start_sums((2, classes, classes), 15), sc.start_sums((2,), 16)
    m, bad = _put(start, cuda, off=1), _put(start_bad, cuda, off=1)
    _ok(_lib().mudg_metric_confusion(pred.ptr, gt.ptr, 2, c["H"], c["W"], classes, m.ptr, bad.ptr, None), c["name"])
    want_m, want_bad = raw.metric_confusion(c["pred"], c["gt"], classes, start, start_bad)
    _same(m.read("confusion"), want_m, f"confusion {c['name']}: cells")
    _same(bad.read("bad"), want_bad, f"confusion {c['name']}: bad")
    _unchanged(c["name"], pred=pred, gt=gt)


# ================================================================================================ neighbours.hip
@pytest.mark.parametrize("K", (0, 8))
@pytest.mark.parametrize("n", sc.CLOUD_METRIC_SIZES)
def test_metric_cloud_equals_the_definition(cuda, n, K):
    c = sc.cloud_metric_case(n)
    print(f"{c['name']}, {K} thresholds: {c['clause']}")
    t2 = sc.CLOUD_T2[:K]
    d2 = _put(c["d2"], cuda, off=1, fill=0)                                                # padding of 0.0: found, inside every threshold
    start = sc.start_sums((2 + K,), 17)
    sums = _put(start, cuda, off=1)                                                        # K = 0: two words, the ten of K = 8 must stay untouched
    table = (ctypes.c_double * K)(*t2) if K else None
    _ok(_lib().mudg_metric_cloud(d2.ptr, n, table, K, sc.CLOUD_R2, sums.ptr, None), c["name"])
    _same(sums.read("sums"), raw.metric_cloud(c["d2"], t2, sc.CLOUD_R2, start), f"metric_cloud {c['name']}, K = {K}: sums")
    d2.unchanged("d2")


def _search_buffers(c, dev, order):
    zeros = np.zeros((len(c["ref_sorted"]), 3), np.uint8)
    return dict(ref=_put(cr.pack(c["ref_sorted"], zeros), dev), keys=_put(c["keys"], dev, off=1), order=_put(order, dev, off=1),
                queries=_put(cr.pack(c["queries"], np.zeros((c["nq"], 3), np.uint8)), dev))


SEARCHES = [(nq, False) for nq in sc.SEARCH_QUERIES] + [(257, True)]


@pytest.mark.parametrize("visit", sc.VISITS)
@pytest.mark.parametrize("nq,one_point", SEARCHES, ids=[f"{'1 point' if one else '300 points'}, {nq} queries" for nq, one in SEARCHES])
def test_cloud_nearest_equals_the_definition_and_leaves_unvisited_slots(cuda, nq, one_point, visit):
    c = sc.search_case(nq, one_point)
    print(f"{c['name']}, visit {visit}: {c['clause']}")
    n = len(c["ref_sorted"])
    for order in (c["order"], c["foreign"]):
        what = f"nearest {c['name']} [visit {visit}, order {'as sorted' if order is c['order'] else 'foreign values'}]"
        bufs = _search_buffers(c, cuda, order)
        table = None if c["visit"][visit] is None else _put(c["visit"][visit], cuda, off=1)
        d2, index = _blank(nq, I64, cuda), _blank(nq, I64, cuda)
        _ok(_lib().mudg_cloud_nearest(bufs["ref"].ptr, bufs["keys"].ptr, bufs["order"].ptr, n, bufs["queries"].ptr, _ptr(table), nq, c["cell"],
                                      sc.SEARCH_R ** 2, d2.ptr, index.ptr, None), what)
        want_d2, want_index, owned = raw.cloud_nearest(c["ref_sorted"], order, c["queries"], c["visit"][visit], sc.SEARCH_R)
        print(f"{what}: {int((~owned).sum())} slots stay unwritten")
        _same(d2.read(f"{what}: d2"), _kept(want_d2, owned), f"{what}: d2")
        _same(index.read(f"{what}: index"), _kept(want_index, owned), f"{what}: index")
        _unchanged(what, visit=table, **bufs)


@pytest.mark.parametrize("visit", sc.VISITS)
@pytest.mark.parametrize("nq,one_point", SEARCHES, ids=[f"{'1 point' if one else '300 points'}, {nq} queries" for nq, one in SEARCHES])
def test_cloud_count_equals_the_definition_and_leaves_unvisited_slots(cuda, nq, one_point, visit):
    c = sc.search_case(nq, one_point)
    print(f"{c['name']}, visit {visit}: {c['clause']}")
    n = len(c["ref_sorted"])
    for cap in (1, 3, sc.BIG_CAP):
        what = f"count {c['name']} [visit {visit}, cap {cap}]"
        bufs = _search_buffers(c, cuda, c["foreign"])                                      # the count never reads the order
        table = None if c["visit"][visit] is None else _put(c["visit"][visit], cuda, off=1)
        counts = _blank(nq, I32, cuda)
        _ok(_lib().mudg_cloud_count(bufs["ref"].ptr, bufs["keys"].ptr, bufs["order"].ptr, n, bufs["queries"].ptr, _ptr(table), nq, c["cell"],
                                    sc.SEARCH_R ** 2, cap, counts.ptr, None), what)
        want, owned = raw.cloud_count(c["ref_sorted"], c["queries"], c["visit"][visit], sc.SEARCH_R, cap)
        _same(counts.read(f"{what}: counts"), _kept(want, owned), f"{what}: counts")
        _unchanged(what, visit=table, **bufs)


# ================================================================================================ cloud.hip
@pytest.mark.parametrize("variant", sc.SWEEP_VARIANTS)
def test_cloud_sweep_equals_the_definition_on_spoiled_tables(cuda, variant):
    c = sc.sweep_case(variant)
    print(f"{variant}: {c['clause']}")
    cam_table, obj_table = sc.sweep_tables(c)
    ncam, nobj, total = cam_table.shape[1], obj_table.shape[1], c["total"]
    ins = dict(rays_o=_put(c["rays_o"], cuda, off=1, nan=True), rays_d=_put(c["rays_d"], cuda, off=2, nan=True), ranges=_put(c["ranges"], cuda, off=1, nan=True),
               offsets=_put(c["offsets"], cuda, off=1), l2w=_put(c["l2w"], cuda, off=1), cams=_put(cam_table, cuda, off=1) if ncam else None,
               objs=_put(obj_table, cuda, off=1) if nobj else None, images=_put(c["images"], cuda, off=1) if ncam else None)
    points, labels = _blank(4 * total, I32, cuda, off=0), _blank(total, I32, cuda)
    _ok(_lib().mudg_cloud_sweep(ins["rays_o"].ptr, ins["rays_d"].ptr, ins["ranges"].ptr, ins["offsets"].ptr, len(c["offsets"]) - 1, c["max_rays"], total,
                                ins["l2w"].ptr, _ptr(ins["cams"]), ncam, _ptr(ins["objs"]), nobj, _ptr(ins["images"]), c["image_bytes"] if ncam else 0,
                                points.ptr, labels.ptr, None), variant)
    want_p, want_l, written, dropped, refused = raw.cloud_sweep(c["rays_o"], c["rays_d"], c["ranges"], c["offsets"], total, c["max_rays"], c["l2w"], c["cams"],
                                                                c["objs"], c["images"], c["image_bytes"])
    print(f"{variant}: {dropped} returns dropped by the offset check, {refused} colours refused by the address check, {int((~written).sum())} slots unwritten")
    _same(points.read("points"), _kept(want_p, written), f"sweep {variant}: points")
    _same(labels.read("labels"), _kept(want_l, written), f"sweep {variant}: labels")
    _unchanged(variant, **ins)


@pytest.mark.parametrize("n", list(sc.VOXEL_RUNS))
def test_cloud_voxel_keys_equal_the_definition(cuda, n):
    for what, xyz in ((f"{n} points", sc.voxel_case(n)["xyz"]),) + ((("65 points, six indices outside +-2^20", sc.voxel_wrap_points()),) if n == 65 else ()):
        points = _put(cr.pack(xyz, np.zeros((len(xyz), 3), np.uint8)), cuda)
        keys = _blank(len(xyz), I64, cuda)
        _ok(_lib().mudg_cloud_voxel_keys(points.ptr, len(xyz), sc.VOXEL, keys.ptr, None), what)
        _same(keys.read("keys"), raw.voxel_keys(xyz, sc.VOXEL), f"voxel keys, {what}")
        points.unchanged("points")


@pytest.mark.parametrize("spoil", sc.VOXEL_SPOILS)
@pytest.mark.parametrize("n", list(sc.VOXEL_RUNS))
def test_cloud_voxel_reduce_adds_to_its_sums_and_drops_spoiled_entries(cuda, n, spoil):
    c = sc.voxel_case(n, spoil)
    print(f"{c['name']}: {c['clause']}; runs {c['runs']}, spoiled entries {c['spoiled']}")
    for start in (np.zeros((c["voxels"], 8), np.uint64), sc.start_sums((c["voxels"], 8), 18)):
        what = f"voxel reduce {c['name']} [sums {'zero' if not start.any() else 'non-zero'} at the start]"
        points, order, segments = _put(c["packed"], cuda), _put(c["order"], cuda, off=1), _put(c["segments"], cuda, off=1)
        sums = _put(start, cuda, off=0)
        _ok(_lib().mudg_cloud_voxel_reduce(points.ptr, order.ptr, segments.ptr, n, sc.VOXEL, sums.ptr, c["voxels"], None), what)
        want, dropped = raw.voxel_reduce(c["packed"], c["order"], c["segments"], sc.VOXEL, start)
        print(f"{what}: {dropped} entries dropped")
        _same(sums.read("sums"), want, what)
        _unchanged(what, points=points, order=order, segments=segments)


@pytest.mark.parametrize("n", list(sc.VOXEL_RUNS))
def test_cloud_voxel_finish_equals_the_definition(cuda, n):
    c = sc.voxel_case(n)
    made, _ = raw.voxel_reduce(c["packed"], c["order"], c["segments"], sc.VOXEL, np.zeros((c["voxels"], 8), np.uint64))
    if n > 1:
        made[-1, 1:] = sc.start_sums((7,), 19)                                             # count 0 and the other words set: a zero point
    sums, out = _put(made, cuda, off=1), _blank(4 * c["voxels"], I32, cuda, off=0)
    _ok(_lib().mudg_cloud_voxel_finish(sums.ptr, c["voxels"], sc.VOXEL, out.ptr, None), c["name"])
    _same(out.read("out"), raw.voxel_finish(made, sc.VOXEL), f"voxel finish {c['name']}")
    sums.unchanged("sums")


# ================================================================================================ consistency.hip
def _consistency(c, dev):
    """A NaN row gives no evidence, so the witness table lies in rows of 0.25 instead, the flags in "usable" and the depths in 5 m: a
    witness id that is used unchecked reads a row, a view and a time of padding that count, and changes the verdicts."""
    V, N, n = c["V"], c["N"], c["V"] * c["H"] * c["W"]
    ins = dict(depth=_put(c["depth"], dev, off=1, fill=5.0), flags=_put(c["flags"], dev, off=1, fill=1), src=_put(c["src"], dev, off=1),
               wit=_put(c["wit"], dev, off=1, fill=QUARTER64), times=_put(c["times"], dev, off=1), witnesses=_put(c["witnesses"], dev, off=1))
    start = sc.start_sums((V, 6), 20)
    outs = dict(agree=_blank(n, U8, dev), violate=_blank(n, U8, dev, off=3), keep=_blank(n, U8, dev, off=2), stats=_put(start, dev, off=1))
    _ok(_lib().mudg_view_consistency(ins["depth"].ptr, ins["flags"].ptr, ins["src"].ptr, ins["wit"].ptr, ins["times"].ptr, ins["witnesses"].ptr, V, N, c["H"], c["W"],
                                     c["r"], c["min_agree"], c["max_violate"], c["rel_tol"], c["abs_tol"], outs["agree"].ptr, outs["violate"].ptr, outs["keep"].ptr,
                                     outs["stats"].ptr, None), c["name"])
    want = raw.view_consistency(c["depth"], c["flags"], c["src"], c["wit"], c["times"], c["witnesses"], start, **{k: c[k] for k in sc.VIEW_PARAMS})
    for (k, buf), w in zip(outs.items(), want):
        _same(buf.read(f"{c['name']}: {k}"), w, f"consistency {c['name']}: {k}")
    _unchanged(c["name"], **ins)
    return want


@pytest.mark.parametrize("ids", sc.VIEW_IDS)
@pytest.mark.parametrize("N", sc.VIEW_WITNESSES)
@pytest.mark.parametrize("hw", sc.VIEW_SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_view_consistency_equals_the_definition_with_spoiled_witness_ids(cuda, hw, N, ids):
    c = sc.view_case(hw, N, ids)
    print(f"{c['name']}: {c['clause']}")
    want = _consistency(c, cuda)
    print(f"{c['name']}: agree up to {int(want[0].max())}, violate up to {int(want[1].max())}, kept {int(want[2].sum())} of {want[2].size}")


def test_view_consistency_puts_u_equal_to_w_outside(cuda):
    c = sc.view_exact_case()
    print(f"{c['name']}: {c['clause']}")
    _consistency(c, cuda)


# ================================================================================================ refusals
# A small valid call of each entry point, in the order of its arguments: a buffer (name, dtype, elements) or a scalar (name, value).
_PIX = 2 * 16 * 16
_SHAPE_ARGS = (("frames", 2), ("H", 16), ("W", 16))
VALID = {
    "depth_align_sums": (("frames_u8", U8, 3 * _PIX), ("lidar", F32, _PIX), *_SHAPE_ARGS, ("sums", I64, 10)),
    "depth_align_solve": (("sums", I64, 10), ("frames", 2), ("coef", I64, 4), ("fitted", U8, 2)),
    "depth_finish": (("frames_u8", U8, 3 * _PIX), ("coef", I64, 4), ("labels", I64, _PIX), ("sky_label", SKY), *_SHAPE_ARGS, ("depth", F32, _PIX), ("vis", U8, 3 * _PIX)),
    "colormap_spectral": (("values", F32, 64), ("n", 64), ("val_min", 0.0), ("val_max", 1.0), ("reversed", 0), ("bytes", U8, 192), ("colours", F32, 192)),
    "depth_unproject": (("depth", F32, _PIX), ("rgb", U8, 3 * _PIX), ("labels", I64, _PIX), ("sky_label", SKY), ("table", I64, 32), *_SHAPE_ARGS, ("min_depth", 0.0),
                        ("max_depth", 100.0), ("points", I32, 4 * _PIX), ("valid", U8, _PIX)),
    "view_flags": (("depth", F32, _PIX), ("labels", I64, _PIX), ("sky_label", SKY), ("dynamic_mask", sc.DYNAMIC_MASK), *_SHAPE_ARGS, ("min_depth", 0.0), ("max_depth", 100.0),
                   ("flags", U8, _PIX)),
    "view_consistency": (("depth", F32, _PIX), ("flags", U8, _PIX), ("src", I64, 32), ("wit", I64, 32), ("times", I32, 2), ("witnesses", I32, 8), ("frames", 2), ("N", 4),
                         ("H", 16), ("W", 16), ("r", 1), ("min_agree", 1), ("max_violate", 0), ("rel_tol", 0.02), ("abs_tol", 0.2), ("agree", U8, _PIX),
                         ("violate", U8, _PIX), ("keep", U8, _PIX), ("stats", I64, 12)),
    "metric_sse": (("a", U8, 3 * _PIX), ("b", U8, 3 * _PIX), *_SHAPE_ARGS, ("sums", I64, 2)),
    "metric_ssim": (("a", U8, 3 * _PIX), ("b", U8, 3 * _PIX), *_SHAPE_ARGS, ("sums", I64, 2)),
    "metric_depth": (("depth", F32, _PIX), ("lidar", F32, _PIX), *_SHAPE_ARGS, ("min_depth", 0.1), ("max_depth", 80.0), ("sums", I64, 16)),
    "metric_confusion": (("pred", I64, _PIX), ("gt", I64, _PIX), *_SHAPE_ARGS, ("classes", 19), ("confusion", I64, 2 * 361), ("bad", I64, 2)),
    "cloud_nearest": (("ref", I32, 32), ("keys", I64, 8), ("order", I64, 8), ("n", 8), ("queries", I32, 32), ("visit", I64, 8), ("nq", 8), ("cell", float(raw.nr.cell_edge(0.5))),
                      ("r2", 0.25), ("d2", I64, 8), ("index", I64, 8)),
    "cloud_count": (("ref", I32, 32), ("keys", I64, 8), ("order", I64, 8), ("n", 8), ("queries", I32, 32), ("visit", I64, 8), ("nq", 8), ("cell", float(raw.nr.cell_edge(0.5))),
                    ("r2", 0.25), ("cap", 4), ("counts", I32, 8)),
    "metric_cloud": (("d2", I64, 64), ("n", 64), ("t2", (0.01, 0.25)), ("K", 2), ("r2", 0.25), ("sums", I64, 4)),
    "cloud_sweep": (("rays_o", F32, 24), ("rays_d", F32, 24), ("ranges", F32, 8), ("offsets", I64, 3), ("frames", 2), ("max_rays", 8), ("total", 8), ("l2w", I64, 24),
                    ("cams", I64, 48), ("ncam", 1), ("objs", I64, 32), ("nobj", 1), ("images", U8, 64), ("image_bytes", 64), ("points", I32, 32), ("labels", I32, 8)),
    "cloud_voxel_keys": (("points", I32, 32), ("n", 8), ("voxel", 0.5), ("keys", I64, 8)),
    "cloud_voxel_reduce": (("points", I32, 32), ("order", I64, 8), ("segments", I64, 8), ("n", 8), ("voxel", 0.5), ("sums", I64, 24), ("voxels", 3)),
    "cloud_voxel_finish": (("sums", I64, 24), ("voxels", 3), ("voxel", 0.5), ("out", I32, 12)),
}


def _call(entry, dev, changes):
    """The valid call of VALID[entry] with `changes` applied: a buffer's name -> None (a null pointer) or bytes to move it by, a scalar's
    name -> its value.  Every buffer holds nothing but its sentinel (tables of sentinels own no element: every lane returns early)."""
    spec = VALID[entry]
    bufs = {a[0]: Flat(a[2], a[1], off=0).blank(dev) for a in spec if len(a) == 3}
    assert set(changes) <= {a[0] for a in spec}, (entry, changes)
    args = []
    for a in spec:
        if len(a) == 3:
            move = changes.get(a[0], 0)
            args.append(None if move is None else bufs[a[0]].ptr + move)
        else:
            v = changes.get(a[0], a[1])
            args.append((ctypes.c_double * len(v))(*v) if isinstance(v, tuple) else v)
    rc = getattr(_lib(), "mudg_" + entry)(*args, None)
    msg = _lib().mudg_last_error()
    torch.cuda.synchronize()
    return rc, (msg.decode() if msg else ""), bufs


@pytest.mark.parametrize("entry", sc.ENTRY_POINTS)
def test_bad_arguments_are_refused_before_any_launch(cuda, entry):
    """The valid call first (it returns 0 and writes nothing outside its views), then every refusal of the entry point: the error code,
    the clause's message, and every buffer still holding its sentinel."""
    rc, msg, bufs = _call(entry, cuda, {})
    assert rc == 0, (entry, rc, msg)
    for k, b in bufs.items():
        b.read(f"{entry}: {k}")
    mine = [r for r in sc.REFUSALS if r[0] == entry]
    assert mine
    for _, wrong, changes, piece in mine:
        rc, msg, bufs = _call(entry, cuda, changes)
        print(f"{entry}, {wrong}: {rc} {msg!r}")
        assert rc == EINVAL and piece in msg and f"mudg_{entry}" in msg, (entry, wrong, rc, msg)
        for k, b in bufs.items():
            b.unchanged(f"{entry}, {wrong}: {k}")
