"""The 13 entry points of csrc/frames.hip, normals.hip, lidar_depth.hip and post.hip (and mudg_depth_complete_scratch) called directly
through hip.lib(), with raw pointers into sentinel-filled buffers (sentinel_buffers.Flat), on the cases of tests/frame_path_cases.py:
every term of every four-pixel / one-pixel predicate falsified alone, row segments and workgroups that are not full, tables spoiled by
one sample either way, streams placed inside a larger tensor, counts and keys that start from what the buffer held, a scratch of
exactly the stated bytes with stale contents.  A kernel that used a spoiled value unchecked would still address inside the test's own
allocation (see frame_path_cases.py): a missing check shows as a wrong result or a changed sentinel, never as a fault.  The
definitions are tests/frame_path_raw_reference.py over frames_reference, normals_reference, lidar_depth_reference and
splat_reference; every comparison is torch.equal on the bits, no tolerance and no element left out, and after every call every result
is read with read() (nothing outside the view was written) and every input checked with unchanged().  fp32 operands a kernel only
reads lie in NaN, everything else in the byte 0xA5; an operand whose rule ignores both lies in a value the rule counts (Flat's fill).
tests/test_frame_path_cpu.py asserts that each case reaches the clause it names.  These entry points touch no MFMA operand: they run
in the default build only."""
import ctypes

import numpy as np
import pytest
import torch

import frame_path_cases as fc
import frame_path_raw_reference as raw
import normals_reference as nm
import splat_reference as sr
from sentinel_buffers import Flat

pytestmark = pytest.mark.gpu
I64, I32, F32, U8 = torch.int64, torch.int32, torch.float32, torch.uint8
F = np.float32
EINVAL = -1
NAN64 = 0x7FF8000000000000
SENT32 = np.frombuffer(bytes([0xA5] * 4), dtype=np.int32)[0]
SKY = fc.SKY
T = fc.FRAMES


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


def _refused(rc, what, entry):
    msg = _lib().mudg_last_error()
    torch.cuda.synchronize()
    print(f"{what}: {rc} {msg!r}")
    assert rc == EINVAL and msg and entry in msg.decode(), (what, rc, msg)


def _unchanged(what, **bufs):
    for k, b in bufs.items():
        if b is not None:
            b.unchanged(f"{what}: {k}")


def _equal(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


# ================================================================================================ frames.hip: resize_u8, resize_f32
def _tables(c, kind, spoiled, dev):
    xt, yt = c["spoiled" if spoiled else "tables"][kind]
    return (xt, yt), _put(xt, dev, off=0), _put(yt, dev, off=4)                            # 16-byte entries, 16-byte aligned


def _run_resize_u8(c, row, dev, src_off=0, dst_off=0, spoiled=False):
    name, mode, C, palette = row
    what = f"resize_u8 {c['name']} {name} C={C} [src +{src_off}, dst +{dst_off}, spoiled {spoiled}]"
    source = c["ids"] if palette else c[f"u8_{C}"]
    (xt, yt), xb, yb = _tables(c, "nearest" if mode == raw.NEAREST else "u8", spoiled, dev)
    src, dst = _put(source, dev, off=src_off), _blank(T * c["H"] * c["W"] * C, U8, dev, off=dst_off)
    _ok(_lib().mudg_resize_u8(src.ptr, dst.ptr, T, c["H0"], c["W0"], C, c["H"], c["W"], mode, int(palette), xb.ptr, yb.ptr, None), what)
    got = dst.read(f"{what}: dst")
    _unchanged(what, src=src, xtab=xb, ytab=yb)
    _same(got, raw.resize_u8(source, xt, yt, mode, palette), what)
    return got


@pytest.mark.parametrize("row", fc.U8_MODES, ids=[f"{r[0]}-{r[2]}" for r in fc.U8_MODES])
@pytest.mark.parametrize("width", list(fc.RESIZE_SHAPES))
def test_resize_u8_equals_the_definition_at_every_alignment_and_on_spoiled_tables(cuda, width, row):
    c = fc.resize_case(width)
    print(f"{c['name']}: {c['clause']}")
    aligned = _run_resize_u8(c, row, cuda)
    assert torch.equal(aligned, _run_resize_u8(c, row, cuda, src_off=1))
    for off in (1, 2, 3):                                                                  # aligned4(dst) false: the bounded path, the same bytes
        assert torch.equal(aligned, _run_resize_u8(c, row, cuda, dst_off=off)), off
    # s0 = -1 and s1 = n_src in the first and last entry of each axis: at most one row and one pixel (36 bytes) outside the source
    _run_resize_u8(c, row, cuda, spoiled=True)
    _run_resize_u8(c, row, cuda, dst_off=1, spoiled=True)


def _run_resize_f32(c, dev, src_off=1, dst_off=0, spoiled=False):
    what = f"resize_f32 {c['name']} [src +{src_off}, dst +{dst_off}, spoiled {spoiled}]"
    (xt, yt), xb, yb = _tables(c, "f32", spoiled, dev)
    src, dst = _put(c["f32"], dev, off=src_off, nan=True), _blank(T * c["H"] * c["W"], F32, dev, off=dst_off)
    _ok(_lib().mudg_resize_f32(src.ptr, dst.ptr, T, c["H0"], c["W0"], c["H"], c["W"], xb.ptr, yb.ptr, None), what)
    got = dst.read(f"{what}: dst")
    _unchanged(what, src=src, xtab=xb, ytab=yb)
    _same(got, raw.resize_f32(c["f32"], xt, yt), what)
    return got


@pytest.mark.parametrize("width", list(fc.RESIZE_SHAPES))
def test_resize_f32_equals_the_definition_in_nan_padding_at_every_alignment_and_on_spoiled_tables(cuda, width):
    """The source lies in NaN, one float off: a second tap of s + 1 instead of min(s + 1, n - 1), or an unclamped table entry, is 0 * NaN."""
    c = fc.resize_case(width)
    print(f"{c['name']}: {c['clause']}")
    aligned = _run_resize_f32(c, cuda, src_off=0)
    for off in (0, 1, 2, 3):                                                               # dst 0, 4, 8, 12 bytes off
        assert torch.equal(_bits(aligned), _bits(_run_resize_f32(c, cuda, dst_off=off))), off
    _run_resize_f32(c, cuda, spoiled=True)
    _run_resize_f32(c, cuda, dst_off=1, spoiled=True)


# ================================================================================================ dense_stream, normal_stream
def _run_stream(c, kind, layout, dev, with_u8=False):
    """kind 0 .. 2: dense_stream; "normal": normal_stream.  Returns the planes gathered from the destination (and the bytes)."""
    lay = fc.stream_layout(layout, c["H"], c["W"])
    what = f"{'normal_stream' if kind == 'normal' else f'dense_stream kind {kind}'} {c['name']} [{layout}, u8 {with_u8}]"
    print(f"{what}: {lay['clause']}")
    floats = kind in (raw.DEPTH, "normal")
    source = {raw.COLOUR: c["u8_3"], raw.SEMANTIC: c["ids"], raw.DEPTH: c["metres"], "normal": c["normals"]}[kind]
    (xt, yt), xb, yb = _tables(c, "f32" if floats else "u8", False, dev)
    src = _put(source, dev, off=1, nan=floats)                                             # fp32 sources are 4-byte aligned only
    dst = _blank(lay["n"], F32, dev, off=lay["dst"])
    norm = None if floats else _put(c["norm"], dev, off=1, nan=True)
    u8 = _blank(T * c["H"] * c["W"] * 3, U8, dev, off=lay["u8"]) if with_u8 else None
    place = (lay["ss"], lay["cs"], lay["fs"], fc.SLAB, fc.FRAME0)
    if kind == "normal":
        rc = _lib().mudg_normal_stream(src.ptr, T, c["H0"], c["W0"], c["H"], c["W"], xb.ptr, yb.ptr, dst.ptr, *place, None)
        planes, want_u8 = raw.normal_stream(source, xt, yt), None
    else:
        rc = _lib().mudg_dense_stream(kind, src.ptr, T, c["H0"], c["W0"], c["H"], c["W"], xb.ptr, yb.ptr, _ptr(norm), dst.ptr, *place, _ptr(u8), None)
        planes, want_u8 = raw.dense_stream(kind, source, xt, yt, c["norm"])
    _ok(rc, what)
    got = dst.read(f"{what}: dst")
    _unchanged(what, src=src, xtab=xb, ytab=yb, norm=norm)
    offsets = raw.stream_offsets(T, c["H"], c["W"], *place)
    _same(got, raw.placed(np.full(lay["n"], SENT32, dtype=np.int32), planes, offsets), f"{what}: dst")      # the planes, and the sentinel everywhere else
    out = {"planes": got[torch.from_numpy(offsets.reshape(-1))]}
    if with_u8:
        out["u8"] = u8.read(f"{what}: u8_out")
        _same(out["u8"], want_u8, f"{what}: u8_out")
    return out


STREAMS = ((raw.COLOUR, False), (raw.COLOUR, True), (raw.SEMANTIC, False), (raw.SEMANTIC, True), (raw.DEPTH, False), ("normal", False))


@pytest.mark.parametrize("kind,with_u8", STREAMS, ids=[f"{k}-{'u8' if u else 'planes'}" for k, u in STREAMS])
@pytest.mark.parametrize("width", list(fc.RESIZE_SHAPES))
def test_streams_are_placed_by_the_headers_formula_at_every_width(cuda, width, kind, with_u8):
    """slab = 1, frame0 = 1 of two streams of four frames: everything but the six planes keeps its sentinel."""
    c = fc.resize_case(width)
    print(f"{c['name']}: {c['clause']}")
    _run_stream(c, kind, "planar", cuda, with_u8)


@pytest.mark.parametrize("kind,with_u8", STREAMS[1::2] + STREAMS[4:5], ids=["colour", "semantic", "normal", "depth"])
@pytest.mark.parametrize("width", (4, 516))
def test_each_term_of_the_stream_predicate_falsified_alone_gives_the_same_values(cuda, width, kind, with_u8):
    c = fc.resize_case(width)
    aligned = _run_stream(c, kind, "planar", cuda, with_u8)
    for layout in fc.STREAM_LAYOUTS:
        if layout == "planar" or (layout == "u8_out one byte off" and not with_u8):
            continue
        assert _equal(aligned, _run_stream(c, kind, layout, cuda, with_u8)), layout


# ================================================================================================ depth_normals
def _run_normals(c, dev, offs, labelled=True, limited=True):
    """Depth padding of 10 m and label padding of sky: a read outside a frame's views counts (unlabelled) or hides a pixel (labelled)."""
    what = f"depth_normals {c['name']} {offs} [labels {labelled}, step limit {limited}]"
    n = T * c["H"] * c["W"]
    depth = _put(c["depth"], dev, off=offs.get("depth", 0), fill=10.0)
    lab = _put(c["labels"], dev, off=offs.get("labels", 0), fill=SKY) if labelled else None
    table = _put(c["table"], dev, off=1)
    normals, valid = _blank(3 * n, F32, dev, off=offs.get("normals", 0)), _blank(n, U8, dev, off=offs.get("valid", 0))
    r = fc.REL_STEP if limited else -1.0
    _ok(_lib().mudg_depth_normals(depth.ptr, _ptr(lab), SKY, table.ptr, T, c["H"], c["W"], fc.MIN_DEPTH, fc.MAX_DEPTH, r, normals.ptr, valid.ptr, None), what)
    got = {"normals": normals.read(f"{what}: normals"), "valid": valid.read(f"{what}: valid")}
    _unchanged(what, depth=depth, labels=lab, table=table)
    want_n, want_v = raw.depth_normals(c["depth"], c["table"], c["labels"] if labelled else None, SKY, fc.MIN_DEPTH, fc.MAX_DEPTH, r)
    _same(got["normals"], want_n, f"{what}: normals")
    _same(got["valid"], want_v, f"{what}: valid")
    wide = c["W"] % 4 == 0 and depth.ptr % 16 == 0 and (lab is None or lab.ptr % 16 == 0) and normals.ptr % 16 == 0 and valid.ptr % 4 == 0
    return got, 4 if wide else 1


@pytest.mark.parametrize("hw", fc.PIXEL_SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_depth_normals_equal_the_definition_in_both_forms(cuda, hw):
    c = fc.normals_case(hw)
    print(f"{c['name']}: {c['clause']}; special pixels {c['special']}")
    for labelled in (True, False):
        for limited in (True, False):
            _, form = _run_normals(c, cuda, {}, labelled, limited)
            assert form == (4 if hw[1] % 4 == 0 else 1)


def test_depth_normals_each_pointer_off_alignment_gives_the_same_bits(cuda):
    c = fc.normals_case(fc.ALIGNED_SIZE)
    aligned, form = _run_normals(c, cuda, {})
    assert form == 4
    for name in ("depth", "labels", "normals", "valid"):                                   # one float, one int64, one float, one byte
        moved, form = _run_normals(c, cuda, {name: 1})
        assert form == 1 and _equal(aligned, moved), name
    moved, form = _run_normals(c, cuda, {"depth": 1}, labelled=False)
    assert form == 1


# ================================================================================================ metric_normals
def _run_score(c, dev, offs, with_valid=True):
    """gt padding of (1, 1, 1): a read of it is a counted pixel."""
    what = f"metric_normals {c['name']} {offs} [valid {with_valid}]"
    pred, gt = _put(c["pred"], dev, off=offs.get("pred", 0)), _put(c["gt"], dev, off=offs.get("gt", 0), fill=1.0)
    valid = _put(c["valid"], dev, off=offs.get("valid", 0)) if with_valid else None
    cosines = _put(nm.cos_table(), dev, off=1)
    start = fc.start_sums((T, nm.BINS), 21)
    hist = _put(start, dev, off=1)
    _ok(_lib().mudg_metric_normals(pred.ptr, gt.ptr, _ptr(valid), cosines.ptr, T, c["H"], c["W"], hist.ptr, None), what)
    got = hist.read(f"{what}: hist")
    _unchanged(what, pred=pred, gt=gt, valid=valid, cosines=cosines)
    _same(got, raw.metric_normals(c["pred"], c["gt"], c["valid"] if with_valid else None, start), f"{what}: hist")
    wide = (c["H"] * c["W"]) % 4 == 0 and pred.ptr % 4 == 0 and gt.ptr % 16 == 0 and (valid is None or valid.ptr % 4 == 0)
    return {"hist": got}, 4 if wide else 1


@pytest.mark.parametrize("hw", fc.SCORE_SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_metric_normals_add_to_the_histogram_in_both_forms_and_every_launch_shape(cuda, hw):
    c = fc.score_case(hw)
    print(f"{c['name']}: {c['clause']}; (pixels a lane, workgroups a frame, sweeps) = {fc.score_launch(hw)}")
    for with_valid in (True, False):
        _, form = _run_score(c, cuda, {}, with_valid)
        assert form == fc.score_launch(hw)[0]


def test_metric_normals_each_pointer_off_alignment_gives_the_same_counts(cuda):
    c = fc.score_case(fc.ALIGNED_SIZE)
    aligned, form = _run_score(c, cuda, {})
    assert form == 4
    for name in ("pred", "gt", "valid"):                                                   # one byte, one float, one byte
        moved, form = _run_score(c, cuda, {name: 1})
        assert form == 1 and _equal(aligned, moved), name


# ================================================================================================ lidar_splat_visible
def _run_visible(c, dev, occluded=True, reach=4, keep=0.95, index_base=0, refused=False):
    what = f"lidar_splat_visible {c['name']} [occluders {occluded}, reach {reach}, rel_keep {keep}, index_base {index_base}]"
    n, nmat = len(c["xyz"]), len(c["mats"])
    points = _put(sr.pack(c["xyz"], np.zeros((n, 3), np.uint8)), dev, off=0)
    ids = None if c["ids"] is None else _put(c["ids"], dev, off=1)
    mats = _put(c["mats"], dev, off=1, nan=True)
    Z = _put(c["occluders"], dev, off=1, fill=fc.NEAR_KEY) if occluded else None             # padding of a near depth: a line that left the image would hide
    keys = _put(c["keys"], dev, off=1)
    seg = c["segments"].reshape(-1)
    table = (ctypes.c_int64 * len(seg))(*[int(v) for v in seg])
    fx, fy, cx, cy = (float(v) for v in fc.CAM)
    rc = _lib().mudg_lidar_splat_visible(points.ptr, _ptr(ids), table, len(seg) // 2, mats.ptr, nmat, _ptr(Z), keys.ptr, c["H"], c["W"], fx, fy, cx, cy,
                                         sr.ZNEAR, sr.ZFAR, c["size"], reach, keep, index_base, None)
    if refused:
        _refused(rc, what, "mudg_lidar_splat_visible")
        _unchanged(what, keys=keys, points=points, ids=ids, mats=mats, occluders=Z)
        return None
    _ok(rc, what)
    got = keys.read(f"{what}: keys")
    _unchanged(what, points=points, ids=ids, mats=mats, occluders=Z)
    want, hidden = raw.lidar_splat_visible(c["xyz"], c["ids"], c["segments"], c["mats"], c["occluders"] if occluded else None, c["keys"], fc.CAM, c["size"], reach,
                                           F(keep), index_base)
    print(f"{what}: {int(hidden.sum())} of {len(hidden)} candidates hidden, {int((want != c['keys']).sum())} keys lowered")
    _same(got, want, f"{what}: keys")
    return got


VARIANTS = {"reach 4": dict(), "reach 1": dict(reach=1), "reach 16": dict(reach=16), "rel_keep 1": dict(keep=1.0), "no occluders": dict(occluded=False)}


@pytest.mark.parametrize("variant", fc.VISIBLE_VARIANTS)
@pytest.mark.parametrize("k", range(4), ids=[f"{h}x{w}-{n}" for (h, w), n in zip(fc.SPLAT_IMAGES, fc.SPLAT_CLOUDS)])
def test_lidar_splat_visible_takes_the_minimum_with_what_the_keys_held(cuda, k, variant):
    c = fc.visible_case(k)
    print(f"{c['name']}: {c['clause']}")
    _run_visible(c, cuda, **VARIANTS[variant])


def test_lidar_splat_visible_walks_eight_segments_across_a_workgroup_and_clamps_ids(cuda):
    c = fc.segments_case("eight")
    print(f"{c['name']}: {c['clause']}")
    _run_visible(c, cuda)
    _run_visible(c, cuda, occluded=False)


def test_lidar_splat_visible_numbers_candidates_from_index_base_up_to_two_to_the_32(cuda):
    c = fc.segments_case("twice")
    print(f"{c['name']}: {c['clause']}")
    n = int(c["segments"][:, 1].sum())
    _run_visible(c, cuda, occluded=False)
    _run_visible(c, cuda)
    got = _run_visible(c, cuda, occluded=False, index_base=2 ** 32 - n)                    # index_base + n = 2^32: the last index a key holds
    assert int((got & 0xFFFFFFFF).max()) >= 2 ** 32 - n
    _run_visible(c, cuda, occluded=False, index_base=2 ** 32 - n + 1, refused=True)
    _run_visible(c, cuda, occluded=False, index_base=-1, refused=True)


def test_lidar_splat_visible_hides_by_the_hand_made_occluders(cuda):
    c = fc.probe_case()
    print(f"{c['name']}: {c['clause']}")
    for probe in fc.PROBES:
        print(f"  home {probe[0]}: {probe[3]}")
    _run_visible(c, cuda, reach=fc.PROBE_REACH, keep=fc.PROBE_KEEP)


# ================================================================================================ lidar_depth_resolve
@pytest.mark.parametrize("occluded", (True, False), ids=("occluders", "keys-only"))
@pytest.mark.parametrize("full", (False, True), ids=("empties", "full"))
@pytest.mark.parametrize("pixels", fc.RESOLVE_PIXELS)
def test_lidar_depth_resolve_copies_the_high_word_and_empties_both_key_images(cuda, pixels, full, occluded):
    c = fc.resolve_case(pixels, full)
    print(f"{c['name']}: {c['clause']}")
    keys = _put(c["keys"], cuda, off=1)
    Z = _put(c["occluders"], cuda, off=1) if occluded else None
    depth = _blank(pixels, F32, cuda, off=1)                                               # 4-byte aligned only
    _ok(_lib().mudg_lidar_depth_resolve(keys.ptr, _ptr(Z), depth.ptr, pixels, None), c["name"])
    want, empty = raw.lidar_depth_resolve(c["keys"])
    _same(depth.read("depth"), want, f"resolve {c['name']}: depth")
    _same(keys.read("keys"), empty, f"resolve {c['name']}: keys")
    if occluded:
        _same(Z.read("occluder keys"), empty, f"resolve {c['name']}: occluder keys")


# ================================================================================================ depth_complete
def _run_complete(c, dev, extrapolate, labelled, with_source, stale, scratch_short=0, scratch_move=0):
    """Depth padding of 20 m (filled) and label padding of sky; the scratch is exactly the stated bytes inside its own sentinels."""
    hw = (c["H"], c["W"])
    what = f"depth_complete {c['name']} [extrapolate {extrapolate}, labels {labelled}, source {with_source}, scratch {'stale' if stale else 'sentinel'}]"
    n = T * hw[0] * hw[1]
    nbytes = _lib().mudg_depth_complete_scratch(T, *hw)
    assert nbytes == raw.complete_scratch(T, *hw), (nbytes, raw.complete_scratch(T, *hw))
    depth = _put(c["depth"], dev, off=1, fill=20.0)
    lab = _put(c["labels"], dev, off=1, fill=SKY) if labelled else None
    out, source = _blank(n, F32, dev, off=1), (_blank(n, U8, dev, off=1) if with_source else None)
    scratch = Flat(nbytes, U8, off=0)
    scratch = scratch.put(torch.full((nbytes,), fc.STALE, dtype=U8), dev) if stale else scratch.blank(dev)
    rc = _lib().mudg_depth_complete(depth.ptr, _ptr(lab), SKY, T, hw[0], hw[1], fc.COMPLETE_M, extrapolate, out.ptr, _ptr(source), scratch.ptr + scratch_move,
                                    nbytes - scratch_short, None)
    if scratch_short or scratch_move:
        _refused(rc, f"{what}, {scratch_short} bytes short, {scratch_move} bytes off", "mudg_depth_complete")
        _unchanged(what, depth=depth, labels=lab, out=out, source=source, scratch=scratch)
        return None
    _ok(rc, what)
    got = {"out": out.read(f"{what}: out")}
    if with_source:
        got["source"] = source.read(f"{what}: source")
    scratch.read(f"{what}: scratch")                                                       # nothing outside the stated bytes
    _unchanged(what, depth=depth, labels=lab)
    want_out, want_source = fc.complete_want(hw, extrapolate, labelled)
    _same(got["out"], want_out, f"{what}: out")
    if with_source:
        _same(got["source"], want_source, f"{what}: source")
    return got


@pytest.mark.parametrize("extrapolate", (0, 1))
@pytest.mark.parametrize("hw", fc.COMPLETE_SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_depth_complete_equals_the_definition_over_a_stale_scratch_of_exactly_the_stated_bytes(cuda, hw, extrapolate):
    c = fc.complete_case(hw)
    print(f"{c['name']}: {c['clause']}")
    for labelled in (False, True):
        for with_source in (False, True):
            fresh = _run_complete(c, cuda, extrapolate, labelled, with_source, stale=False)
            again = _run_complete(c, cuda, extrapolate, labelled, with_source, stale=True)
            assert _equal(fresh, again)


def test_depth_complete_scratch_follows_the_headers_formula_and_a_wrong_scratch_is_refused(cuda):
    for shape in ((1, 1, 1), (2, 1, 1), (2, 3, 5), (3, 7, 9), (2, 33, 65), (65535, 1, 1), (1, 65535, 256), (1, 4096, 4096)):
        assert _lib().mudg_depth_complete_scratch(*shape) == raw.complete_scratch(*shape), shape
    for shape in ((0, 1, 1), (65536, 1, 1), (1, 0, 4), (1, 4, 0), (1, 65536, 1), (1, 4097, 4096)):
        assert _lib().mudg_depth_complete_scratch(*shape) == -1, shape
    c = fc.complete_case((31, 33))
    _run_complete(c, cuda, 1, True, True, stale=False, scratch_short=1)
    _run_complete(c, cuda, 1, True, True, stale=False, scratch_move=4)


# ================================================================================================ post.hip
@pytest.mark.parametrize("HW", fc.U8_HW)
@pytest.mark.parametrize("C", (1, 3))
def test_frames_to_u8_equals_the_definition_on_every_byte_boundary(cuda, C, HW):
    video = fc.u8_video(C, HW)
    src, out = _put(video, cuda, off=1, nan=True), _blank(video.size, U8, cuda, off=1)
    _ok(_lib().mudg_frames_to_u8(src.ptr, out.ptr, 2, C, 2, HW, None), f"frames_to_u8 C={C} HW={HW}")
    _same(out.read("out"), raw.frames_to_u8(video), f"frames_to_u8 C={C} HW={HW}")
    src.unchanged("video")


def _run_sheet(C, hw, clamp, rescale, dev, video_off=0, out_off=0):
    what = f"log_sheet C={C} {hw} clamp={clamp} rescale={rescale} [video +{video_off}, out +{out_off}]"
    video = fc.sheet_video(C, hw, clamp, rescale)
    src, out = _put(video, dev, off=video_off, nan=True), _blank(2 * 2 * hw[0] * hw[1] * 3, U8, dev, off=out_off)
    _ok(_lib().mudg_log_sheet(src.ptr, out.ptr, 2, C, 2, hw[0], hw[1], clamp, rescale, None), what)
    got = out.read(f"{what}: out")
    src.unchanged(f"{what}: video")
    _same(got, raw.log_sheet(video, clamp, rescale), what)
    return got


@pytest.mark.parametrize("hw", fc.SHEET_SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("C", (1, 3))
def test_log_sheet_equals_the_definition_in_both_forms_and_the_four_settings(cuda, C, hw):
    for clamp, rescale in fc.SHEET_SETTINGS:
        aligned = _run_sheet(C, hw, clamp, rescale, cuda)
        assert torch.equal(aligned, _run_sheet(C, hw, clamp, rescale, cuda, video_off=1))   # one float off: the one-pixel form
        assert torch.equal(aligned, _run_sheet(C, hw, clamp, rescale, cuda, out_off=1))     # one byte off


@pytest.mark.parametrize("pixels", fc.POST_PIXELS)
def test_depth_from_u8_equals_the_definition(cuda, pixels):
    frames = fc.u8_pixels(pixels)
    src, depth = _put(frames, cuda, off=1), _blank(pixels, F32, cuda, off=1)
    _ok(_lib().mudg_depth_from_u8(src.ptr, depth.ptr, pixels, None), f"depth_from_u8 {pixels}")
    _same(depth.read("depth"), raw.depth_from_u8(frames), f"depth_from_u8 {pixels}")
    src.unchanged("frames")


@pytest.mark.parametrize("hw", fc.U8_HW)
def test_semantic_nearest_gives_the_first_of_equally_near_colours(cuda, hw):
    img = fc.semantic_image(hw)
    src, vis, labels = _put(img, cuda, off=1), _blank(3 * hw, U8, cuda, off=1), _blank(hw, I64, cuda, off=1)
    _ok(_lib().mudg_semantic_nearest(src.ptr, vis.ptr, labels.ptr, hw, None), f"semantic_nearest {hw}")
    want_vis, want_labels = raw.semantic_nearest(img)
    _same(vis.read("vis"), want_vis, f"semantic_nearest {hw}: vis")
    _same(labels.read("labels"), want_labels, f"semantic_nearest {hw}: labels")
    src.unchanged("img")


# ================================================================================================ refusals
def test_bad_arguments_are_refused_before_any_launch(cuda):
    """A null pointer, a size of zero or a table that is not 16-byte aligned: -1, the entry's name in the message, every buffer untouched."""
    lib = _lib()
    a, b, c, d = (Flat(64, U8, off=0).blank(cuda) for _ in range(4))
    w = Flat(64, I64, off=0).blank(cuda)
    seg = (ctypes.c_int64 * 2)(0, 1)
    calls = (
        ("mudg_resize_u8", lambda: lib.mudg_resize_u8(None, b.ptr, 1, 2, 2, 1, 2, 2, 0, 0, w.ptr, w.ptr, None)),
        ("mudg_resize_u8", lambda: lib.mudg_resize_u8(a.ptr, b.ptr, 1, 2, 2, 2, 2, 2, 0, 0, w.ptr, w.ptr, None)),
        ("mudg_resize_u8", lambda: lib.mudg_resize_u8(a.ptr, b.ptr, 1, 2, 2, 1, 2, 2, 0, 0, w.ptr + 8, w.ptr, None)),
        ("mudg_resize_f32", lambda: lib.mudg_resize_f32(a.ptr, b.ptr, 0, 2, 2, 2, 2, w.ptr, w.ptr, None)),
        ("mudg_resize_f32", lambda: lib.mudg_resize_f32(a.ptr, b.ptr, 1, 2, 2, 2, 2, w.ptr, w.ptr + 8, None)),
        ("mudg_dense_stream", lambda: lib.mudg_dense_stream(2, a.ptr, 1, 2, 2, 2, 2, w.ptr, w.ptr, None, b.ptr, 12, 4, 4, 0, 0, c.ptr, None)),
        ("mudg_dense_stream", lambda: lib.mudg_dense_stream(0, a.ptr, 1, 2, 2, 2, 2, w.ptr, w.ptr, None, b.ptr, 12, 4, 4, 0, 0, None, None)),
        ("mudg_dense_stream", lambda: lib.mudg_dense_stream(2, a.ptr, 1, 2, 2, 2, 2, w.ptr, w.ptr, None, b.ptr, 12, 4, 3, 0, 0, None, None)),
        ("mudg_dense_stream", lambda: lib.mudg_dense_stream(2, a.ptr, 1, 2, 2, 2, 2, w.ptr, w.ptr, None, b.ptr + 1, 12, 4, 4, 0, 0, None, None)),
        ("mudg_normal_stream", lambda: lib.mudg_normal_stream(a.ptr + 2, 1, 2, 2, 2, 2, w.ptr, w.ptr, b.ptr, 12, 4, 4, 0, 0, None)),
        ("mudg_normal_stream", lambda: lib.mudg_normal_stream(a.ptr, 1, 2, 2, 2, 2, w.ptr, w.ptr, b.ptr, 12, 4, 4, -1, 0, None)),
        ("mudg_depth_normals", lambda: lib.mudg_depth_normals(a.ptr, None, SKY, None, 1, 2, 2, 0.0, 1.0, -1.0, b.ptr, c.ptr, None)),
        ("mudg_depth_normals", lambda: lib.mudg_depth_normals(a.ptr, None, SKY, w.ptr, 1, 2, 2, 1.0, 1.0, -1.0, b.ptr, c.ptr, None)),
        ("mudg_depth_normals", lambda: lib.mudg_depth_normals(a.ptr, None, SKY, w.ptr, 1, 2, 2, 0.0, 1.0, float("nan"), b.ptr, c.ptr, None)),
        ("mudg_metric_normals", lambda: lib.mudg_metric_normals(a.ptr, b.ptr, None, None, 1, 2, 2, w.ptr, None)),
        ("mudg_metric_normals", lambda: lib.mudg_metric_normals(a.ptr, b.ptr, None, w.ptr, 0, 2, 2, w.ptr, None)),
        ("mudg_lidar_splat_visible", lambda: lib.mudg_lidar_splat_visible(a.ptr, None, seg, 9, b.ptr, 1, None, w.ptr, 2, 2, 1.0, 1.0, 0.0, 0.0, 0.1, 9.0, 1.0, 4, 0.95, 0, None)),
        ("mudg_lidar_splat_visible", lambda: lib.mudg_lidar_splat_visible(a.ptr, None, seg, 1, b.ptr, 1, w.ptr, w.ptr, 2, 2, 1.0, 1.0, 0.0, 0.0, 0.1, 9.0, 1.0, 17, 0.95, 0, None)),
        ("mudg_lidar_splat_visible", lambda: lib.mudg_lidar_splat_visible(a.ptr, None, seg, 1, b.ptr, 2, None, w.ptr, 2, 2, 1.0, 1.0, 0.0, 0.0, 0.1, 9.0, 1.0, 4, 0.95, 0, None)),
        ("mudg_lidar_depth_resolve", lambda: lib.mudg_lidar_depth_resolve(w.ptr, None, a.ptr, 0, None)),
        ("mudg_lidar_depth_resolve", lambda: lib.mudg_lidar_depth_resolve(w.ptr + 4, None, a.ptr, 4, None)),
        ("mudg_depth_complete", lambda: lib.mudg_depth_complete(a.ptr, None, SKY, 1, 2, 2, 0.05, 1, b.ptr, None, c.ptr, 64, None)),
        ("mudg_frames_to_u8", lambda: lib.mudg_frames_to_u8(a.ptr, None, 1, 1, 1, 4, None)),
        ("mudg_depth_from_u8", lambda: lib.mudg_depth_from_u8(a.ptr, b.ptr, 0, None)),
        ("mudg_semantic_nearest", lambda: lib.mudg_semantic_nearest(a.ptr, b.ptr, None, 4, None)),
        ("mudg_log_sheet", lambda: lib.mudg_log_sheet(a.ptr, b.ptr, 1, 2, 1, 2, 2, 1, 1, None)),
    )
    assert {name[5:] for name, _ in calls} == set(fc.ENTRY_POINTS)
    for name, call in calls:
        _refused(call(), name, name)
        _unchanged(name, a=a, b=b, c=c, d=d, w=w)
