"""The three entry points of csrc/splat.hip called directly through hip.lib(), with raw pointers into sentinel-filled buffers
(sentinel_buffers.Flat), on the cases of tests/splat_cases.py: images that are no whole tiles, clouds that do not fill their last
workgroup, every sprite size, hand-placed points on every bound of the rule, out-of-range ids, unaligned bases, pose strides with a gap.
The definition is tests/splat_reference.py; every comparison is torch.equal on the bits, no tolerance and no pixel left out, and after
every call everything outside each view must still hold its sentinel.  Float operands the kernels only read lie in NaN, integer ones in
the byte 0xA5: a read of padding shows in the result.  tests/test_splat_cpu.py asserts that each case reaches the clause it names."""
import numpy as np
import pytest
import torch

import splat_cases as sc
import splat_reference as sr
from sentinel_buffers import Flat

pytestmark = pytest.mark.gpu
I64, I32, F32, U8 = torch.int64, torch.int32, torch.float32, torch.uint8
NO_EARLY_REJECT = 1                                             # MUDG_SPLAT_NO_EARLY_REJECT (include/mudg_hip.h)
EINVAL = -1
SENTINEL_F32 = np.frombuffer(bytes([0xA5] * 4), dtype=np.float32)[0]


def _t(a):
    """numpy -> a tensor of the same bits (unsigned words as the signed type of their width)."""
    a = np.ascontiguousarray(a)
    a = a.view({np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype))
    return torch.from_numpy(a.copy()).reshape(-1)


def _bits(x):
    return x.view(I32) if x.dtype == F32 else x


def _same(got, want, what):
    got, want = _bits(got.reshape(-1)), _bits(_t(want))
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    differ = int((got != want).sum())
    print(f"{what}: {differ} of {want.numel()} values differ")
    assert torch.equal(got, want), (what, differ)


def _ptr(buf):
    return None if buf is None else buf.ptr


def _lib():
    from mudg_amd import hip
    return hip.lib()


def _ok(rc, what):
    msg = _lib().mudg_last_error()
    assert rc == 0, (what, rc, msg.decode() if msg else "")


# ------------------------------------------------------------------------------------------------ mudg_splat_points
def _draw(case, dev, *, ids, stats, early_reject, seed=None):
    """One launch into a key image (seed, or empty) that lies 8 bytes off a 16-byte address inside its sentinels.  Returns the keys and
    what was added to the counter pair."""
    n, (P, nmat), H, W = len(case["xyz"]), case["mats"].shape[:2], case["H"], case["W"]
    pts = Flat(4 * n, I32).put(_t(sr.pack(case["xyz"], case["rgb"])), dev)
    mats = Flat(12 * P * nmat, F32, off=1, nan=True).put(_t(case["mats"]), dev)
    idb = None if ids is None else Flat(n, I32, off=1).put(_t(ids), dev)
    keys = Flat(P * H * W, I64, off=1).put(_t(np.full((P, H, W), sr.EMPTY) if seed is None else seed), dev)
    start = (1000, 77)
    st = Flat(2, I64, off=1).put(torch.tensor(start, dtype=I64), dev) if stats else None
    fx, fy, cx, cy = (float(v) for v in sc.CAM)
    rc = _lib().mudg_splat_points(pts.ptr, _ptr(idb), n, mats.ptr, P, nmat, keys.ptr, H, W, fx, fy, cx, cy, float(case["znear"]), float(case["zfar"]),
                                  case["size"], 0 if early_reject else NO_EARLY_REJECT, _ptr(st), None)
    _ok(rc, case["name"])
    torch.cuda.synchronize()
    got = keys.read(f"{case['name']}: keys")
    for buf, what in ((pts, "points"), (mats, "matrices"), (idb, "ids")):
        if buf is not None:
            buf.unchanged(f"{case['name']}: {what}")
    added = None
    if stats:
        added = tuple(int(a) - b for a, b in zip(st.read(f"{case['name']}: stats"), start))
    return got, added


@pytest.mark.parametrize("name", [c["name"] for c in sc.points_cases()])
def test_splat_points_equals_the_definition_in_every_form(cuda, name):
    """The key image as integers against the definition's, for the four template forms (ids or none, counters or none) with the early
    reject on and off; the counters added to a non-zero pair; then the same cloud drawn on top of a seeded key image."""
    case = {c["name"]: c for c in sc.points_cases()}[name]
    print(f"{name}: {case['clause']}")
    want, covered = sc.points_keys(name)
    nonempty = int((want != sr.EMPTY).sum())
    nmat = case["mats"].shape[1]
    id_forms = [case["ids"]] if nmat > 1 else [None, case["ids"] if case["ids"] is not None else np.zeros(len(case["xyz"]), np.int32)]
    for ids in id_forms:
        for stats in (False, True):
            for early_reject in (True, False):
                what = f"{name} [ids {ids is not None}, stats {stats}, early reject {early_reject}]"
                got, added = _draw(case, cuda, ids=ids, stats=stats, early_reject=early_reject)
                _same(got, want, what)
                if stats:
                    print(f"{what}: covered {added[0]} (definition {covered}), issued {added[1]}, {nonempty} pixels drawn")
                    assert added[0] == covered, (what, added, covered)
                    assert added[1] == covered if not early_reject else nonempty <= added[1] <= covered, (what, added, nonempty, covered)
    seed = sc.seeded_keys(case)
    args = (sc.CAM, case["size"], case["H"], case["W"], case["znear"], case["zfar"])
    on_top = np.stack([sr.splat_keys(case["xyz"], m[0] if case["ids"] is None else m, *args, ids=case["ids"], seed=seed[p])
                       for p, m in enumerate(case["mats"])])
    assert np.array_equal(on_top, np.minimum(seed, want))                                 # keys only ever decrease
    for early_reject in (True, False):
        got, _ = _draw(case, cuda, ids=case["ids"], stats=False, early_reject=early_reject, seed=seed)
        _same(got, on_top, f"{name} [on a seeded image, early reject {early_reject}]")


# ------------------------------------------------------------------------------------------------ mudg_splat_resolve
def _resolve(dev, pixels, offs, name):
    ko, do, co = offs
    keys = Flat(pixels, I64, off=ko).put(_t(sc.resolve_keys(pixels)), dev)
    pts = Flat(4 * sc.RESOLVE_BUFFER, I32).put(_t(sc.resolve_points()), dev)
    depth, colour = Flat(pixels, F32, off=do).blank(dev), Flat(pixels, I32, off=co).blank(dev)
    wide = pixels % 4 == 0 and all(b.ptr % 16 == 0 for b in (keys, depth, colour))
    rc = _lib().mudg_splat_resolve(keys.ptr, pts.ptr, sc.RESOLVE_POINTS, depth.ptr, colour.ptr, pixels, None)
    _ok(rc, name)
    torch.cuda.synchronize()
    pts.unchanged(f"{name}: points")
    return depth.read(f"{name}: depth"), colour.read(f"{name}: colour"), keys.read(f"{name}: keys"), 4 if wide else 1


@pytest.mark.parametrize("name", [c[0] for c in sc.RESOLVE_CASES])
def test_splat_resolve_equals_the_definition_and_clears_the_keys(cuda, name):
    _, clause, pixels, offs, form = {c[0]: c for c in sc.RESOLVE_CASES}[name]
    print(f"{name}: {clause}")
    want_d, want_c, want_k = sr.resolve(sc.resolve_keys(pixels), sc.resolve_points(), sc.RESOLVE_POINTS)
    depth, colour, keys, ran = _resolve(cuda, pixels, offs, name)
    assert ran == form, (name, ran, form)                                                 # the addresses choose the kernel the case aims at
    _same(depth, want_d, f"resolve {name}: depth")
    _same(colour, want_c, f"resolve {name}: colour")
    _same(keys, want_k, f"resolve {name}: keys afterwards")
    assert bool((keys == -1).all())


def test_both_forms_of_splat_resolve_give_the_same_bits(cuda):
    wide = _resolve(cuda, 1024, (0, 0, 0), "1024 wide")
    for offs in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        narrow = _resolve(cuda, 1024, offs, f"1024 narrow {offs}")
        assert wide[3] == 4 and narrow[3] == 1
        for a, b, what in zip(wide[:3], narrow[:3], ("depth", "colour", "keys")):
            assert torch.equal(_bits(a), _bits(b)), (offs, what)


# ------------------------------------------------------------------------------------------------ mudg_splat_compose
def _compose(dev, hw, *, T, t, gap=0, obj=True, outs=("rgb", "depth", "mask"), poses=2):
    """One call on the layers of sc.compose_layers(hw); sparse_frames and sparse_depth are compared over their whole extent (every
    frame, the gaps between the poses) with the definition written into sentinel-filled arrays.  Returns their bits."""
    H, W = hw
    plane = H * W
    bg_c, bg_d, ob_c, ob_d = sc.compose_layers(hw, poses)
    stride = 3 * T * plane + gap
    extent = (poses - 1) * stride + 3 * T * plane
    what = f"compose {H}x{W} [T {T}, t {t}, gap {gap}, object layer {obj}, outputs {'+'.join(outs) or 'none'}]"
    want_s, want_d = np.full(extent, SENTINEL_F32), np.full(extent, SENTINEL_F32)
    want_rgb, want_depth, want_mask = sr.compose_frame(want_s, want_d, stride, T, t, bg_c, bg_d, *((ob_c, ob_d) if obj else ()))
    ins = dict(bg_c=Flat(poses * plane, I32, off=1).put(_t(bg_c), dev), bg_d=Flat(poses * plane, F32, off=3, nan=True).put(_t(bg_d), dev))
    if obj:
        ins.update(ob_c=Flat(poses * plane, I32, off=2).put(_t(ob_c), dev), ob_d=Flat(poses * plane, F32, off=1, nan=True).put(_t(ob_d), dev))
    sparse, sdepth = Flat(extent, F32, off=1).blank(dev), Flat(extent, F32, off=3).blank(dev)
    out = dict(rgb=Flat(3 * poses * plane, U8, off=1).blank(dev) if "rgb" in outs else None,
               depth=Flat(poses * plane, F32, off=1).blank(dev) if "depth" in outs else None,
               mask=Flat(poses * plane, U8, off=3).blank(dev) if "mask" in outs else None)
    rc = _lib().mudg_splat_compose(ins["bg_c"].ptr, ins["bg_d"].ptr, _ptr(ins.get("ob_c")), _ptr(ins.get("ob_d")), sparse.ptr, sdepth.ptr, stride,
                                   poses, T, t, H, W, _ptr(out["rgb"]), _ptr(out["depth"]), _ptr(out["mask"]), None)
    _ok(rc, what)
    torch.cuda.synchronize()
    for k, buf in ins.items():
        buf.unchanged(f"{what}: {k}")
    got_s, got_d = sparse.read(f"{what}: sparse_frames"), sdepth.read(f"{what}: sparse_depth")
    _same(got_s, want_s, f"{what}: sparse_frames")
    _same(got_d, want_d, f"{what}: sparse_depth")
    for k, want in (("rgb", want_rgb), ("depth", want_depth), ("mask", want_mask)):
        if out[k] is not None:
            _same(out[k].read(f"{what}: {k}"), want, f"{what}: {k}")
    return _bits(got_s), _bits(got_d)


@pytest.mark.parametrize("hw", sc.COMPOSE_SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_splat_compose_equals_the_definition_frame_by_frame(cuda, hw):
    """T = 3 at every t (the other frames keep their sentinel), a pose stride with a gap of 24 floats, no object layer, and each
    optional output alone: the condition tensors are the same bits whichever outputs are asked for."""
    print(sc.compose_clause(hw))
    for t in range(3):
        _compose(cuda, hw, T=3, t=t)
    _compose(cuda, hw, T=2, t=1, gap=24)
    _compose(cuda, hw, T=1, t=0, obj=False)
    _compose(cuda, hw, T=2, t=0, obj=False, outs=(), gap=24)
    full = _compose(cuda, hw, T=1, t=0)
    for outs in ((), ("rgb",), ("depth",), ("mask",)):
        some = _compose(cuda, hw, T=1, t=0, outs=outs)
        assert torch.equal(some[0], full[0]) and torch.equal(some[1], full[1]), outs


# ------------------------------------------------------------------------------------------------ refusals
def _valid_call(entry, dev):
    """A small valid call of each entry point: (the buffers by argument name, the other arguments, how to make the call)."""
    lib = _lib()
    if entry == "points":
        case = sc.points_cases()[0]
        n = 8
        xyz = np.tile(np.array([[0.5, 0.5, 1.0]], np.float32), (n, 1))
        bufs = dict(points=Flat(4 * n, I32).put(_t(sr.pack(xyz, case["rgb"][:n])), dev), mats=Flat(36, F32, nan=True).put(_t(np.stack([sc.EYE] * 3)), dev),
                    keys=Flat(64, I64).put(_t(np.full(64, sr.EMPTY)), dev), stats=Flat(2, I64).blank(dev))
        args = dict(n=n, poses=1, nmat=1, H=8, W=8, znear=1e-4, zfar=200.0, point_size=2.5)

        def call(p, a):
            return lib.mudg_splat_points(p["points"], None, a["n"], p["mats"], a["poses"], a["nmat"], p["keys"], a["H"], a["W"], 1.0, 1.0, 0.0, 0.0,
                                         a["znear"], a["zfar"], a["point_size"], 0, p["stats"], None)
    elif entry == "resolve":
        bufs = dict(keys=Flat(16, I64).put(_t(np.full(16, sr.EMPTY)), dev), points=Flat(32, I32).blank(dev), depth=Flat(16, F32).blank(dev),
                    colour=Flat(16, I32).blank(dev))
        args = dict(n=8, pixels=16)

        def call(p, a):
            return lib.mudg_splat_resolve(p["keys"], p["points"], a["n"], p["depth"], p["colour"], a["pixels"], None)
    else:
        bufs = dict(bg_colour=Flat(64, I32).blank(dev), bg_depth=Flat(64, F32).blank(dev), obj_colour=Flat(64, I32).blank(dev),
                    obj_depth=Flat(64, F32).blank(dev), sparse=Flat(576, F32).blank(dev), sdepth=Flat(576, F32).blank(dev),
                    rgb_out=Flat(192, U8).blank(dev), depth_out=Flat(64, F32).blank(dev), mask_out=Flat(64, U8).blank(dev))
        args = dict(pose_stride=576, poses=1, T=3, t=1, H=8, W=8)

        def call(p, a):
            return lib.mudg_splat_compose(p["bg_colour"], p["bg_depth"], p["obj_colour"], p["obj_depth"], p["sparse"], p["sdepth"], a["pose_stride"],
                                          a["poses"], a["T"], a["t"], a["H"], a["W"], p["rgb_out"], p["depth_out"], p["mask_out"], None)
    return bufs, args, call


@pytest.mark.parametrize("entry", ["points", "resolve", "compose"])
def test_the_refused_calls_start_from_a_valid_one(cuda, entry):
    bufs, args, call = _valid_call(entry, cuda)
    _ok(call({k: b.ptr for k, b in bufs.items()}, args), entry)
    torch.cuda.synchronize()
    for k, b in bufs.items():
        b.read(f"{entry}: {k}")                                                           # the guards hold


@pytest.mark.parametrize("entry,wrong", [r[:2] for r in sc.REFUSALS], ids=[f"{r[0]}: {r[1]}" for r in sc.REFUSALS])
def test_bad_arguments_are_refused_before_any_launch(cuda, entry, wrong):
    _, _, changes, piece = {r[:2]: r for r in sc.REFUSALS}[(entry, wrong)]
    bufs, args, call = _valid_call(entry, cuda)
    ptrs = {k: b.ptr for k, b in bufs.items()}
    for k, v in changes.items():
        if k in ptrs:
            ptrs[k] = None if v is None else ptrs[k] + v                                  # a null pointer, or one moved by v bytes
        elif k == "pose_stride_delta":
            args["pose_stride"] = 3 * args["T"] * args["H"] * args["W"] + v
        else:
            assert k in args, k
            args[k] = v
    rc = call(ptrs, args)
    msg = _lib().mudg_last_error()
    torch.cuda.synchronize()
    assert rc == EINVAL and msg and piece in msg.decode(), (entry, wrong, rc, msg)
    for k, b in bufs.items():
        b.unchanged(f"{entry}, {wrong}: {k}")
