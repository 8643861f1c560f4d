"""Clouds rendered as 3D Gaussians: the forward half of a tile-binned splat renderer on the GPU (csrc/gaussians.hip).

MuDG's generated views end up in a scene of 3D Gaussians that is rendered at poses nobody drove.  The point splat of render.py is
sparse on purpose (its images are the model's conditions): it has no opacity, no footprint that grows towards the camera, and leaves
holes.  Here every point of a PointCloud carries a covariance and an opacity; a call projects them with EWA covariances, bins them into
16 x 16 tiles, sorts each tile by depth and blends front to back.  The rule is stated operation by operation in DESIGN.md §23 and
the numpy definition that the tests keep reproduces it bit for bit.  Colour is one constant per Gaussian, or, with coefficients `sh`
(csrc/gaussians_sh.hip), that constant plus real spherical harmonics of degrees 1 .. 3 of the direction the Gaussian is
seen from.  `render` is the inference path; `render_differentiable`, `GaussianModel` and `fit` optimise position,
covariance, opacity and colour (with `sh_degree` also the harmonics) against images through the backward kernels of
csrc/gaussians_bwd.hip; `DensityControl`, `DensityStats` and `densify_and_prune` let a
fit clone, split and prune its Gaussians through csrc/gaussians_density.hip; `image_loss` is 3DGS's L1 + D-SSIM loss with
its backward in csrc/gaussians_loss.hip, which `fit(..., ssim_weight=0.2)` minimises; `render_differentiable` also differentiates its
matrices (csrc/gaussians_pose.hip), and `CameraPoses` with `fit(..., poses=)` refines the cameras.  There is no CPU path: tensors that are not on the GPU are
an error.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from . import hip, ops
from .render import ZFAR, ObjectSet, PointCloud, scaled_intrinsics, virtual_poses

ZNEAR = 0.2                      # the Jacobian has 1 / zc^2
MAX_ENTRIES = 2 ** 28            # (key, value) pairs a call may sort: 3 GiB of keys and values


def rotation_from_quaternions(quats):
    """Unit-or-not quaternions (n, 4) as (w, x, y, z) -> (n, 3, 3): the rotation of the normalised quaternion, in torch."""
    w, x, y, z = (quats / quats.norm(dim=1, keepdim=True)).unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)


def covariance_from_scales_rotations(scales, quats):
    """scales (n, 3) and unit-or-not quaternions (n, 4) as (w, x, y, z) -> (n, 6) fp32 (xx, xy, xz, yy, yz, zz) of R S^2 R^T, in torch on
    the tensors' device."""
    scales = torch.as_tensor(scales, dtype=torch.float32)
    quats = torch.as_tensor(quats, dtype=torch.float32).to(scales.device)
    if scales.dim() != 2 or scales.shape[1] != 3 or tuple(quats.shape) != (scales.shape[0], 4):
        raise hip.MudgError(f"expected scales (n, 3) and quaternions (n, 4), got {tuple(scales.shape)} and {tuple(quats.shape)}")
    m = rotation_from_quaternions(quats) * scales[:, None, :]             # R S
    full = m @ m.transpose(1, 2)
    return torch.stack([full[:, 0, 0], full[:, 0, 1], full[:, 0, 2], full[:, 1, 1], full[:, 1, 2], full[:, 2, 2]], dim=1).contiguous()


def _on_gpu(name, t, dtype, shape):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype or tuple(t.shape) != tuple(shape):
        got = f"{tuple(t.shape)} {t.dtype} on {t.device}" if torch.is_tensor(t) else type(t).__name__
        raise hip.MudgError(f"{name}: expected a {dtype} tensor of shape {tuple(shape)} on the GPU (there is no CPU path), got {got}")
    return t.contiguous()


class Gaussians:
    """A PointCloud (positions and colours), `cov` (n, 6) fp32 = (xx, xy, xz, yy, yz, zz) in the point's own frame (the world for the
    background, the object's frame for an object), `opacity` (n,) fp32 in [0, 1] and `ids` (n,) int32 or None: the matrix a point goes
    through, 0 for the background and 1 + object for an object.  `sh` (n, K - 1, 3) fp32 in byte units or None: the coefficients of the
    real spherical harmonics of degrees 1 .. L, K = (L + 1)^2, L = 1, 2 or 3; with them `colour` (n, 3) fp32 in byte units
    is the direction-independent term (default: the cloud's bytes), and render draws max(0, colour + sum B_k(d) sh[k - 1]) per view.
    `features` (n, F) fp32 or None, 1 <= F <= ops.GAUSS_FEAT_MAX: a row of class scores per Gaussian; with them render
    also returns the blended scores and a label image."""
    sh = colour = features = None

    def __init__(self, cloud: PointCloud, cov: torch.Tensor, opacity: torch.Tensor, ids: Optional[torch.Tensor] = None,
                 sh: Optional[torch.Tensor] = None, colour: Optional[torch.Tensor] = None, features: Optional[torch.Tensor] = None):
        if not isinstance(cloud, PointCloud) or not cloud.points.is_cuda:
            raise hip.MudgError("Gaussians: the cloud is a PointCloud on the GPU (there is no CPU path)")
        n = len(cloud)
        self.cloud = cloud
        self.cov = _on_gpu("Gaussians: cov", cov, torch.float32, (n, 6))
        self.opacity = _on_gpu("Gaussians: opacity", opacity, torch.float32, (n,))
        self.ids = None if ids is None else _on_gpu("Gaussians: ids", ids, torch.int32, (n,))
        self.sh = self.colour = None
        if sh is not None:
            self.sh = _on_gpu("Gaussians: sh", sh, torch.float32, (n, _sh_rows_of("Gaussians", sh), 3))
            self.colour = _byte_colours(cloud.points) if colour is None else _on_gpu("Gaussians: colour", colour, torch.float32, (n, 3))
        elif colour is not None:
            raise hip.MudgError("Gaussians: colour comes with sh; without harmonics the colour is the cloud's bytes")
        self.features = None if features is None else _on_gpu("Gaussians: features", features, torch.float32, (n, _feature_width_of("Gaussians", features)))

    def __len__(self):
        return len(self.cloud)

    @staticmethod
    def _per_point(name, value, n, device):
        if torch.is_tensor(value) and value.dim() > 0:
            if tuple(value.shape) != (n,):
                raise hip.MudgError(f"Gaussians: {name} is a number or an (n,) tensor, got {tuple(value.shape)} for {n} points")
            return value.to(device=device, dtype=torch.float32)
        return torch.full((n,), float(value), dtype=torch.float32, device=device)

    @classmethod
    def from_cloud(cls, cloud: PointCloud, scale, opacity=1.0, ids=None):
        """Isotropic: covariance s^2 I.  scale: a number or an (n,) tensor, metres; for a cloud thinned at voxel_size a multiple of it."""
        if not isinstance(cloud, PointCloud) or not cloud.points.is_cuda:
            raise hip.MudgError("Gaussians.from_cloud: the cloud is a PointCloud on the GPU (there is no CPU path)")
        n, dev = len(cloud), cloud.points.device
        s = cls._per_point("scale", scale, n, dev)
        cov = torch.zeros((n, 6), dtype=torch.float32, device=dev)
        cov[:, 0] = cov[:, 3] = cov[:, 5] = s * s
        return cls(cloud, cov, cls._per_point("opacity", opacity, n, dev), ids)

    @classmethod
    def from_scales_rotations(cls, cloud: PointCloud, scales, quats, opacity=1.0, ids=None):
        """Covariance R S^2 R^T from per-axis scales (n, 3) and quaternions (n, 4) = (w, x, y, z)."""
        if not isinstance(cloud, PointCloud) or not cloud.points.is_cuda:
            raise hip.MudgError("Gaussians.from_scales_rotations: the cloud is a PointCloud on the GPU (there is no CPU path)")
        n, dev = len(cloud), cloud.points.device
        cov = covariance_from_scales_rotations(torch.as_tensor(scales).to(dev), torch.as_tensor(quats).to(dev))
        return cls(cloud, cov, cls._per_point("opacity", opacity, n, dev), ids)

    @classmethod
    def from_scene(cls, background: PointCloud, objects: Optional[ObjectSet], scale, object_scale=None, opacity=1.0):
        """One set for a scene: the background with id 0 and scale `scale`, every object's points with id 1 + object and `object_scale`
        (default: `scale`), so that one sort lets them occlude one another."""
        if not isinstance(background, PointCloud) or (objects is not None and not isinstance(objects, ObjectSet)):
            raise hip.MudgError("Gaussians.from_scene: the background is a PointCloud and the objects an ObjectSet (or None)")
        if objects is None:
            return cls.from_cloud(background, scale, opacity)
        if torch.is_tensor(scale) and scale.dim() > 0 or torch.is_tensor(object_scale) and object_scale.dim() > 0:
            raise hip.MudgError("Gaussians.from_scene: scale and object_scale are numbers")
        nb, no, dev = len(background), len(objects.cloud), background.points.device
        s = torch.cat([torch.full((nb,), float(scale)), torch.full((no,), float(scale if object_scale is None else object_scale))]).to(dev)
        ids = torch.cat([torch.zeros((nb,), dtype=torch.int32, device=dev), objects.ids.to(dev) + 1])
        return cls.from_cloud(PointCloud.concatenated(background, objects.cloud), s, opacity, ids)


def _sh_rows_of(name, sh):
    """K - 1 of coefficients (n, K - 1, 3), refused in `name`'s words unless L is 1, 2 or 3."""
    rows = sh.shape[1] if torch.is_tensor(sh) and sh.dim() == 3 else -1
    if rows not in [ops.gauss_sh_rows(d) for d in range(1, ops.GAUSS_SH_MAX_DEGREE + 1)]:
        got = tuple(sh.shape) if torch.is_tensor(sh) else type(sh).__name__
        raise hip.MudgError(f"{name}: sh is an (n, K - 1, 3) fp32 tensor on the GPU with K = 4, 9 or 16 (degrees 1 .. 3), got {got}")
    return rows


def _feature_width_of(name, features):
    """F of features (n, F), refused in `name`'s words unless 1 <= F <= ops.GAUSS_FEAT_MAX."""
    width = features.shape[1] if torch.is_tensor(features) and features.dim() == 2 else -1
    if not 1 <= width <= ops.GAUSS_FEAT_MAX:
        got = tuple(features.shape) if torch.is_tensor(features) else type(features).__name__
        raise hip.MudgError(f"{name}: features is an (n, F) fp32 tensor on the GPU with 1 <= F <= {ops.GAUSS_FEAT_MAX}, got {got}")
    return width


def label_image(features, alpha, label_alpha=0.5):
    """Blended scores (..., F, H, W) and alpha (..., H, W) -> uint8 labels (..., H, W): the argmax over the F scores, the lowest index
    on ties, and 255 (unlabelled) where alpha <= label_alpha."""
    best = features.max(dim=-3, keepdim=True).values
    index = torch.arange(features.shape[-3], device=features.device).reshape(-1, 1, 1)
    first = torch.where(features == best, index, features.shape[-3]).amin(dim=-3)      # scores that are not numbers: unlabelled
    return torch.where((alpha > label_alpha) & (first < features.shape[-3]), first, 255).to(torch.uint8)


def _sh_degree_of(sh):
    return {ops.gauss_sh_rows(d): d for d in range(1, ops.GAUSS_SH_MAX_DEGREE + 1)}[sh.shape[1]]


def _byte_colours(pts):
    """The colour words of packed points as (n, 3) fp32 in byte units."""
    word = pts[:, 3]
    return torch.stack([word & 0xff, (word >> 8) & 0xff, (word >> 16) & 0xff], dim=1).to(torch.float32)


def _bin(name, pts, cov, opacity, mats, cams, hw, ids, znear, zfar, max_entries):
    """Project, scan the tile counts, read the entry count E (the one host synchronisation) and refuse too many in `name`'s words, then
    keys, the stable sort and the tiles' ranges.  Returns a namespace of uv, conic, depth, rect, count, offsets, entries (E), values
    (sorted), order and ranges; the last three are None when E is 0."""
    uv, conic, depth, rect, count = ops.gauss_project(pts, cov, opacity, mats, cams, hw, ids=ids, znear=znear, zfar=zfar)
    ends = torch.cumsum(count.reshape(-1), 0, dtype=torch.int64)
    offsets = (ends - count.reshape(-1)).reshape(count.shape)
    entries = int(ends[-1].item())
    if entries >= 2 ** 31 or entries > int(max_entries):
        raise hip.MudgError(f"{name}: {entries} (tile, Gaussian) entries exceed max_entries = {int(max_entries)} (and must stay below 2^31): "
                            "thin the cloud, shrink the scale or draw fewer views per call")
    b = SimpleNamespace(uv=uv, conic=conic, depth=depth, rect=rect, count=count, offsets=offsets, entries=entries, values=None, order=None,
                        ranges=None)
    if entries:
        keys, values = ops.gauss_keys(depth, rect, count, offsets, entries, hw)
        keys, b.order = torch.sort(keys, stable=True)
        tx, ty = ops.gauss_tiles(*hw)
        b.values, b.ranges = values[b.order], ops.gauss_ranges(keys, mats.shape[0] * tx * ty)
    return b


def _blank(views, h, w, device):
    """(rgb, depth, alpha) of a call that drew nothing."""
    return (torch.zeros((views, 3, h, w), dtype=torch.float32, device=device), torch.zeros((views, h, w), dtype=torch.float32, device=device),
            torch.zeros((views, h, w), dtype=torch.float32, device=device))


def render(g: Gaussians, mats, cams, hw, *, znear=ZNEAR, zfar=ZFAR, max_entries=MAX_ENTRIES, stats=None, label_alpha=0.5):
    """Draw `g` into V views.  mats: (V, nmat, 12) fp32 on the GPU, row-major 3 x 4 matrices, mats[v][0] the world-to-camera matrix of
    view v and mats[v][1 + o] that matrix times object o's transform (zero for an object the view does not show); cams: (fx, fy, cx, cy)
    shared by the views; hw: (H, W).  Returns {"rgb": (V, 3, H, W) in [0, 1] on black, "depth": (V, H, W) alpha-weighted metres, "alpha":
    (V, H, W)}, fp32.  stats: a dict that receives "entries" (E, the (tile, Gaussian) pairs), "longest_tile" and the tensors "count",
    "rect", "values" (sorted) and "ranges"; a (V NT,) int32 tensor put under "walked" beforehand is filled with the entries each tile's
    workgroup staged (tools; not with harmonics).  With g.sh the colours of every (view, Gaussian) are evaluated first
    and the blend reads those; without, nothing changes.  One host synchronisation reads E (a second one, for the longest tile, only with stats); more than
    max_entries (or 2^31 - 1) entries are refused.  With g.features the blend is the one that also sums the scores: the
    dict gains "features" (V, F, H, W) fp32, the blended scores sum_entries feat[g] w (not divided by alpha), and "labels" (V, H, W)
    uint8 = label_image(features, alpha, label_alpha); rgb, depth and alpha keep their values up to the rounding of a colour byte to
    fp32, which is exact.  Without features the call, its launches and its dict are what they were."""
    if not isinstance(g, Gaussians):
        raise hip.MudgError("render: expected Gaussians")
    if not torch.is_tensor(mats) or not mats.is_cuda or mats.dtype != torch.float32 or mats.dim() != 3 or mats.shape[2] != 12:
        raise hip.MudgError("render: the matrices are a (V, nmat, 12) fp32 tensor on the GPU (there is no CPU path)")
    h, w = (int(v) for v in hw)
    views = mats.shape[0]
    tx, ty = ops.gauss_tiles(h, w)
    tiles = views * tx * ty
    if h <= 0 or w <= 0 or views == 0 or tiles >= 2 ** 31:
        raise hip.MudgError(f"render: {views} views of {h} x {w} ({tiles} tiles; V NT < 2^31)")
    if g.ids is None and mats.shape[1] != 1:
        raise hip.MudgError(f"render: {mats.shape[1]} matrices per view need Gaussians with ids")
    pts, dev = g.cloud.points, g.cloud.points.device
    b = _bin("render", pts, g.cov, g.opacity, mats.contiguous(), cams, (h, w), g.ids, znear, zfar, max_entries)
    if stats is not None:
        stats.update(entries=b.entries, longest_tile=0, count=b.count, rect=b.rect, values=None, ranges=None)
    if b.entries == 0:
        out = dict(zip(("rgb", "depth", "alpha"), _blank(views, h, w, dev)))
        if g.features is not None:
            out["features"] = torch.zeros((views, g.features.shape[1], h, w), dtype=torch.float32, device=dev)
            out["labels"] = label_image(out["features"], out["alpha"], label_alpha)
        return out
    walked = stats.get("walked") if stats is not None else None
    if g.features is not None:                                              # §29: the blend that also sums the scores
        if walked is not None:
            raise hip.MudgError("render: the blend that sums features does not count the entries it walked")
        colours = _byte_colours(pts) if g.sh is None else ops.gauss_sh_colour(pts, mats.contiguous(), b.count, g.colour, g.sh, ids=g.ids)
        rgb, out_depth, alpha, features, _ = ops.gauss_blend_feat(colours, g.features, b.uv, b.conic, b.depth, b.values, b.ranges, (h, w),
                                                                  with_state=False)
        if stats is not None:
            stats.update(longest_tile=int((b.ranges[:, 1] - b.ranges[:, 0]).max().item()), values=b.values, ranges=b.ranges)
        return {"rgb": rgb, "depth": out_depth, "alpha": alpha, "features": features, "labels": label_image(features, alpha, label_alpha)}
    if g.sh is not None:
        if walked is not None:
            raise hip.MudgError("render: the blend that reads per-view colours does not count the entries it walked")
        colours = ops.gauss_sh_colour(pts, mats.contiguous(), b.count, g.colour, g.sh, ids=g.ids)
        rgb, out_depth, alpha = ops.gauss_blend_views(colours, b.uv, b.conic, b.depth, b.values, b.ranges, (h, w))
    else:
        rgb, out_depth, alpha = ops.gauss_blend(pts, b.uv, b.conic, b.depth, b.values, b.ranges, (h, w), walked=walked)
    if stats is not None:
        stats.update(longest_tile=int((b.ranges[:, 1] - b.ranges[:, 0]).max().item()), values=b.values, ranges=b.ranges)
    return {"rgb": rgb, "depth": out_depth, "alpha": alpha}


def scene_matrices(objects: Optional[ObjectSet], w2c, frame):
    """(P, 4, 4) float64 world-to-camera of one frame -> (P, 1 + objects, 12) fp32 on the host: §12's table with the background first."""
    w2c = np.asarray(w2c, dtype=np.float64)
    table = w2c[:, None, :3, :]
    if objects is not None:
        table = np.concatenate([table, objects.matrices(w2c, frame)], axis=1)
    return np.ascontiguousarray(table.reshape(w2c.shape[0], -1, 12).astype(np.float32))


def render_scene(g: Gaussians, objects: Optional[ObjectSet], intr, c2w_frames, hw_native, hw_out, poses=None, *, frame_ids=None, shift=2.0,
                 znear=ZNEAR, zfar=ZFAR, max_entries=MAX_ENTRIES, stats=None, label_alpha=0.5):
    """Render T frames at P poses, with render_conditions' argument conventions: intr (3, 3) or (T, 3, 3) at hw_native, c2w_frames
    (T, 4, 4), poses None (the original pose and virtual_poses(c2w, shift): P = 3) or (T, P, 4, 4), frame_ids the scene's frame numbers
    for the objects' transforms.  `g` is Gaussians.from_scene's set (ids 0 and 1 + object): background and objects go through one sort
    and occlude one another per pixel.  Returns {"rgb": (P, T, 3, H, W), "depth", "alpha": (P, T, H, W)} fp32 and "rgb_u8": (P, T, H, W, 3)
    uint8 = floor(rgb 255 + 0.5) clamped.  stats: a list that receives one dict per frame.  With g.features also "features" (P, T, F, H, W)
    and "labels" (P, T, H, W) uint8, as render gives them."""
    if not isinstance(g, Gaussians) or (objects is not None and not isinstance(objects, ObjectSet)):
        raise hip.MudgError("render_scene: expected Gaussians and an ObjectSet (or None)")
    c2w_frames = np.asarray(c2w_frames, dtype=np.float64)
    T = c2w_frames.shape[0]
    if poses is None:
        poses = np.stack([np.stack(virtual_poses(c, shift, with_ori_pose=True)) for c in c2w_frames])
    poses = np.asarray(poses, dtype=np.float64)
    if c2w_frames.shape != (T, 4, 4) or poses.ndim != 4 or poses.shape[0] != T or poses.shape[2:] != (4, 4):
        raise hip.MudgError(f"render_scene: cameras {c2w_frames.shape} with poses {poses.shape}")
    frame_ids = list(range(T)) if frame_ids is None else [int(f) for f in frame_ids]
    intr = np.broadcast_to(np.asarray(intr, dtype=np.float64), (T, 3, 3))
    dev = g.cloud.points.device
    w2c = np.linalg.inv(poses)                                                            # host, float64, once per (frame, pose)
    mats = torch.from_numpy(np.stack([scene_matrices(objects, w2c[t], frame_ids[t]) for t in range(T)])).to(dev)      # one upload
    frames = []
    for t in range(T):
        st = {} if stats is not None else None
        frames.append(render(g, mats[t], scaled_intrinsics(intr[t], hw_native, hw_out).astype(np.float32), hw_out, znear=znear, zfar=zfar,
                             max_entries=max_entries, stats=st, label_alpha=label_alpha))
        if stats is not None:
            stats.append(st)
    out = {k: torch.stack([f[k] for f in frames], dim=1) for k in frames[0]}
    out["rgb_u8"] = torch.floor(out["rgb"] * 255.0 + 0.5).clamp_(0.0, 255.0).to(torch.uint8).permute(0, 1, 3, 4, 2).contiguous()
    return out


# ------------------------------------------------------------------------------------------------ fitting Gaussians to images (§24)
def _pack_xyz(xyz):
    """(n, 3) fp32 -> packed (n, 4) int32 points with a zero colour word: how positions travel to the kernels."""
    return torch.cat([xyz.detach().contiguous().view(torch.int32), torch.zeros((xyz.shape[0], 1), dtype=torch.int32, device=xyz.device)], dim=1)


class _Render(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, colour, cov, opacity, mats, cams, hw, ids, znear, zfar, max_entries, density=None, sh=None, sh_degree=None,
                features=None):
        if features is not None:                                            # §29: its own forward; backward tells by ctx.features
            return _Render._forward_features(ctx, xyz, colour, cov, opacity, mats, cams, hw, ids, znear, zfar, max_entries, density, sh,
                                             sh_degree, features)
        h, w = hw
        ctx.features = False
        ctx.density = density
        ctx.sh_degree = sh_degree if sh is not None else None
        pts = _pack_xyz(xyz)
        cov, opacity, colour = cov.detach().contiguous(), opacity.detach().contiguous(), colour.detach().contiguous()
        b = _bin("render_differentiable", pts, cov, opacity, mats, cams, (h, w), ids, znear, zfar, max_entries)
        ctx.meta = (cams, (h, w), ids, znear, zfar, b.entries)
        ctx.mats_shape = tuple(mats.shape)
        if b.entries == 0:
            ctx.save_for_backward(xyz, *(() if sh is None else (sh,)))
            return _blank(mats.shape[0], h, w, xyz.device)
        if sh is not None:                                                  # §27: one colour per (view, Gaussian)
            sh = sh.detach().contiguous()
            colours = ops.gauss_sh_colour(pts, mats, b.count, colour, sh, ids=ids, active=sh_degree)
            rgb, out_depth, alpha, state = ops.gauss_blend_train_views(colours, b.uv, b.conic, b.depth, b.values, b.ranges, (h, w))
            ctx.save_for_backward(pts, colour, cov, mats, b.uv, b.conic, b.depth, b.values, b.order, b.offsets, b.count, b.ranges, state, sh,
                                  colours)
            return rgb, out_depth, alpha
        rgb, out_depth, alpha, state = ops.gauss_blend_train(colour, b.uv, b.conic, b.depth, b.values, b.ranges, (h, w))
        ctx.save_for_backward(pts, colour, cov, mats, b.uv, b.conic, b.depth, b.values, b.order, b.offsets, b.count, b.ranges, state)
        return rgb, out_depth, alpha

    @staticmethod
    def _forward_features(ctx, xyz, colour, cov, opacity, mats, cams, hw, ids, znear, zfar, max_entries, density, sh, sh_degree, features):
        """forward with features (n, F): the same projection, binning and harmonics, then the blend that also sums the
        scores.  Returns (rgb, depth, alpha, feat)."""
        h, w = hw
        ctx.features = True
        ctx.density = density
        ctx.sh_degree = sh_degree if sh is not None else None
        pts = _pack_xyz(xyz)
        cov, opacity, colour = cov.detach().contiguous(), opacity.detach().contiguous(), colour.detach().contiguous()
        features = features.detach().contiguous()
        b = _bin("render_differentiable", pts, cov, opacity, mats, cams, (h, w), ids, znear, zfar, max_entries)
        ctx.meta = (cams, (h, w), ids, znear, zfar, b.entries)
        ctx.shapes = (tuple(mats.shape), tuple(features.shape), None if sh is None else tuple(sh.shape))
        if b.entries == 0:
            ctx.save_for_backward(xyz)
            return _blank(mats.shape[0], h, w, xyz.device) + (torch.zeros((mats.shape[0], features.shape[1], h, w), dtype=torch.float32,
                                                                          device=xyz.device),)
        colours = colour
        if sh is not None:                                                  # §27: one colour per (view, Gaussian)
            sh = sh.detach().contiguous()
            colours = ops.gauss_sh_colour(pts, mats, b.count, colour, sh, ids=ids, active=sh_degree)
        rgb, out_depth, alpha, feat, state = ops.gauss_blend_feat(colours, features, b.uv, b.conic, b.depth, b.values, b.ranges, (h, w))
        ctx.save_for_backward(pts, colour, cov, mats, b.uv, b.conic, b.depth, b.values, b.order, b.offsets, b.count, b.ranges, state, features,
                              feat, *(() if sh is None else (sh, colours)))
        return rgb, out_depth, alpha, feat

    @staticmethod
    def _backward_features(ctx, d_rgb, d_depth, d_alpha, d_feat):
        """backward of _forward_features: blend_bwd_feat, then project_bwd (and the harmonics', the matrices' and density's passes) on
        `partial` exactly as without features, and feat_bwd on `partial_feat`.  One gradient per argument of forward."""
        cams, hw, ids, znear, zfar, entries = ctx.meta
        mats_shape, feat_shape, sh_shape = ctx.shapes
        if entries == 0:                                                    # nothing was drawn: no launch
            n, dev = ctx.saved_tensors[0].shape[0], ctx.saved_tensors[0].device
            z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
            return (z(n, 3), z(n, 3), z(n, 6), z(n), z(*mats_shape) if ctx.needs_input_grad[4] else None) + (None,) * 7 + (
                None if sh_shape is None else z(*sh_shape), None, z(*feat_shape))
        pts, colour, cov, mats, uv, conic, depth, values, order, offsets, count, ranges, state, features, feat = ctx.saved_tensors[:15]
        sh, colours = ctx.saved_tensors[15:] if len(ctx.saved_tensors) > 15 else (None, colour)
        views, (h, w) = mats.shape[0], hw
        grad = lambda g, shape: torch.zeros(shape, dtype=torch.float32, device=pts.device) if g is None else g.to(torch.float32).contiguous()
        ups = (grad(d_rgb, (views, 3, h, w)), grad(d_depth, (views, h, w)), grad(d_alpha, (views, h, w)), grad(d_feat, tuple(feat.shape)))
        partial, partial_feat = ops.gauss_blend_bwd_feat(colours, features, uv, conic, depth, values, order, ranges, hw, state, feat, *ups)
        d_xyz, d_cov, d_opacity, d_colour = ops.gauss_project_bwd(pts, cov, mats, cams, hw, count, offsets, partial, ids=ids, znear=znear,
                                                                  zfar=zfar)
        d_features = ops.gauss_feat_bwd(count, offsets, partial_feat)
        d_mats = d_sh = None
        if ctx.needs_input_grad[4]:
            d_mats = ops.gauss_pose_bwd(pts, cov, mats, cams, hw, count, offsets, partial, ids=ids, znear=znear, zfar=zfar)
        if sh is not None:
            d_colour, d_sh, d_xyz_dir = ops.gauss_sh_bwd(pts, mats, count, offsets, partial, colour, sh, ids=ids, active=ctx.sh_degree)
            d_xyz = d_xyz + d_xyz_dir
            if d_mats is not None:
                d_mats = d_mats + ops.gauss_sh_pose_bwd(pts, mats, count, offsets, partial, colour, sh, ids=ids, active=ctx.sh_degree)
        if ctx.density is not None:
            ops.gauss_density_accumulate(partial, count, offsets, hw, ctx.density.grad_sum, ctx.density.seen)
        return (d_xyz, d_colour, d_cov, d_opacity, d_mats) + (None,) * 7 + (d_sh, None, d_features)

    @staticmethod
    def backward(ctx, d_rgb, d_depth, d_alpha, d_feat=None):
        if ctx.features:
            return _Render._backward_features(ctx, d_rgb, d_depth, d_alpha, d_feat)
        cams, hw, ids, znear, zfar, entries = ctx.meta
        if entries == 0:                                                    # nothing was drawn: no launch
            n, dev = ctx.saved_tensors[0].shape[0], ctx.saved_tensors[0].device
            z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
            tail = (torch.zeros_like(ctx.saved_tensors[1]), None) if len(ctx.saved_tensors) > 1 else ()
            d_mats = z(*ctx.mats_shape) if ctx.needs_input_grad[4] else None
            return (z(n, 3), z(n, 3), z(n, 6), z(n), d_mats) + (None,) * 7 + tail
        pts, colour, cov, mats, uv, conic, depth, values, order, offsets, count, ranges, state = ctx.saved_tensors[:13]
        sh, colours = ctx.saved_tensors[13:] if len(ctx.saved_tensors) > 13 else (None, None)
        views, (h, w) = mats.shape[0], hw
        grad = lambda g, shape: torch.zeros(shape, dtype=torch.float32, device=pts.device) if g is None else g.to(torch.float32).contiguous()
        ups = (grad(d_rgb, (views, 3, h, w)), grad(d_depth, (views, h, w)), grad(d_alpha, (views, h, w)))
        if sh is None:
            partial = ops.gauss_blend_bwd(colour, uv, conic, depth, values, order, ranges, hw, state, *ups)
        else:
            partial = ops.gauss_blend_bwd_views(colours, uv, conic, depth, values, order, ranges, hw, state, *ups)
        d_xyz, d_cov, d_opacity, d_colour = ops.gauss_project_bwd(pts, cov, mats, cams, hw, count, offsets, partial, ids=ids, znear=znear,
                                                                  zfar=zfar)
        tail = ()                                                           # as many gradients as forward was given arguments
        d_mats = None                                                       # §28: only when the matrices ask; else nothing is launched
        if ctx.needs_input_grad[4]:
            d_mats = ops.gauss_pose_bwd(pts, cov, mats, cams, hw, count, offsets, partial, ids=ids, znear=znear, zfar=zfar)
        if sh is not None:                                                  # §27: the colour columns again, through the harmonics
            d_colour, d_sh, d_xyz_dir = ops.gauss_sh_bwd(pts, mats, count, offsets, partial, colour, sh, ids=ids, active=ctx.sh_degree)
            d_xyz = d_xyz + d_xyz_dir
            tail = (d_sh, None)
            if d_mats is not None:
                d_mats = d_mats + ops.gauss_sh_pose_bwd(pts, mats, count, offsets, partial, colour, sh, ids=ids, active=ctx.sh_degree)
        if ctx.density is not None:                                         # §25: a second pass over the partials' columns 8 and 9
            ops.gauss_density_accumulate(partial, count, offsets, hw, ctx.density.grad_sum, ctx.density.seen)
        return (d_xyz, d_colour, d_cov, d_opacity, d_mats) + (None,) * 7 + tail


def render_differentiable(xyz, colour, cov, opacity, mats, cams, hw, *, ids=None, znear=ZNEAR, zfar=ZFAR, max_entries=MAX_ENTRIES,
                          density=None, sh=None, sh_degree=None, features=None):
    """`render` with gradients.  xyz (n, 3), colour (n, 3) in byte units (0 .. 255, not necessarily whole), cov (n, 6) and
    opacity (n,): fp32 on the GPU; mats, cams, hw and ids as `render` takes them.  Returns (rgb (V, 3, H, W), depth (V, H, W), alpha
    (V, H, W)); backward gives gradients for the first four arguments and, when `mats` requires one, for the matrices (DESIGN.md §28:
    d_mats (V, nmat, 12), the sum over every Gaussian that goes through a matrix in one fixed order, two more launches and with harmonics
    four; zeros when nothing was drawn); none for the camera.  With matrices that do not require a gradient nothing else happens: the same
    launches, the same bits.  One host synchronisation reads the entry count.  density: a DensityStats of n Gaussians; backward then adds every Gaussian's screen-space gradient norm and the
    views that counted it.  With None nothing else happens: the same launches, the same bits.  sh: (n, K - 1, 3) fp32
    coefficients in byte units of the harmonics of degrees 1 .. L, K = (L + 1)^2, L = 1, 2 or 3: `colour` is then the
    direction-independent term, every (view, Gaussian) gets max(0, colour + sum B_k(d) sh[k - 1]), backward also gives the gradient of sh
    and adds to xyz's what reaches it through the direction; sh_degree (default L) is the highest degree that takes part, and the
    coefficients above it get a zero gradient.  With sh None nothing else happens: the same launches, the same bits.  features: (n, F)
    fp32 class scores, 1 <= F <= ops.GAUSS_FEAT_MAX: the call then returns (rgb, depth, alpha, feat) with feat (V, F, H, W)
    the blended scores sum feat[g] w, rgb, depth and alpha keep their bits, and backward also gives the gradient of features; the
    gradients of everything else include what reaches them through feat.  With features None nothing else happens."""
    if features is not None:
        features = _on_gpu("render_differentiable: features", features, torch.float32,
                           (xyz.shape[0] if torch.is_tensor(xyz) else -1, _feature_width_of("render_differentiable", features)))
    n = xyz.shape[0] if torch.is_tensor(xyz) and xyz.dim() == 2 else -1
    if density is not None and (not isinstance(density, DensityStats) or density.grad_sum.shape[0] != n):
        raise hip.MudgError(f"render_differentiable: density is a DensityStats of {n} Gaussians")
    for name, t, shape in (("xyz", xyz, (n, 3)), ("colour", colour, (n, 3)), ("cov", cov, (n, 6)), ("opacity", opacity, (n,))):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != shape or n <= 0:
            got = f"{tuple(t.shape)} {t.dtype} on {t.device}" if torch.is_tensor(t) else type(t).__name__
            raise hip.MudgError(f"render_differentiable: {name} is an fp32 tensor of shape {shape} on the GPU (there is no CPU path), got {got}")
    if not torch.is_tensor(mats) or not mats.is_cuda or mats.dtype != torch.float32 or mats.dim() != 3 or mats.shape[2] != 12 or mats.shape[0] == 0:
        raise hip.MudgError("render_differentiable: the matrices are a (V, nmat, 12) fp32 tensor on the GPU (there is no CPU path)")
    if ids is not None:
        ids = _on_gpu("render_differentiable: ids", ids, torch.int32, (n,))
    elif mats.shape[1] != 1:
        raise hip.MudgError(f"render_differentiable: {mats.shape[1]} matrices per view need ids")
    h, w = (int(v) for v in hw)
    tx, ty = ops.gauss_tiles(h, w)
    if h <= 0 or w <= 0 or mats.shape[0] * tx * ty >= 2 ** 31:
        raise hip.MudgError(f"render_differentiable: {mats.shape[0]} views of {h} x {w} (V NT < 2^31)")
    args = (xyz, colour, cov, opacity, mats.contiguous(), tuple(float(c) for c in cams), (h, w), ids, float(znear), float(zfar), int(max_entries),
            density)
    if sh is None:
        if sh_degree is not None:
            raise hip.MudgError("render_differentiable: sh_degree comes with sh")
        return _Render.apply(*args) if features is None else _Render.apply(*args, None, None, features)
    sh = _on_gpu("render_differentiable: sh", sh, torch.float32, (n, _sh_rows_of("render_differentiable", sh), 3))
    degree = _sh_degree_of(sh)
    active = degree if sh_degree is None else int(sh_degree)
    if not 0 <= active <= degree:
        raise hip.MudgError(f"render_differentiable: sh_degree {active} of coefficients of degree {degree}")
    return _Render.apply(*args, sh, active) if features is None else _Render.apply(*args, sh, active, features)


# ------------------------------------------------------------------------------------------------ camera poses that move (§28)
SMALL_ANGLE = 1e-2               # below this |omega| Rodrigues' coefficients come from their series (the next term is below 1e-11 of them)


def rodrigues(omega):
    """(V, 3) rotation vectors -> (V, 3, 3) rotations exp([omega]x) = I + a K + b K^2 with a = sin(t) / t and b = (1 - cos(t)) / t^2, t =
    |omega|; below SMALL_ANGLE a and b come from their series in t^2, which are also differentiable at zero.  In torch, in omega's dtype."""
    t2 = (omega * omega).sum(1)
    small = t2 < SMALL_ANGLE ** 2
    t = torch.sqrt(torch.where(small, torch.ones_like(t2), t2))            # the branch not taken stays finite, and so does its gradient
    a = torch.where(small, 1 - t2 / 6 + t2 * t2 / 120, torch.sin(t) / t)
    b = torch.where(small, 0.5 - t2 / 24 + t2 * t2 / 720, (1 - torch.cos(t)) / (t * t))
    x, y, z = omega.unbind(1)
    zero = torch.zeros_like(x)
    k = torch.stack([zero, -z, y, z, zero, -x, -y, x, zero], dim=1).reshape(-1, 3, 3)
    eye = torch.eye(3, dtype=omega.dtype, device=omega.device)
    kk = omega[:, :, None] * omega[:, None, :] - t2[:, None, None] * eye    # K^2 = omega omega^T - |omega|^2 I: elementwise, no BLAS call
    return eye + a[:, None, None] * k + b[:, None, None] * kk


class CameraPoses:
    """A correction to the camera poses of `views` views that an optimiser moves: one leaf `twist` (V, 6) fp32 = (omega,
    tau) per view, zero at the start.  apply(mats) returns [R(omega_v) | tau_v] o mats[v][o] for every matrix o of view v: a rotation
    (Rodrigues' formula) and a translation applied on the left, in the camera's frame, so that a view's background and object matrices
    move together.  It is torch, so autograd carries render_differentiable's d_mats to `twist`.  The views in `fixed` get the identity
    and no gradient: with Gaussians that move too, one fixed view is the gauge.  The translation is not coupled to the rotation as a
    proper SE(3) exponential would couple it."""

    def __init__(self, views, *, fixed=(), device="cuda"):
        self.views = int(views)
        self.fixed = tuple(sorted({int(v) for v in fixed}))
        if self.views <= 0 or any(not 0 <= v < self.views for v in self.fixed):
            raise hip.MudgError(f"CameraPoses: {self.views} views with {self.fixed} fixed (views > 0, fixed views among them)")
        self.twist = torch.zeros((self.views, 6), dtype=torch.float32, device=device).requires_grad_(True)
        free = torch.ones((self.views, 1), dtype=torch.float32, device=device)
        free[list(self.fixed)] = 0.0
        self._free = free

    def __len__(self):
        return self.views

    def apply(self, mats, pick=None):
        """mats (P, nmat, 12) fp32 on the twist's device, view pick[k] (default: k, and then P = V) behind mats[k] -> the corrected (P,
        nmat, 12).  A zero twist returns the same values: R is exactly the identity and the products with its zeros vanish (the one bit
        that can change is the sign of a matrix entry that is -0.0, which comes back +0.0)."""
        if not torch.is_tensor(mats) or mats.dtype != torch.float32 or mats.dim() != 3 or mats.shape[2] != 12:
            raise hip.MudgError("CameraPoses.apply: the matrices are a (P, nmat, 12) fp32 tensor")
        twist = self.twist * self._free                                     # a fixed view: exactly zero, and no gradient
        if pick is not None:
            twist = twist[torch.as_tensor(pick, device=twist.device).long()]
        if twist.shape[0] != mats.shape[0]:
            raise hip.MudgError(f"CameraPoses.apply: {mats.shape[0]} views of matrices for {twist.shape[0]} poses")
        m = mats.reshape(mats.shape[0], mats.shape[1], 3, 4)
        out = (rodrigues(twist[:, :3])[:, None, :, :, None] * m[:, :, None, :, :]).sum(3)      # R m, elementwise: no BLAS, one order
        out = torch.cat([out[..., :3], out[..., 3:] + twist[:, None, 3:, None]], dim=-1)
        return out.reshape(mats.shape)

    def _corrections(self):
        """(V, 4, 4) float64 on the host."""
        with torch.no_grad():
            twist = (self.twist * self._free).detach().to("cpu", torch.float64)
            c = torch.eye(4, dtype=torch.float64).repeat(self.views, 1, 1)
            c[:, :3, :3] = rodrigues(twist[:, :3])
            c[:, :3, 3] = twist[:, 3:]
        return c.numpy()

    def world_to_camera(self, w2c):
        """(V, 4, 4) world-to-camera matrices -> the corrected ones, float64 on the host."""
        w2c = np.asarray(w2c, dtype=np.float64)
        if w2c.shape != (self.views, 4, 4):
            raise hip.MudgError(f"CameraPoses.world_to_camera: expected ({self.views}, 4, 4), got {w2c.shape}")
        return self._corrections() @ w2c

    def camera_to_world(self, c2w):
        """(V, 4, 4) camera-to-world matrices -> the corrected ones, float64 on the host: what render_scene takes as poses."""
        c2w = np.asarray(c2w, dtype=np.float64)
        if c2w.shape != (self.views, 4, 4):
            raise hip.MudgError(f"CameraPoses.camera_to_world: expected ({self.views}, 4, 4), got {c2w.shape}")
        return c2w @ np.linalg.inv(self._corrections())


PARAMETERS = ("xyz", "colour", "log_scale", "quat", "opacity_logit")
LEARNING_RATES = {"xyz": 2e-3, "colour": 2.0, "log_scale": 5e-3, "quat": 1e-3, "opacity_logit": 5e-2}      # metres, bytes, log metres, -, logits
LEARNING_RATES["sh"] = LEARNING_RATES["colour"] / 20       # bytes; 3DGS's ratio of the two rates, not tuned here
POSE_LEARNING_RATE = 1e-3                                 # radians and metres of a CameraPoses twist; not tuned here.  Beside
#                                                            LEARNING_RATES, not in it: that table is the model's leaves, and the twist is not one
CLASS_LEARNING_RATE = 0.05                                 # logits of GaussianModel.class_logits, opacity_logit's rate; not tuned here (DESIGN.md
#                                                            §29).  Beside LEARNING_RATES as the twist's rate is: the table's keys are pinned
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-15
MAX_SEED_OPACITY = 0.999                       # a seed opacity of 1 would be an infinite logit


class GaussianModel:
    """Gaussians as the tensors an optimiser moves: `xyz` (n, 3) metres, `colour` (n, 3) in byte units, `log_scale` (n, 3) (the logarithm
    of the per-axis standard deviation), `quat` (n, 4) = (w, x, y, z), `opacity_logit` (n,), all fp32 leaves on the GPU that require
    gradients, and `ids` (n,) int32 or None as Gaussians has them.  Covariance R exp(log_scale)^2 R^T and opacity sigmoid(opacity_logit)
    are torch expressions, so autograd carries the kernels' gradients to the parameters.  `sh` (n, K - 1, 3) fp32 in byte units or None:
    the coefficients of the harmonics of degrees 1 .. L, a sixth leaf when present; enable_sh(L) creates zeros.
    `class_logits` (n, F) fp32 or None: a row of class scores per Gaussian, one more leaf when present;
    enable_classes(F) creates zeros."""
    sh = class_logits = None

    def __init__(self, xyz, colour, log_scale, quat, opacity_logit, ids=None, sh=None, class_logits=None):
        n = xyz.shape[0] if torch.is_tensor(xyz) and xyz.dim() == 2 else -1
        shapes = {"xyz": (n, 3), "colour": (n, 3), "log_scale": (n, 3), "quat": (n, 4), "opacity_logit": (n,)}
        for name, t in zip(PARAMETERS, (xyz, colour, log_scale, quat, opacity_logit)):
            setattr(self, name, _on_gpu(f"GaussianModel: {name}", t, torch.float32, shapes[name]).detach().clone().requires_grad_(True))
        self.ids = None if ids is None else _on_gpu("GaussianModel: ids", ids, torch.int32, (n,))
        self.sh = None
        if sh is not None:
            self.sh = _on_gpu("GaussianModel: sh", sh, torch.float32, (n, _sh_rows_of("GaussianModel", sh), 3)).detach().clone().requires_grad_(True)
        self.class_logits = None
        if class_logits is not None:
            width = _feature_width_of("GaussianModel", class_logits)
            self.class_logits = _on_gpu("GaussianModel: class_logits", class_logits, torch.float32, (n, width)).detach().clone().requires_grad_(True)

    def __len__(self):
        return self.xyz.shape[0]

    @property
    def sh_degree(self):
        """L of the model's harmonics, 0 without."""
        return 0 if self.sh is None else _sh_degree_of(self.sh)

    def enable_sh(self, degree):
        """Give the model zero coefficients of degrees 1 .. `degree` (1, 2 or 3).  A model that has harmonics keeps them if the degree is
        theirs and refuses another."""
        degree = int(degree)
        if not 1 <= degree <= ops.GAUSS_SH_MAX_DEGREE:
            raise hip.MudgError(f"GaussianModel.enable_sh: degree {degree} (1, 2 or 3)")
        if self.sh is None:
            self.sh = torch.zeros((len(self), ops.gauss_sh_rows(degree), 3), dtype=torch.float32, device=self.xyz.device).requires_grad_(True)
        elif self.sh_degree != degree:
            raise hip.MudgError(f"GaussianModel.enable_sh: the model has harmonics of degree {self.sh_degree}, not {degree}")
        return self

    def enable_classes(self, classes):
        """Give the model zero class scores for `classes` classes (1 .. ops.GAUSS_FEAT_MAX).  A model that has scores keeps them if the
        number is theirs and refuses another."""
        classes = int(classes)
        if not 1 <= classes <= ops.GAUSS_FEAT_MAX:
            raise hip.MudgError(f"GaussianModel.enable_classes: {classes} classes (1 .. {ops.GAUSS_FEAT_MAX})")
        if self.class_logits is None:
            self.class_logits = torch.zeros((len(self), classes), dtype=torch.float32, device=self.xyz.device).requires_grad_(True)
        elif self.class_logits.shape[1] != classes:
            raise hip.MudgError(f"GaussianModel.enable_classes: the model has {self.class_logits.shape[1]} classes, not {classes}")
        return self

    def parameters(self):
        """The leaves by name: PARAMETERS, "sh" when the model has harmonics and "class_logits" when it has class scores."""
        more = (("sh",) if self.sh is not None else ()) + (("class_logits",) if self.class_logits is not None else ())
        return {name: getattr(self, name) for name in PARAMETERS + more}

    def covariance(self):
        return covariance_from_scales_rotations(torch.exp(self.log_scale), self.quat)

    def opacity(self):
        return torch.sigmoid(self.opacity_logit)

    @classmethod
    def from_cloud(cls, cloud: PointCloud, scale, opacity=0.9, ids=None):
        """Seeded as Gaussians.from_cloud seeds: isotropic `scale` (a number or (n,) tensor, metres), the cloud's positions and colours, the
        identity rotation.  opacity is clamped to [1 / 255, 0.999] so that its logit is finite."""
        if not isinstance(cloud, PointCloud) or not cloud.points.is_cuda:
            raise hip.MudgError("GaussianModel.from_cloud: the cloud is a PointCloud on the GPU (there is no CPU path)")
        n, dev = len(cloud), cloud.points.device
        pts = cloud.points
        xyz = pts[:, :3].contiguous().view(torch.float32)
        word = pts[:, 3]
        colour = torch.stack([word & 0xff, (word >> 8) & 0xff, (word >> 16) & 0xff], dim=1).to(torch.float32)
        s = Gaussians._per_point("scale", scale, n, dev)
        op = Gaussians._per_point("opacity", opacity, n, dev).clamp(1.0 / 255.0, MAX_SEED_OPACITY)
        quat = torch.zeros((n, 4), dtype=torch.float32, device=dev)
        quat[:, 0] = 1.0
        return cls(xyz, colour, torch.log(s)[:, None].expand(n, 3).contiguous(), quat, torch.log(op) - torch.log1p(-op), ids)

    @classmethod
    def from_scene(cls, background: PointCloud, objects: Optional[ObjectSet], scale, object_scale=None, opacity=0.9):
        """Gaussians.from_scene's set as a model: the background with id 0, every object's points with id 1 + object."""
        g = Gaussians.from_scene(background, objects, scale, object_scale, 1.0)
        s = torch.sqrt(g.cov[:, 0])
        return cls.from_cloud(g.cloud, s, opacity, g.ids)

    def gaussians(self) -> Gaussians:
        """The inference set: positions as they are, colours rounded (floor(c + 0.5)) and clamped to bytes, covariance and opacity
        evaluated.  render, render_scene and render_cloud_views' renderer draw it.  With harmonics the set also carries `sh` and, beside
        the byte word, `colour`, both unrounded: what the fit optimised is what is drawn."""
        with torch.no_grad():
            byte = torch.floor(self.colour + 0.5).clamp_(0.0, 255.0).to(torch.int32)
            word = byte[:, 0] | (byte[:, 1] << 8) | (byte[:, 2] << 16)
            pts = torch.cat([self.xyz.contiguous().view(torch.int32), word[:, None]], dim=1).contiguous()
            features = None if self.class_logits is None else self.class_logits.detach().clone()      # §29: the scores, as fitted
            if self.sh is None:
                return Gaussians(PointCloud(pts), self.covariance().contiguous(), self.opacity().contiguous(), self.ids, features=features)
            return Gaussians(PointCloud(pts), self.covariance().contiguous(), self.opacity().contiguous(), self.ids,
                             sh=self.sh.detach().clone(), colour=self.colour.detach().clone(), features=features)


# ------------------------------------------------------------------------------------------------ growing and pruning while fitting (§25)
class DensityStats:
    """What density control knows about n Gaussians: `grad_sum` (n,) fp32, the sum over the counted views of the norm of the loss's
    gradient with respect to the projected centre in [-1, 1] screen units, and `seen` (n,) int32, the number of those views.
    render_differentiable(..., density=stats) adds to both in its backward; reset() zeroes them (reset(n): for n Gaussians)."""

    def __init__(self, n, device):
        self.device = torch.device(device)
        if int(n) <= 0 or self.device.type != "cuda":
            raise hip.MudgError(f"DensityStats: {int(n)} Gaussians on {self.device} (n > 0, on the GPU: there is no CPU path)")
        self.reset(n)

    def __len__(self):
        return self.grad_sum.shape[0]

    def reset(self, n=None):
        n = len(self) if n is None else int(n)
        self.grad_sum = torch.zeros((n,), dtype=torch.float32, device=self.device)
        self.seen = torch.zeros((n,), dtype=torch.int32, device=self.device)


class DensityControl:
    """When and how `fit` grows and prunes.  Statistics are gathered in iterations start <= i < stop; after every `every`
    of them densify_and_prune runs: a Gaussian whose opacity is below min_opacity or whose largest scale exceeds max_scale (metres) goes; one
    whose mean gradient norm reaches grad_threshold is split in two along its longest axis if that scale exceeds split_scale (metres) and
    cloned if not.  split_shrink divides a child's scales; the children sit split_offset = sqrt(1 - 1 / split_shrink^2) standard
    deviations either side of the parent, which keeps the variance along that axis.  reset_every: inside the window, every so many iterations
    opacities above reset_opacity are set to it.  max_gaussians: a step that would exceed it only prunes.  grad_threshold, min_opacity,
    reset_opacity and split_shrink default to the 3DGS paper's values and are not tuned here; split_scale and max_scale have no default:
    the paper derives them from a scene extent this project does not define.  `history` receives one dict of counts per step."""

    def __init__(self, start, stop, every, grad_threshold=2e-4, *, split_scale, max_scale, min_opacity=0.005, reset_every=None,
                 reset_opacity=0.01, max_gaussians=None, split_shrink=1.6):
        self.start, self.stop, self.every = int(start), int(stop), int(every)
        self.grad_threshold, self.split_scale, self.max_scale = float(grad_threshold), float(split_scale), float(max_scale)
        self.min_opacity, self.reset_opacity, self.split_shrink = float(min_opacity), float(reset_opacity), float(split_shrink)
        self.reset_every = None if reset_every is None else int(reset_every)
        self.max_gaussians = None if max_gaussians is None else int(max_gaussians)
        numbers = (self.grad_threshold, self.split_scale, self.max_scale, self.min_opacity, self.reset_opacity, self.split_shrink)
        if (self.start < 0 or self.every <= 0 or any(v != v for v in numbers) or not 0.0 < self.reset_opacity < 1.0 or self.split_shrink <= 1.0
                or (self.reset_every is not None and self.reset_every <= 0) or (self.max_gaussians is not None and self.max_gaussians <= 0)):
            raise hip.MudgError("DensityControl: start >= 0, every > 0, thresholds that are numbers, 0 < reset_opacity < 1, split_shrink > 1, "
                                "reset_every and max_gaussians positive or None")
        self.split_offset = float(np.sqrt(1.0 - 1.0 / self.split_shrink ** 2))
        self.log_shrink = float(np.float32(np.log(self.split_shrink)))
        self.reset_logit = float(np.log(self.reset_opacity) - np.log1p(-self.reset_opacity))
        self.history = []

    def gathers(self, it):
        return self.start <= it < self.stop

    def densifies_after(self, it):
        return self.gathers(it) and (it + 1 - self.start) % self.every == 0

    def resets_after(self, it):
        return self.reset_every is not None and self.gathers(it) and (it + 1) % self.reset_every == 0


def density_rows(action, rows, value, m, v):
    """colour's rule of DESIGN.md §25 for any per-Gaussian tensor, in torch: `action` (n,) and `rows` (n,) int32 are the plan's; a kept
    Gaussian's row is copied with its moments, a cloned one's is copied with its moments and once more with zero moments, a split one's
    twice with zero moments, a pruned one's not at all; children are adjacent and the survivors keep their order.  Returns (value, m, v)
    with sum(rows) rows.  densify_and_prune moves `sh` with it: once per `every` iterations, so no kernel."""
    n = action.shape[0]
    rows = rows.to(torch.int64)
    src = torch.repeat_interleave(torch.arange(n, device=action.device), rows)
    start = torch.cumsum(rows, 0) - rows
    first = torch.arange(src.shape[0], device=action.device) == start[src]
    act = action[src]
    carries = (act == ops.GAUSS_KEEP) | ((act == ops.GAUSS_CLONE) & first)
    carries = carries.reshape((-1,) + (1,) * (value.dim() - 1))
    return value[src], torch.where(carries, m[src], torch.zeros_like(m[src])), torch.where(carries, v[src], torch.zeros_like(v[src]))


def densify_and_prune(model: GaussianModel, stats: DensityStats, moments: dict, control: DensityControl, *, grow=True) -> dict:
    """One step of density control: plan, exclusive sum, apply.  moments: {name: (m, v)}, the Adam moments of the model's
    parameters (a missing name: zeros).  Replaces the model's five leaves (fresh leaves that require gradients), its ids and the
    entries of `moments` (with harmonics also `sh` and its moments, by colour's rule: density_rows), and zeroes `stats` at the new size; survivors keep their order and a Gaussian's children are adjacent.  If growing
    would exceed control.max_gaussians the step is planned again without it.  A step that would leave no Gaussian raises MudgError and
    leaves everything as it was.  Two host synchronisations: the new count, and the counts returned: {"before", "after", "kept",
    "pruned", "cloned", "split", "grew"}."""
    if not isinstance(model, GaussianModel) or not isinstance(stats, DensityStats) or not isinstance(control, DensityControl):
        raise hip.MudgError("densify_and_prune: expected a GaussianModel, a DensityStats and a DensityControl")
    n = len(model)
    if len(stats) != n:
        raise hip.MudgError(f"densify_and_prune: statistics of {len(stats)} Gaussians for a model of {n}")
    with torch.no_grad():
        scale = torch.exp(model.log_scale.detach()).contiguous()
        rot = rotation_from_quaternions(model.quat.detach()).reshape(n, 9).contiguous()
        opacity = torch.sigmoid(model.opacity_logit.detach()).contiguous()
        for grew in ((True, False) if grow else (False,)):
            action, rows = ops.gauss_density_plan(stats.grad_sum, stats.seen, opacity, scale, grad_threshold=control.grad_threshold,
                                                  split_scale=control.split_scale, min_opacity=control.min_opacity,
                                                  max_scale=control.max_scale, grow=grew)
            ends = torch.cumsum(rows, 0, dtype=torch.int64)
            total = int(ends[-1].item())
            if not grew or control.max_gaussians is None or total <= control.max_gaussians:
                break
        if total <= 0:
            raise hip.MudgError(f"densify_and_prune: the step would prune all {n} Gaussians (min_opacity {control.min_opacity}, max_scale "
                                f"{control.max_scale})")
        tensors = []
        for name in PARAMETERS:
            p = getattr(model, name).detach()
            m, v = moments[name] if name in moments else (torch.zeros_like(p), torch.zeros_like(p))
            tensors += [p, m, v]
        outs, ids = ops.gauss_density_apply(action, ends - rows, total, scale, rot, tensors, split_offset=control.split_offset,
                                            log_shrink=control.log_shrink, ids=model.ids)
        kept, pruned, cloned, split = torch.bincount(action, minlength=4).tolist()
        if model.sh is not None:                                            # §27: the harmonics follow colour's rule
            p = model.sh.detach()
            m, v = moments["sh"] if "sh" in moments else (torch.zeros_like(p), torch.zeros_like(p))
            sh, sh_m, sh_v = density_rows(action, rows, p, m, v)
        if model.class_logits is not None:                                  # §29: and so do the class scores
            p = model.class_logits.detach()
            m, v = moments["class_logits"] if "class_logits" in moments else (torch.zeros_like(p), torch.zeros_like(p))
            logits, logits_m, logits_v = density_rows(action, rows, p, m, v)
    if model.class_logits is not None:
        model.class_logits = logits.contiguous().requires_grad_(True)
        moments["class_logits"] = (logits_m.contiguous(), logits_v.contiguous())
    if model.sh is not None:
        model.sh = sh.contiguous().requires_grad_(True)
        moments["sh"] = (sh_m.contiguous(), sh_v.contiguous())
    for k, name in enumerate(PARAMETERS):
        setattr(model, name, outs[3 * k].requires_grad_(True))
        moments[name] = (outs[3 * k + 1], outs[3 * k + 2])
    model.ids = ids
    stats.reset(total)
    return {"before": n, "after": total, "kept": kept, "pruned": pruned, "cloned": cloned, "split": split, "grew": grew}


def reset_opacity(model: GaussianModel, moments: dict, control: DensityControl):
    """Opacities above control.reset_opacity become it, and the opacity's two Adam moments start again at zero."""
    with torch.no_grad():
        model.opacity_logit.clamp_(max=control.reset_logit)
        for t in moments.get("opacity_logit", ()):
            t.zero_()


# ------------------------------------------------------------------------------------------------ the image loss with an SSIM term (§26)
class _ImageLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb, targets, depth, depth_targets, ssim_weight, depth_weight):
        maps, partial = ops.gauss_loss(rgb, targets, depth, depth_targets)
        totals = ops.gauss_loss_finish(partial, rgb.shape[2:], ssim_weight=ssim_weight, depth_weight=depth_weight)
        ctx.weights = (ssim_weight, depth_weight)
        ctx.has_depth = depth is not None
        ctx.save_for_backward(rgb, targets, maps, totals, *((depth, depth_targets) if depth is not None else ()))
        ctx.mark_non_differentiable(totals)
        return totals[0].clone(), totals

    @staticmethod
    def backward(ctx, up, _):
        rgb, targets, maps, totals = ctx.saved_tensors[:4]
        depth, depth_targets = ctx.saved_tensors[4:] if ctx.has_depth else (None, None)
        ssim_weight, depth_weight = ctx.weights
        up = up.to(torch.float32).reshape(1).contiguous()                   # stays on the device: the kernel reads it
        d_rgb, d_depth = ops.gauss_loss_bwd(rgb, targets, maps, totals, up, depth, depth_targets, ssim_weight=ssim_weight,
                                            depth_weight=depth_weight, want_depth=ctx.has_depth and ctx.needs_input_grad[2])
        return d_rgb, None, d_depth, None, None, None


def _image_loss_args(rgb, targets, depth, depth_targets, ssim_weight, depth_weight):
    if not torch.is_tensor(rgb) or rgb.dim() != 4 or rgb.shape[1] != 3 or rgb.numel() == 0:
        got = tuple(rgb.shape) if torch.is_tensor(rgb) else type(rgb).__name__
        raise hip.MudgError(f"image_loss: rgb is a (V, 3, H, W) fp32 tensor on the GPU (there is no CPU path), got {got}")
    v, _, h, w = rgb.shape
    rgb = _on_gpu("image_loss: rgb", rgb, torch.float32, (v, 3, h, w))
    targets = _on_gpu("image_loss: targets", targets, torch.float32, (v, 3, h, w))
    if (depth is None) != (depth_targets is None):
        raise hip.MudgError("image_loss: depth and depth_targets come together or not at all")
    if depth is not None:
        depth = _on_gpu("image_loss: depth", depth, torch.float32, (v, h, w))
        depth_targets = _on_gpu("image_loss: depth_targets", depth_targets, torch.float32, (v, h, w))
    ssim_weight, depth_weight = float(ssim_weight), float(depth_weight)
    if not 0.0 <= ssim_weight <= 1.0 or not (0.0 <= depth_weight < float("inf")):
        raise hip.MudgError(f"image_loss: ssim_weight {ssim_weight} lies in [0, 1] and depth_weight {depth_weight} is finite and not negative")
    return rgb, targets, depth, depth_targets, ssim_weight, depth_weight


def image_loss(rgb, targets, depth=None, depth_targets=None, *, ssim_weight=0.2, depth_weight=0.0):
    """(1 - ssim_weight) mean|rgb - targets| + ssim_weight (1 - mean SSIM) + depth_weight times the mean of |depth - depth_targets| over
    the pixels where depth_targets is positive (divisor at least 1): 3DGS's L1 + D-SSIM loss with fit's depth term, in three launches of
    csrc/gaussians_loss.hip.  rgb and targets (V, 3, H, W), depth and depth_targets (V, H, W) or both None: fp32 on the
    GPU.  Returns a 0-d fp32 loss whose backward gives gradients for rgb and depth, with no host synchronisation on either side.  SSIM here
    is the training convention: float images, the 11-tap window ops.SSIM_WINDOW / 65536 with zero padding so that every pixel has a value
    (images below 11 x 11 are legal), C1 = 0.01^2, C2 = 0.03^2, the mean over all V 3 H W values.  It is not metrics.psnr_ssim's
    convention, which takes uint8 frames, the valid region only and integer moments.  image_loss.terms gives the parts for logging."""
    return _ImageLoss.apply(*_image_loss_args(rgb, targets, depth, depth_targets, ssim_weight, depth_weight))[0]


def _image_loss_terms(rgb, targets, depth=None, depth_targets=None, *, ssim_weight=0.2, depth_weight=0.0):
    """The parts of image_loss as 0-d fp32 tensors on the GPU, without gradients: loss, l1 (mean |rgb - targets|), ssim (mean S), depth (the
    masked mean absolute depth difference) and depth_count (the pixels it is over, int32)."""
    rgb, targets, depth, depth_targets, ssim_weight, depth_weight = _image_loss_args(rgb, targets, depth, depth_targets, ssim_weight, depth_weight)
    with torch.no_grad():
        _, partial = ops.gauss_loss(rgb.detach(), targets.detach(), None if depth is None else depth.detach(), depth_targets)
        totals = ops.gauss_loss_finish(partial, rgb.shape[2:], ssim_weight=ssim_weight, depth_weight=depth_weight)
    return dict(loss=totals[0], l1=totals[1], ssim=totals[2], depth=totals[3], depth_count=totals.view(torch.int32)[5])


image_loss.terms = _image_loss_terms


# ------------------------------------------------------------------------------------------------ the class loss (§29)
UNLABELLED = 255                 # a label image's "no class here"; any label >= F is unlabelled


class _ClassLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, labels, weight):
        maps, partial = ops.gauss_class_loss(feat, labels)
        totals = ops.gauss_class_loss_finish(partial, feat.shape[0], feat.shape[2:], weight=weight)
        ctx.weight = weight
        ctx.save_for_backward(maps, totals)
        ctx.mark_non_differentiable(totals)
        return totals[3].clone(), totals

    @staticmethod
    def backward(ctx, up, _):
        maps, totals = ctx.saved_tensors
        up = up.to(torch.float32).reshape(1).contiguous()                   # stays on the device: the kernel reads it
        return ops.gauss_class_loss_bwd(maps, totals, up, weight=ctx.weight), None, None


def _class_labels(name, labels, shape):
    """uint8 labels as they are; int64 labels converted, values outside 0 .. 254 becoming UNLABELLED."""
    if torch.is_tensor(labels) and labels.dtype == torch.int64:
        labels = torch.where((labels >= 0) & (labels < UNLABELLED), labels, UNLABELLED).to(torch.uint8)
    return _on_gpu(f"{name}: labels", labels, torch.uint8, shape)


def class_loss(feat, labels, *, weight=1.0):
    """weight times the mean over the labelled pixels of the softmax cross-entropy of feat (V, F, H, W) fp32, the blended class scores of
    render_differentiable(..., features=), against labels (V, H, W) uint8 (or int64, converted): a pixel is labelled iff its label is
    below F, so UNLABELLED = 255 marks sky and holes; with no labelled pixel the loss and its gradient are zero.  Three launches of
    csrc/gaussians_feat.hip, no host synchronisation on either side.  Returns a 0-d fp32 loss whose backward gives the
    gradient of feat.  class_loss.terms gives the sum and the count."""
    return _ClassLoss.apply(*_class_loss_args(feat, labels, weight))[0]


def _class_loss_args(feat, labels, weight):
    if not torch.is_tensor(feat) or feat.dim() != 4 or feat.numel() == 0 or not 1 <= feat.shape[1] <= ops.GAUSS_FEAT_MAX:
        got = tuple(feat.shape) if torch.is_tensor(feat) else type(feat).__name__
        raise hip.MudgError(f"class_loss: feat is a (V, 1 .. {ops.GAUSS_FEAT_MAX}, H, W) fp32 tensor on the GPU (there is no CPU path), got {got}")
    v, f, h, w = feat.shape
    weight = float(weight)
    if not 0.0 <= weight < float("inf"):
        raise hip.MudgError(f"class_loss: weight {weight} is finite and not negative")
    return _on_gpu("class_loss: feat", feat, torch.float32, (v, f, h, w)), _class_labels("class_loss", labels, (v, h, w)), weight


def _class_loss_terms(feat, labels, *, weight=1.0):
    """The parts of class_loss as 0-d tensors on the GPU, without gradients: loss, sum (of the labelled pixels' losses) and count (int32)."""
    feat, labels, weight = _class_loss_args(feat, labels, weight)
    with torch.no_grad():
        totals = ops.gauss_class_loss_finish(ops.gauss_class_loss(feat.detach(), labels)[1], feat.shape[0], feat.shape[2:], weight=weight)
    return dict(loss=totals[3], sum=totals[0], count=totals.view(torch.int32)[1])


class_loss.terms = _class_loss_terms


def fit(model: GaussianModel, targets, mats, cams, hw, *, iters, lr=None, views_per_step=None, depth_targets=None, depth_weight=0.0,
        trainable=PARAMETERS, znear=ZNEAR, zfar=ZFAR, max_entries=MAX_ENTRIES, density=None, ssim_weight=0.0, sh_degree=0, sh_raise_every=None,
        poses=None, label_targets=None, class_weight=0.0, classes=None):
    """Optimise `model` in place against targets (V, 3, H, W) fp32 in [0, 1] seen through mats (V, nmat, 12) and cams.
    Iteration i renders the views_per_step (default: all) views (i views_per_step + k) mod V, takes the mean absolute difference of rgb,
    adds depth_weight times the mean absolute depth difference over the pixels where depth_targets (V, H, W) is positive, and takes one
    Adam step (betas 0.9 / 0.999, eps 1e-15, no weight decay) through train.kernels.adamw_multi_: one launch for all tensors that share
    a learning rate.  lr: a dict over PARAMETERS (missing names take LEARNING_RATES) or None; trainable: the names that move.
    density: a DensityControl or None.  With one, iterations inside its window gather statistics, densify_and_prune runs
    after every `every` of them (the model's leaves, the moments and the optimiser's tables are rebuilt, the Adam step count keeps running),
    opacities are reset every reset_every iterations, and each step's counts are appended to density.history; with None, or an empty
    window, the fit is the fixed-set fit bit for bit.  ssim_weight: with 0 (the default) the loss is the torch expression above, bit for
    bit what it was before the keyword existed; with a value in (0, 1] the iteration's loss is image_loss:
    (1 - ssim_weight) times the mean absolute difference plus ssim_weight (1 - mean SSIM) plus the same depth term, forward and backward
    in the kernels of csrc/gaussians_loss.hip; 3DGS fits with 0.2.  sh_degree: L = 1, 2 or 3 fits view-dependent colour:
    the model gets zero coefficients of degrees 1 .. L if it has none (one that has them must have that degree), "sh" moves with the
    other parameters at its own rate LEARNING_RATES["sh"] (lr may name it), density control carries its rows and moments as it carries
    colour's, and model.gaussians() hands the coefficients to render.  The active degree starts at 0 and rises by one every
    sh_raise_every iterations until it is L; None: all degrees from the first iteration.  With sh_degree=0 (the default) nothing changes,
    bit for bit, and a model that has harmonics is refused.  poses: a CameraPoses of V views or None.  With one, every
    iteration renders through poses.apply(mats[pick], pick), the matrices' gradient reaches poses.twist, and the twist is one more tensor
    of the Adam step at POSE_LEARNING_RATE (lr may name "pose"; the rate is not tuned); trainable=() is then allowed and is pure
    registration against fixed Gaussians; density control does not touch the twist.  With None nothing changes, bit for bit.
    label_targets: (V, H, W) uint8 (or int64) label images, 255 or any value >= classes unlabelled, with class_weight > 0:
    the model gets zero class scores for `classes` classes (default: metrics.CLASSES) if it has none, every iteration renders them
    with the colours and adds class_loss(feat, label_targets[pick], weight=class_weight), "class_logits" moves at
    CLASS_LEARNING_RATE (lr may name it), density control carries its rows and moments as it carries sh's, and
    model.gaussians() hands the scores to render.  With label_targets None or class_weight 0 nothing changes, bit for bit.  Returns the
    loss of every iteration."""
    from .train import kernels as K
    if not isinstance(model, GaussianModel):
        raise hip.MudgError("fit: expected a GaussianModel")
    if density is not None and not isinstance(density, DensityControl):
        raise hip.MudgError("fit: density is a DensityControl or None")
    ssim_weight = float(ssim_weight)
    if not 0.0 <= ssim_weight <= 1.0:
        raise hip.MudgError(f"fit: ssim_weight {ssim_weight} lies in [0, 1]")
    h, w = (int(v) for v in hw)
    if not torch.is_tensor(mats) or not mats.is_cuda or mats.dtype != torch.float32 or mats.dim() != 3 or mats.shape[2] != 12 or mats.shape[0] == 0:
        raise hip.MudgError("fit: the matrices are a (V, nmat, 12) fp32 tensor on the GPU (there is no CPU path)")
    views = mats.shape[0]
    targets = _on_gpu("fit: targets", targets, torch.float32, (views, 3, h, w))
    if depth_targets is not None:
        depth_targets = _on_gpu("fit: depth_targets", depth_targets, torch.float32, (views, h, w))
    sh_degree = int(sh_degree)
    if not 0 <= sh_degree <= ops.GAUSS_SH_MAX_DEGREE or (sh_raise_every is not None and int(sh_raise_every) <= 0):
        raise hip.MudgError(f"fit: sh_degree {sh_degree} is 0 .. {ops.GAUSS_SH_MAX_DEGREE} and sh_raise_every {sh_raise_every} positive or None")
    if model.sh_degree != sh_degree and (sh_degree == 0 or model.sh is not None):
        raise hip.MudgError(f"fit: sh_degree {sh_degree} for a model with harmonics of degree {model.sh_degree}")
    if poses is not None and (not isinstance(poses, CameraPoses) or len(poses) != views or poses.twist.device != mats.device):
        raise hip.MudgError(f"fit: poses is a CameraPoses of {views} views on the matrices' device, or None")
    class_weight = float(class_weight)
    if not 0.0 <= class_weight < float("inf"):
        raise hip.MudgError(f"fit: class_weight {class_weight} is finite and not negative")
    with_classes = label_targets is not None and class_weight > 0.0
    if with_classes:
        from .metrics import CLASSES
        label_targets = _class_labels("fit", label_targets, (views, h, w))
        model.enable_classes(CLASSES if classes is None else classes)
    known = PARAMETERS + ("sh", "pose", "class_logits")
    rates = {**LEARNING_RATES, "pose": POSE_LEARNING_RATE, "class_logits": CLASS_LEARNING_RATE, **(lr or {})}
    names = [n for n in PARAMETERS if n in tuple(trainable)]
    if (not names and poses is None) or "pose" in tuple(trainable) or set(trainable) - set(known) or set(rates) - set(known) or int(iters) < 0:
        raise hip.MudgError(f"fit: trainable and lr name parameters among {PARAMETERS}, got {tuple(trainable)} and {tuple(rates)}")
    if sh_degree:
        model.enable_sh(sh_degree)
        names.append("sh")
    if with_classes:
        names.append("class_logits")
    if poses is not None:
        names.append("pose")
    leaf = lambda n: poses.twist if n == "pose" else getattr(model, n)
    per = views if views_per_step is None else int(views_per_step)
    if not 1 <= per <= views:
        raise hip.MudgError(f"fit: {per} views per step of {views}")
    moments = {}

    def bind():
        """The optimiser's view of the model's leaves: again after every step that replaced them (their addresses changed)."""
        params = [leaf(n) for n in names]
        grads = [torch.zeros_like(p) for p in params]
        for n, p in zip(names, params):
            if n not in moments:
                moments[n] = (torch.zeros_like(p), torch.zeros_like(p))
        tables = {}
        for rate in sorted({float(rates[n]) for n in names}):
            rows = [(p.detach(), g, *moments[n]) for n, p, g in zip(names, params, grads) if float(rates[n]) == rate]
            tables[rate] = K.chunk_table(rows)
        return params, grads, tables

    params, grads, tables = bind()
    stats = None
    losses = []
    for it in range(int(iters)):
        gathers = density is not None and density.gathers(it)
        if gathers and stats is None:
            stats = DensityStats(len(model), mats.device)
        pick = torch.tensor([(it * per + k) % views for k in range(per)], device=mats.device)
        harmonics = {}
        if sh_degree:                                                       # §27: the active degree rises by one every sh_raise_every
            harmonics = dict(sh=model.sh, sh_degree=sh_degree if sh_raise_every is None else min(sh_degree, it // int(sh_raise_every)))
        if with_classes:                                                    # §29: the scores ride the same walk
            harmonics["features"] = model.class_logits
        rgb, depth, _, *scores = render_differentiable(model.xyz, model.colour, model.covariance(), model.opacity(),
                                                       mats[pick] if poses is None else poses.apply(mats[pick], pick), cams, (h, w),
                                                       ids=model.ids, znear=znear, zfar=zfar, max_entries=max_entries,
                                                       density=stats if gathers else None, **harmonics)
        with_depth = depth_targets is not None and bool(depth_weight)
        if ssim_weight:                                                     # §26: the loss and its backward in csrc/gaussians_loss.hip
            loss = image_loss(rgb, targets[pick], depth if with_depth else None, depth_targets[pick] if with_depth else None,
                              ssim_weight=ssim_weight, depth_weight=float(depth_weight) if with_depth else 0.0)
        else:
            loss = (rgb - targets[pick]).abs().mean()
            if with_depth:
                want = depth_targets[pick]
                seen = want > 0
                loss = loss + float(depth_weight) * ((depth - want).abs() * seen).sum() / seen.sum().clamp(min=1)
        if with_classes:
            loss = loss + class_loss(scores[0], label_targets[pick], weight=class_weight)
        for g, d in zip(grads, torch.autograd.grad(loss, params, allow_unused=True)):
            g.zero_() if d is None else g.copy_(d)
        for rate, (table, chunks) in tables.items():
            K.adamw_multi_(table, chunks, lr=rate, betas=ADAM_BETAS, eps=ADAM_EPS, weight_decay=0.0, step=it + 1)
        losses.append(loss.detach())
        if gathers and density.densifies_after(it):
            density.history.append(dict(densify_and_prune(model, stats, moments, density), iteration=it))
            params, grads, tables = bind()
        if gathers and density.resets_after(it):
            reset_opacity(model, moments, density)
    return torch.stack(losses).tolist() if losses else []
