"""The tensor-level part of MuDG's inference driver (reference: virtual_render/virtual_pose_render.py —
get_latent_z 54-59, image_guided_synthesis 62-147), with the same argument order, cond / uc dict layout and return
value, on the MI355X path.  The reference file also holds the Waymo frame loaders, PNG/NPY writers and the CLI; those
are host I/O outside the denoising path (SURVEY.md §8(f) rank 3 covers this call sequence, the sliding-window loop with its
autoregressive colour re-feed — `synthesize_windows` below, fed with tensors by the caller — and the per-modality
post-processing in `virtual_render/eval_tools.py`).

Conditioning encoders: `model.embedder` (CLIP image tower) and `model.cond_stage_model` (CLIP text tower) are whatever
modules the config instantiated — they are third-party and not part of this path; `model.image_proj_model` (the
Resampler) and both VAE encodes run on the HIP kernels.
"""
import torch

from lvdm.models.samplers.ddim import DDIMSampler
from lvdm.models.samplers.ddim_multiplecond import DDIMSampler as DDIMSampler_multicond


def get_latent_z(model, videos):
    """(b, c, t, h, w) pixels -> (b, 4, t, h/8, w/8) scaled latents, frame-wise through the VAE encoder."""
    b, c, t, h, w = videos.shape
    frames = videos.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w)
    z = model.encode_first_stage(frames)
    return z.reshape(b, t, *z.shape[1:]).permute(0, 2, 1, 3, 4)


class GuidanceInputs:
    """Everything the guided sampler needs for one batch of modality streams, built once: the conditional dict, the
    unconditional dict (empty prompt + tokens of an all-zero image) and — for three-way guidance — the image-only dict
    (empty prompt + the real image tokens).  All of them share the channel-concat conditioning (the VAE latents of the
    sparse colour and sparse depth renderings); the dict layout is the one LatentDiffusion.apply_model / DiffusionWrapper
    consume ({"c_crossattn": [tokens], "c_concat": [latents]}, virtual_pose_render.py:75-112 in the reference)."""

    def __init__(self, model, prompts, sparse_x, sparse_depth, guided, three_way):
        self.batch = sparse_x.shape[0]
        key_frame = sparse_x[:, :, 0]                                      # the conditioning image of every stream
        tokens = lambda image: model.image_proj_model(model.embedder(image))          # CLIP tower -> Resampler, (b, 16 t, d)
        text = model.get_learned_conditioning(prompts)                     # (b, 77, d)
        image_tokens = tokens(key_frame)
        self.hybrid = model.model.conditioning_key == "hybrid"
        self.concat = None
        self.sparse_z = None
        if self.hybrid:
            self.sparse_z = get_latent_z(model, sparse_x)
            self.concat = torch.cat([self.sparse_z, get_latent_z(model, sparse_depth)], dim=1)
        self.cond = self._entry(text, image_tokens)
        self.uncond = self.image_only = None
        if guided:
            blank = model.get_learned_conditioning(self.batch * [""]) if model.uncond_type == "empty_seq" else torch.zeros_like(text)
            self.uncond = self._entry(blank, tokens(torch.zeros_like(key_frame)))
            if three_way:
                self.image_only = self._entry(blank, image_tokens)

    def _entry(self, text, image_tokens):
        entry = {"c_crossattn": [torch.cat([text, image_tokens], dim=1)]}
        if self.hybrid:
            entry["c_concat"] = [self.concat]
        return entry


def image_guided_synthesis(model, prompts, sparse_x, sparse_depth, class_label, noise_shape, n_samples=1, ddim_steps=50,
                           ddim_eta=1., unconditional_guidance_scale=1.0, cfg_img=None, fs=None, text_input=False,
                           multiple_cond_cfg=False, timestep_spacing="uniform", guidance_rescale=0.0, **kwargs):
    """Same signature and return value as the reference's function (virtual_pose_render.py:62-147): guided DDIM sampling
    of `n_samples` variants for a batch of modality streams, decoded to pixels, (batch, variants, c, t, h, w)."""
    batch = sparse_x.shape[0]
    guided = unconditional_guidance_scale != 1.0
    three_way = bool(multiple_cond_cfg) and cfg_img != 1.0
    inputs = GuidanceInputs(model, prompts if text_input else [""] * batch, sparse_x, sparse_depth, guided, three_way)
    sampler = (DDIMSampler_multicond if multiple_cond_cfg else DDIMSampler)(model)
    extra = dict(kwargs, unconditional_conditioning_img_nonetext=inputs.image_only)
    if inputs.hybrid:
        extra.update(sparse_x=inputs.sparse_z, class_label=class_label)
    frame_rate = torch.tensor([fs] * batch, dtype=torch.long, device=model.device)
    variants = []
    for _ in range(n_samples):
        latents, _ = sampler.sample(S=ddim_steps, conditioning=inputs.cond, batch_size=batch, shape=noise_shape[1:],
                                    verbose=False, unconditional_guidance_scale=unconditional_guidance_scale,
                                    unconditional_conditioning=inputs.uncond, eta=ddim_eta, cfg_img=cfg_img, mask=None, x0=None,
                                    fs=frame_rate, timestep_spacing=timestep_spacing, guidance_rescale=guidance_rescale, **extra)
        variants.append(model.decode_first_stage(latents))
    return torch.stack(variants).permute(1, 0, 2, 3, 4, 5)


def synthesize_windows(model, windows, noise_shape, video_length=16, **synthesis_kwargs):
    """The sliding-window loop of run_inference_multi (virtual_pose_render.py:222-355) on tensors.

    `windows` yields, per window, a dict with the three modality streams in the reference's order (colour, depth,
    semantic): "sparse" (3, c, t, h, w), "dense" (3, c, t, h, w), "sparse_depth" (3, c, t, h, w), "class_label" (3, 1) —
    what get_color_frames / get_depth_frames / get_semantic_frames / get_sparse_depth load from disk there.  Consecutive
    windows overlap by half (the index advances by video_length // 2, :247); before a window is synthesised, the colour
    stream's first video_length // 2 sparse frames are replaced by the last video_length // 2 frames generated for the
    previous window (:269-274) and its frame 0 by the dense frame 0 (:275).  Returns the list of clamped samples
    (3, n_samples, c, t, h, w) per window, as batch_samples after :243."""
    half = video_length // 2
    carry = None
    results = []
    for win in windows:
        sparse = win["sparse"].clone()
        if carry is not None:
            sparse[0, :, 0:half] = carry[:, 0:half]
            sparse[0, :, 0] = win["dense"][0, :, 0]
        dev = model.device
        samples = image_guided_synthesis(model, [""] * sparse.shape[0], sparse.to(dev), win["sparse_depth"].to(dev),
                                         win["class_label"].to(dev), noise_shape, **synthesis_kwargs)
        samples = torch.clamp(samples.float(), -1., 1.)
        results.append(samples)
        for nn in range(samples.shape[0]):
            if int(win["class_label"][nn, 0]) == 0:                        # the colour stream re-feeds itself
                carry = samples[nn, 0, :, half:video_length].to(sparse.device)      # (c, half, h, w)
    return results


def render_windows(scene, dense_frames, pose, video_length=16):
    """Yields the window dicts `synthesize_windows` consumes, with the sparse conditions rendered on the GPU from the scene's point
    clouds (mudg_amd/render.py) instead of read from pre-rendered files.

    scene: mudg_amd.render.Scene (background cloud, objects, intrinsics, per-frame c2w, native size).  dense_frames:
    (3, c, frames, h, w) in [-1, 1], the colour / depth / semantic dense streams of the whole clip; decoding camera files is host I/O
    and stays with the caller; (h, w) is the size rendered at.  pose: 0, 1 or 2 — the original camera or the reference's virtual pose 1
    (2 m to the left) or 2 (2 m to the right), its move_id — or a (4, 4) camera-from-virtual-camera matrix applied to every frame's
    c2w.  As in the reference's loaders (virtual_render/data_tools.py:40, 61, 153, 212) the three streams carry the same sparse
    colour and sparse depth, class labels 0, 500 and 1, and sparse frame 0 of every stream is that stream's dense frame 0; windows
    advance by video_length // 2 (virtual_pose_render.py:246 there)."""
    import numpy as np
    from mudg_amd import render
    c2w = np.asarray(scene.c2w, dtype=np.float64)
    frames = c2w.shape[0]
    if dense_frames.dim() != 5 or dense_frames.shape[0] != 3 or dense_frames.shape[2] != frames:
        raise ValueError(f"render_windows: dense_frames {tuple(dense_frames.shape)} for three streams of {frames} frames")
    if np.ndim(pose) == 0:
        cams = np.stack([render.virtual_poses(c, with_ori_pose=True)[int(pose)] for c in c2w])
    else:
        cams = c2w @ np.asarray(pose, dtype=np.float64)
    intr = np.broadcast_to(np.asarray(scene.intr, dtype=np.float64), (frames, 3, 3))
    labels = torch.tensor(render.CLASS_LABELS, dtype=torch.long)[:, None]
    for start in range(0, frames - video_length + 1, max(video_length // 2, 1)):
        sel = slice(start, start + video_length)
        cond = render.render_conditions(scene.background, scene.objects, intr[sel], c2w[sel], scene.hw_native, dense_frames.shape[-2:],
                                        poses=cams[sel, None], frame_ids=range(start, start + video_length))
        dense = dense_frames[:, :, sel]
        sparse = cond["sparse_frames"].repeat(3, 1, 1, 1, 1)
        sparse[:, :, 0] = dense[:, :, 0].to(sparse.device)
        yield {"sparse": sparse, "dense": dense, "sparse_depth": cond["sparse_depth"].repeat(3, 1, 1, 1, 1), "class_label": labels}


def window_outputs(samples, window_conditions, variant=0):
    """What a window's three generated streams are worth downstream, all on the GPU.

    samples: one entry of synthesize_windows' result, (3, n_samples, c, t, h, w) in [-1, 1], the colour, depth and semantic streams;
    window_conditions: mudg_amd.render.render_conditions(..., return_images=True) of that window's frames at the pose it was generated
    at (one pose: "depth" is (1, t, h, w) metres, 0 where no LiDAR return landed).  Returns a dict:
      "color"            (t, h, w, 3) uint8     the colour stream, as save_virtual_color_results writes it (eval_tools.py:22-28)
      "semantic_labels"  (t, h, w) int64        the nearest of the 19 class colours (eval_tools.py:309-347)
      "semantic"         (t, h, w, 3) uint8     the labels' own colours
      "depth"            (t, h, w) fp32 metres  the depth stream fitted per frame to the rendered LiDAR depth, 100 m on sky (class 10),
                                                clipped to [0, 100] (data_process/depthlab_tools.py:67-87, 114-136)
      "depth_vis"        (t, h, w, 3) uint8     its Spectral picture (eval_tools.py:137-306)
      "coef", "fitted"   (t, 2) float64, (t,) uint8   the fitted line per frame; fitted = 0 where a frame had too few returns and the
                                                stream's own 100 m scale was kept
    variant: which of the n_samples to take."""
    from mudg_amd import depth, ops
    if samples.dim() != 6 or samples.shape[0] != 3 or samples.shape[2] != 3:
        raise ValueError(f"window_outputs: samples {tuple(samples.shape)}, expected (3, n_samples, 3, t, h, w)")
    lidar = window_conditions["depth"]
    if lidar.dim() != 4 or lidar.shape[0] != 1 or tuple(lidar.shape[1:]) != (samples.shape[3],) + tuple(samples.shape[4:]):
        raise ValueError(f"window_outputs: rendered depth {tuple(lidar.shape)} for samples {tuple(samples.shape)} (one pose, the window's frames)")
    u8 = ops.frames_to_uint8(samples[:, variant])                             # (3, t, h, w, 3)
    vis, labels = zip(*(ops.semantic_nearest(frame.permute(2, 0, 1)) for frame in u8[2]))
    labels = torch.stack(labels)
    metric = depth.metric_depth(u8[1], lidar[0], labels, visualise=True)
    return {"color": u8[0], "semantic_labels": labels, "semantic": torch.stack(vis).permute(0, 2, 3, 1).contiguous(),
            "depth": metric["depth"], "depth_vis": metric["vis"], "coef": metric["coef"], "fitted": metric["fitted"]}


def fuse_window_outputs(outputs_by_pose, scene, frame_ids, poses, **rule):
    """One window generated at several poses -> one filtered cloud and the window's consistency scores.

    outputs_by_pose: window_outputs' dicts of the same window, one per entry of poses; scene: the mudg_amd.render.Scene the window was
    rendered from; frame_ids: the window's frames, positions in the scene's cameras; poses: as render_windows takes them, 0 / 1 / 2 or
    a (4, 4) camera-from-virtual-camera matrix each.  The views are stacked pose by pose, a view's time id is its frame and its
    witnesses are mudg_amd.depth.default_witnesses' — the other poses of its frame, then every view within `reach` frames — so a pixel
    tagged as a movable class is compared across poses of its own frame only.  **rule: mudg_amd.depth.fuse_views' keywords
    (voxel_size, r, min_agree, max_violate, rel_tol, abs_tol, ..., and either reach or witnesses, not both).  Returns (mudg_amd.render.PointCloud of the kept pixels,
    mudg_amd.metrics.view_consistency's scores with the device result under "result")."""
    import numpy as np
    from mudg_amd import depth, metrics, render
    frame_ids = [int(f) for f in frame_ids]
    if len(outputs_by_pose) != len(poses) or not poses or not frame_ids:
        raise ValueError(f"fuse_window_outputs: {len(outputs_by_pose)} outputs for {len(poses)} poses and {len(frame_ids)} frames")
    c2w = np.asarray(scene.c2w, dtype=np.float64)[frame_ids]
    intr = np.broadcast_to(np.asarray(scene.intr, dtype=np.float64), (np.asarray(scene.c2w).shape[0], 3, 3))[frame_ids]
    cams = [np.stack([render.virtual_poses(c, with_ori_pose=True)[int(p)] for c in c2w]) if np.ndim(p) == 0 else c2w @ np.asarray(p, dtype=np.float64)
            for p in poses]
    for out in outputs_by_pose:
        if out["depth"].shape[0] != len(frame_ids):
            raise ValueError(f"fuse_window_outputs: outputs of {out['depth'].shape[0]} frames for frames {frame_ids}")
    stack = lambda name: torch.cat([out[name] for out in outputs_by_pose])
    times = np.tile(np.asarray(frame_ids, dtype=np.int32), len(poses))
    pose_ids = np.repeat(np.arange(len(poses), dtype=np.int32), len(frame_ids))
    if "witnesses" not in rule:                                               # given lists go through as they are (reach beside them is refused)
        rule["witnesses"] = depth.default_witnesses(times, pose_ids, rule.pop("reach", 2))
    cloud, result = depth.fuse_views(stack("depth"), stack("color"), np.concatenate([intr] * len(poses)), np.concatenate(cams), scene.hw_native,
                                     stack("semantic_labels"), times=times, **rule)
    scores = metrics.view_consistency(result)
    scores["result"] = result
    return cloud, scores


def render_cloud_views(cloud, scene, frame_ids, pose, hw_out, scale, *, fitted=None, **kw):
    """A cloud drawn as isotropic 3D Gaussians at a pose (mudg_amd/gaussians.py): what a fused cloud looks like in pixels.

    cloud: fuse_window_outputs' cloud, or any mudg_amd.render.PointCloud in world coordinates (the moving objects are whatever the cloud
    holds of them: no ObjectSet is drawn); scene: the mudg_amd.render.Scene whose cameras are used; frame_ids: positions in the scene's
    cameras; pose: as render_windows takes it, 0 / 1 / 2 or a (4, 4) camera-from-virtual-camera matrix; hw_out: the size rendered at;
    scale: the Gaussians' standard deviation in metres, a number or one per point (for a cloud thinned at voxel_size a multiple of it).
    **kw: opacity (default 1) and mudg_amd.gaussians.render_scene's keywords (znear, zfar, max_entries, stats).  Returns (frames (t, h,
    w, 3) uint8, alpha (t, h, w) fp32): the frames on black, ready for mudg_amd.metrics.psnr_ssim against the scene's own frames.
    fitted: fit_cloud_views' mudg_amd.gaussians.Gaussians, drawn in place of the seeded cloud (cloud, scale and opacity are then unused and
    cloud may be None).  If they carry class scores the call returns (frames, alpha, labels (t, h, w) int64): the argmax
    of the blended scores, 255 where alpha <= label_alpha (a keyword, default 0.5), ready for mudg_amd.metrics.segmentation_scores."""
    import numpy as np
    from mudg_amd import gaussians, render
    frame_ids = [int(f) for f in frame_ids]
    if not frame_ids:
        raise ValueError("render_cloud_views: no frames")
    c2w = np.asarray(scene.c2w, dtype=np.float64)[frame_ids]
    intr = np.broadcast_to(np.asarray(scene.intr, dtype=np.float64), (np.asarray(scene.c2w).shape[0], 3, 3))[frame_ids]
    if np.ndim(pose) == 0:
        cams = np.stack([render.virtual_poses(c, with_ori_pose=True)[int(pose)] for c in c2w])
    else:
        cams = c2w @ np.asarray(pose, dtype=np.float64)
    if fitted is not None and not isinstance(fitted, gaussians.Gaussians):
        raise ValueError("render_cloud_views: fitted is fit_cloud_views' Gaussians")
    g = gaussians.Gaussians.from_cloud(cloud, scale, kw.pop("opacity", 1.0)) if fitted is None else fitted
    out = gaussians.render_scene(g, None, intr, c2w, scene.hw_native, hw_out, poses=cams[:, None], frame_ids=frame_ids, **kw)
    if "labels" in out:
        return out["rgb_u8"][0], out["alpha"][0], out["labels"][0].to(torch.int64)
    return out["rgb_u8"][0], out["alpha"][0]


def fit_cloud_views(cloud, scene, frame_ids, frames_u8, pose, hw_out, scale, *, labels=None, **kw):
    """The companion of render_cloud_views: a cloud seeded as isotropic Gaussians and optimised against a window's frames
    (mudg_amd.gaussians.fit).

    cloud, scene, frame_ids, pose, hw_out and scale as render_cloud_views takes them; frames_u8: (t, h, w, 3) uint8 on the GPU at hw_out,
    what the cameras saw (or the model generated) at those frames and that pose.  The frames share one camera: per-frame intrinsics
    that differ are refused.  **kw: opacity (the seed, default 0.9), history (a list that receives the loss of every iteration) and
    fit's keywords (iters, default 200; lr, views_per_step, depth_targets, depth_weight, trainable, znear, zfar, max_entries; density, a
    mudg_amd.gaussians.DensityControl: the fit then clones, splits and prunes Gaussians, DESIGN.md §25, so that the result need not have
    the cloud's size; ssim_weight, default 0: above it the fit minimises mudg_amd.gaussians.image_loss, L1 + D-SSIM, DESIGN.md §26, and
    3DGS's value is 0.2; sh_degree, default 0, and sh_raise_every: with L = 1, 2 or 3 every Gaussian also learns spherical harmonics of
    degrees 1 .. L, DESIGN.md §27, so that its colour may differ between the poses a fit sees; poses, default None: a mudg_amd.gaussians.CameraPoses
    of t views, one per frame, whose twist the fit then moves with the Gaussians, DESIGN.md §28, because a scenario's camera poses and
    tracked boxes carry calibration and tracking error; its world_to_camera gives the corrected cameras afterwards).  Returns the fitted
    mudg_amd.gaussians.Gaussians, which render, render_scene and the renderer of render_cloud_views draw; one fitted with harmonics
    carries them, and its colour then depends on the pose it is drawn at.  labels: (t, h, w) int64 or uint8 label images at hw_out, such
    as window_outputs' "semantic_labels", with the keyword class_weight > 0 (and classes, default mudg_amd.metrics.CLASSES): every
    Gaussian then also learns a row of class scores by softmax cross-entropy, values outside 0 .. classes - 1 are
    unlabelled, and the returned Gaussians carry the scores, which render_cloud_views(..., fitted=) draws as a label image at any pose.
    The scores start at zero: they are not seeded from lifted labels."""
    import numpy as np
    import torch
    from mudg_amd import gaussians, hip, render
    frame_ids = [int(f) for f in frame_ids]
    if not frame_ids:
        raise ValueError("fit_cloud_views: no frames")
    h, w = (int(v) for v in hw_out)
    if not torch.is_tensor(frames_u8) or not frames_u8.is_cuda or frames_u8.dtype != torch.uint8 or tuple(frames_u8.shape) != (len(frame_ids), h, w, 3):
        raise hip.MudgError(f"fit_cloud_views: the frames are a ({len(frame_ids)}, {h}, {w}, 3) uint8 tensor on the GPU (there is no CPU path)")
    c2w = np.asarray(scene.c2w, dtype=np.float64)[frame_ids]
    intr = np.broadcast_to(np.asarray(scene.intr, dtype=np.float64), (np.asarray(scene.c2w).shape[0], 3, 3))[frame_ids]
    if not (intr == intr[0]).all():
        raise hip.MudgError("fit_cloud_views: the frames of one fit share one camera")
    if np.ndim(pose) == 0:
        cams = np.stack([render.virtual_poses(c, with_ori_pose=True)[int(pose)] for c in c2w])
    else:
        cams = c2w @ np.asarray(pose, dtype=np.float64)
    mats = torch.from_numpy(gaussians.scene_matrices(None, np.linalg.inv(cams), 0)).to(frames_u8.device)
    k = render.scaled_intrinsics(intr[0], scene.hw_native, (h, w)).astype(np.float32)
    model = gaussians.GaussianModel.from_cloud(cloud, scale, kw.pop("opacity", 0.9))
    history = kw.pop("history", None)
    kw.setdefault("iters", 200)
    targets = frames_u8.permute(0, 3, 1, 2).to(torch.float32).div_(255.0).contiguous()
    if labels is not None:
        kw["label_targets"] = labels
    losses = gaussians.fit(model, targets, mats, k, (h, w), **kw)
    if history is not None:
        history.extend(losses)
    return model.gaussians()
