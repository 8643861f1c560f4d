"""Frames in: camera images, depth maps and label maps resized into the clips the model takes, on the GPU.

The reference prepares the dense streams on the host, per frame and stream, with cv2.resize, then stacks, permutes and normalises
(lvdm/data/waymo_data.py:55-412, virtual_render/data_tools.py:7-215, data_process/tools/semantic_tools.py:45-73).  Here the frames of a
scene are resident on the GPU (the camera images are uploaded for the point clouds anyway) and one kernel per stream (csrc/frames.hip)
goes from them to the (3, T, h, w) tensor in [-1, 1]; the sparse pair comes from the renderer (render.py).  DESIGN.md §16 states the
resize rules: they are this project's definition, written after the reference's calls, and have not been compared with cv2 itself.
The fourth modality, surface normals (waymo_data.py:194-265), has its own kernel (csrc/normals.hip) and its maps come from
files or from depth.normals_from_depth.  Reading and decoding files stays with the caller.  There is no CPU path: frames that are not
on the GPU are an error.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import hip, ops, render

CAPTION = "A photo a of driving scene."                            # waymo_data.py:60, spelled as there
FPS = 10
CLASS_LABEL = {"color": 0, "semantic": 1, "depth": 500}            # waymo_data.py:125, 189, 337: the streams of an inference window
MODALITY_LABEL = {**CLASS_LABEL, "normal": 1000}                   # the four dense modalities of training; waymo_data.py:262
LABEL_SETS = (("color", "semantic", "depth"), ("color", "semantic", "normal"))  # the two triples get_label draws from (waymo_data.py:350-360)
STREAM_ORDER = ("color", "depth", "semantic")                      # data_tools.py: the streams of an inference window


def stream_from_images(images_u8, hw_out, out=None, return_u8=False, **place):
    """(T, H0, W0, 3) uint8 camera images -> the colour stream (3, T, h, w): 8-bit linear resize, (v / 255 - 0.5) * 2.  out / slab /
    frame0 place it inside a larger tensor (ops.dense_stream); return_u8 also gives the resized frames (T, h, w, 3)."""
    return ops.dense_stream("color", images_u8, hw_out, out, return_u8=return_u8, **place)


def stream_from_labels(labels_u8, hw_out, out=None, return_u8=False, **place):
    """(T, H0, W0) uint8 class ids -> the semantic stream (3, T, h, w): the 21 class colours looked up on the taps of the 8-bit linear
    resize (an id above 20 is black), then the colour normalisation."""
    return ops.dense_stream("semantic", labels_u8, hw_out, out, return_u8=return_u8, **place)


def stream_from_depth(depth_f32, hw_out, out=None, **place):
    """(T, H0, W0) fp32 metres -> the depth stream (3, T, h, w): fp32 linear resize, (clamp(d, 0, 100) / 100 - 0.5) * 2 in all channels."""
    return ops.dense_stream("depth", depth_f32, hw_out, out, **place)


def stream_from_normals(normals_f32, hw_out, out=None, **place):
    """(T, H0, W0, 3) fp32 normal maps "already in [-1, 1]" -> the normal stream (3, T, h, w): fp32 linear resize of every channel and
    nothing else — no normalisation, no renormalisation to unit length (waymo_data.py:227-229, 253-254)."""
    return ops.normal_stream(normals_f32, hw_out, out, **place)


_STREAM = {"color": stream_from_images, "semantic": stream_from_labels, "depth": stream_from_depth, "normal": stream_from_normals}


def dense_streams(images, depth, labels, hw_out):
    """The `dense_frames` argument of render_windows, (3, 3, T, h, w): the colour, depth and semantic streams of a clip.  A stream whose
    source is None is the colour stream (every loader of data_tools.py reads the colour images)."""
    h, w = (int(v) for v in hw_out)
    out = torch.empty((3, 3, images.shape[0], h, w), dtype=torch.float32, device=images.device)
    sources = {"color": images, "depth": depth, "semantic": labels}
    for slab, name in enumerate(STREAM_ORDER):
        kind = name if sources[name] is not None else "color"
        _STREAM[kind](sources[kind], (h, w), out, slab=slab)
    return out


class SceneFrames:
    """One camera's frames of a scene, resident on the GPU: images (F, H0, W0, 3) uint8 and, optionally, depth (F, H0, W0) fp32 metres,
    labels (F, H0, W0) uint8 class ids and normals (F, H0, W0, 3) fp32 (loaded maps, or depth.normals_from_depth's)."""

    def __init__(self, images, depth=None, labels=None, normals=None):
        self.images = ops._splat_tensor("SceneFrames: images", images, torch.uint8)
        if images.dim() != 4 or images.shape[3] != 3 or images.numel() == 0:
            raise hip.MudgError(f"SceneFrames: images are (frames, H, W, 3) uint8, got {tuple(images.shape)}")
        shape = tuple(images.shape[:3])
        self.depth = None if depth is None else ops._splat_tensor("SceneFrames: depth", depth, torch.float32, shape)
        self.labels = None if labels is None else ops._splat_tensor("SceneFrames: labels", labels, torch.uint8, shape)
        self.normals = None if normals is None else ops._splat_tensor("SceneFrames: normals", normals, torch.float32, shape + (3,))

    @classmethod
    def from_loader(cls, load_image, camera, frames: Sequence[int], load_depth=None, load_labels=None, load_normals=None, device="cuda"):
        """load_image(camera, frame) -> (H0, W0, 3) uint8 is the callable Scene.from_scenario takes; load_depth, load_labels and
        load_normals have the same form and return (H0, W0) fp32 metres, (H0, W0) uint8 class ids and (H0, W0, 3) fp32 normals.  One
        upload per stream."""
        def stack(load, dtype):
            return torch.from_numpy(np.stack([np.asarray(load(camera, int(f)), dtype=dtype) for f in frames])).to(device)
        return cls(stack(load_image, np.uint8), None if load_depth is None else stack(load_depth, np.float32),
                   None if load_labels is None else stack(load_labels, np.uint8),
                   None if load_normals is None else stack(load_normals, np.float32))

    def __len__(self):
        return self.images.shape[0]

    def source(self, label):
        src = {"color": self.images, "depth": self.depth, "semantic": self.labels, "normal": self.normals}[label]
        if src is None:
            raise hip.MudgError(f"SceneFrames: the scene holds no {label} frames")
        return src


def choose_label(train_labels, u):
    """get_label (waymo_data.py:342-362) for the draw u in [0, 1): one label: that label; two: the first if u > 0.5, else the second;
    three: [0, 0.25) depth — normal if the three hold it —, [0.25, 0.5) semantic, [0.5, 1) colour — closed on the left, where the
    reference returns None at 0.25, 0.5.  Four labels are an error: the reference returns None there and fails on it."""
    if len(train_labels) == 1:
        return train_labels[0]
    if len(train_labels) == 2:
        return train_labels[0] if u > 0.5 else train_labels[1]
    if len(train_labels) != 3:
        raise hip.MudgError(f"choose_label: {len(train_labels)} labels (one, two, or three of which the draw is defined)")
    return ("normal" if "normal" in train_labels else "depth") if u < 0.25 else ("semantic" if u < 0.5 else "color")


class SceneClips:
    """The training items of one scene and camera, what the reference's Waymo.__getitem__ yields: item i is frames i .. i + T - 1 (the
    reference centres a T-frame window on each image: the same set of windows).  The dense stream is resized from the resident frames,
    the sparse pair is rendered at the original pose, and sparse frame 0 is the colour stream's frame 0 whatever the label
    (waymo_data.py:100, 164, 311).  Everything stays on the device."""

    def __init__(self, scene: render.Scene, scene_frames: SceneFrames, hw_out, video_length=16, train_labels=("color", "semantic", "depth"),
                 generator=None):
        self.scene, self.frames = scene, scene_frames
        self.hw_out = tuple(int(v) for v in hw_out)
        self.video_length = int(video_length)
        self.train_labels = tuple(train_labels)
        for label in self.train_labels:
            self._check_label(label)
        if not 1 <= len(self.train_labels) <= 3 or (len(self.train_labels) == 3 and set(self.train_labels) not in map(set, LABEL_SETS)):
            raise hip.MudgError(f"SceneClips: train_labels {self.train_labels} (one or two of {tuple(MODALITY_LABEL)}, or one of the triples "
                                f"{' | '.join(map(str, LABEL_SETS))})")
        self.c2w = np.asarray(scene.c2w, dtype=np.float64)
        if self.c2w.shape[0] != len(scene_frames) or self.video_length < 1 or self.video_length > len(scene_frames):
            raise hip.MudgError(f"SceneClips: {len(scene_frames)} resident frames, {self.c2w.shape[0]} camera poses, clips of {self.video_length}")
        self.intr = np.broadcast_to(np.asarray(scene.intr, dtype=np.float64), (self.c2w.shape[0], 3, 3))
        self.generator = np.random.default_rng() if generator is None else generator
        self._class_label = {k: torch.tensor([v], device=scene_frames.images.device) for k, v in MODALITY_LABEL.items()}      # uploaded once

    def _check_label(self, label):
        if label not in MODALITY_LABEL:
            raise hip.MudgError(f"SceneClips: label {label!r} ({' | '.join(MODALITY_LABEL)})")
        if label == "normal" and self.frames.normals is None:                # unlike depth and labels, refused before any item is made
            raise hip.MudgError("SceneClips: the 'normal' stream needs normal maps and the scene's frames hold none (SceneFrames(..., normals=))")

    def __len__(self):
        return len(self.frames) - self.video_length + 1

    def __getitem__(self, index, label: Optional[str] = None):
        if label is None:
            label = choose_label(self.train_labels, self.generator.random())
        self._check_label(label)
        index = int(index)
        if not 0 <= index < len(self):
            raise IndexError(f"SceneClips: item {index} of {len(self)}")
        sel = slice(index, index + self.video_length)
        dense = _STREAM[label](self.frames.source(label)[sel], self.hw_out)
        cond = render.render_conditions(self.scene.background, self.scene.objects, self.intr[sel], self.c2w[sel], self.scene.hw_native,
                                        self.hw_out, poses=self.c2w[sel, None], frame_ids=range(sel.start, sel.stop))
        stream_from_images(self.frames.images[index:index + 1], self.hw_out, cond["sparse_frames"], slab=0, frame0=0)
        return {"dense_frames": dense, "sparse_frames": cond["sparse_frames"][0], "sparse_depth": cond["sparse_depth"][0], "caption": CAPTION,
                "fps": FPS, "class_label": self._class_label[label].clone()}

    @staticmethod
    def collate(items):
        """Items -> the batch get_batch_input / shared_step take: tensors stacked on the device, the captions as a list."""
        if not items:
            raise hip.MudgError("SceneClips.collate: no items")
        dev = items[0]["dense_frames"].device
        batch = {k: torch.stack([it[k] for it in items]) for k in ("dense_frames", "sparse_frames", "sparse_depth", "class_label")}
        batch["caption"] = [it["caption"] for it in items]
        if len({it["fps"] for it in items}) != 1:
            raise hip.MudgError("SceneClips.collate: the items' frame rates differ")
        batch["fps"] = torch.full((len(items),), items[0]["fps"], dtype=torch.long, device=dev)
        return batch
