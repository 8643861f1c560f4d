"""Writing what log_images returns to disk, at the drop-in boundary (reference: utils/save_video.py, prepare_to_log 120-136 and
log_local 62-118).

Same names and signatures.  What differs: the tensors stay on the device between the two calls, and the frame sheet of an entry —
the samples stacked along the height (make_grid(nrow=1, padding=0)), a one-channel entry repeated to three, clamp to [-1, 1],
(x + 1) / 2, * 255, truncation — is ONE kernel launch (mudg_log_sheet) whose uint8 result is all that crosses to the host, a quarter
of the bytes; the clamp prepare_to_log applies is folded into that launch.  CPU tensors take the same expressions in torch.
Captions go to .txt and image sheets to .jpg through PIL, as in the reference.  Video sheets are written with torchvision.io
(h264, crf 10, as the reference) when it is importable and as the .npy of the (t, n*h, w, 3) uint8 array otherwise: no encoder and
no TensorBoard writer are part of this package."""
import os

import numpy as np
import torch


class PreparedLogs(dict):
    """What prepare_to_log returns: the entries, and whether the clamp to [-1, 1] is still to be applied to the device tensors
    among them (log_local does it inside the sheet kernel)."""
    clamp = False


def prepare_to_log(batch_logs, max_images=100000, clamp=True):
    if batch_logs is None:
        return None
    out = PreparedLogs()
    for key in batch_logs:
        value = batch_logs[key]
        n = value.shape[0] if hasattr(value, "shape") else len(value)
        value = value[:min(n, max_images)]
        # in batch_logs: images <batched tensor> & caption <text list>
        if isinstance(value, torch.Tensor):
            value = value.detach()
            if clamp and not value.is_cuda:
                value = torch.clamp(value.float(), -1., 1.)
        out[key] = value
    out.clamp = bool(clamp)
    return out


def _sheet(value, clamp, rescale):
    """(n, c, t, h, w) -> (t, n*h, w, 3) uint8 numpy array; (n, c, h, w) -> (n*h, w, 3)."""
    if value.is_cuda:
        from mudg_amd import ops
        return ops.log_sheet(value, clamp=clamp, rescale=rescale).cpu().numpy()
    five = value.dim() == 5
    grid = value.float() if five else value.float().unsqueeze(2)
    if clamp:
        grid = torch.clamp(grid, -1., 1.)
    n, c, t, h, w = grid.shape
    grid = grid.permute(2, 1, 0, 3, 4).reshape(t, c, n * h, w).expand(t, 3, n * h, w)
    if rescale:
        grid = (grid + 1.0) / 2.0
    grid = (grid * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
    return grid if five else grid[0]


def _video_writer():
    try:
        from torchvision.io import write_video
        return write_video
    except Exception:
        return None


def log_local(batch_logs, save_dir, filename, save_fps=10, rescale=True):
    """save images and videos from images dict"""
    if batch_logs is None:
        return None
    clamp = bool(getattr(batch_logs, "clamp", False))
    os.makedirs(save_dir, exist_ok=True)
    for key in batch_logs:
        value = batch_logs[key]
        if isinstance(value, list) and value and isinstance(value[0], str):
            # a batch of captions
            with open(os.path.join(save_dir, "%s-%s.txt" % (key, filename)), "w") as f:
                for i, txt in enumerate(value):
                    f.write(f"idx={i}, txt={txt}\n")
        elif isinstance(value, torch.Tensor) and value.dim() in (4, 5):
            if value.shape[1] != 1 and value.shape[1] != 3:          # only grayscale or rgb entries
                continue
            grid = _sheet(value, clamp, rescale)
            if value.dim() == 4:
                from PIL import Image
                Image.fromarray(grid).save(os.path.join(save_dir, "%s-%s.jpg" % (key, filename)))
                continue
            write_video = _video_writer()
            if write_video is not None:
                write_video(os.path.join(save_dir, "%s-%s.mp4" % (key, filename)), torch.from_numpy(grid), fps=save_fps, video_codec="h264",
                            options={"crf": "10"})
            else:
                np.save(os.path.join(save_dir, "%s-%s.npy" % (key, filename)), grid)
