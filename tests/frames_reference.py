"""The frame-resize rules of DESIGN.md §16 as a plain numpy definition (CPU), written independently of mudg_amd/frames.py and of the
table code in mudg_amd/ops.py: the tests hold the kernels of csrc/frames.hip to this file bit for bit, and tests/test_frames_cpu.py holds
this file to things known without it.  The rules are the project's own (they restate the reference's cv2.resize calls and have not been
compared with cv2)."""
import numpy as np

F32 = np.float32

# data_process/tools/semantic_tools.py:47-69 (data: the 21 class colours)
PALETTE = np.array([[255, 120, 50], [255, 192, 203], [255, 255, 0], [0, 150, 245], [0, 255, 255], [255, 127, 0], [255, 0, 0],
                    [255, 240, 150], [135, 60, 0], [160, 32, 240], [255, 0, 255], [139, 137, 137], [75, 0, 75], [150, 240, 80],
                    [230, 230, 250], [0, 175, 0], [0, 255, 127], [222, 155, 161], [140, 62, 69], [227, 164, 30], [0, 128, 0]], dtype=np.uint8)


def linear_coords(n_src, n_dst):
    """Per output sample: first tap, second tap, fraction (fp32).  One sample at a time, as the rule reads."""
    scale = np.float64(n_src) / np.float64(n_dst)
    first, second, frac = [], [], []
    for d in range(n_dst):
        f = F32((np.float64(d) + 0.5) * scale - 0.5)
        s = int(np.floor(f))
        f = F32(f - F32(s))
        if s < 0:
            s, f = 0, F32(0)
        if s >= n_src - 1:
            s, f = n_src - 1, F32(0)
        first.append(s)
        second.append(min(s + 1, n_src - 1))
        frac.append(f)
    return np.array(first), np.array(second), np.array(frac, dtype=F32)


def nearest_coords(n_src, n_dst):
    scale = np.float64(n_src) / np.float64(n_dst)
    return np.array([min(int(np.floor(np.float64(d) * scale)), n_src - 1) for d in range(n_dst)])


def coefficients(frac):
    """fraction -> (coefficient of the first tap, of the second), int16, half to even; products and the subtraction in fp32."""
    c1 = np.rint(frac * F32(2048)).astype(np.int16)
    c0 = np.rint((F32(1) - frac) * F32(2048)).astype(np.int16)
    return c0, c1


def resize_u8_linear(src, hw_out):
    """(T, H0, W0, C) uint8 -> (T, h, w, C) uint8."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 4
    h, w = hw_out
    y0, y1, fy = linear_coords(src.shape[1], h)
    x0, x1, fx = linear_coords(src.shape[2], w)
    a0, a1 = (c.astype(np.int32)[None, None, :, None] for c in coefficients(fx))
    b0, b1 = (c.astype(np.int32)[None, :, None, None] for c in coefficients(fy))
    s = src.astype(np.int32)
    rows = s[:, :, x0] * a0 + s[:, :, x1] * a1                      # (T, H0, w, C) int32, the horizontal pass
    r0, r1 = rows[:, y0], rows[:, y1]
    out = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def resize_u8_nearest(src, hw_out):
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 4
    ys, xs = nearest_coords(src.shape[1], hw_out[0]), nearest_coords(src.shape[2], hw_out[1])
    return src[:, ys][:, :, xs]


def resize_f32_linear(src, hw_out):
    """(T, H0, W0) fp32 -> (T, h, w) fp32; each multiply and add rounded to fp32 on its own, operands in the rule's order."""
    src = np.asarray(src)
    assert src.dtype == F32 and src.ndim == 3
    h, w = hw_out
    y0, y1, fy = linear_coords(src.shape[1], h)
    x0, x1, fx = linear_coords(src.shape[2], w)
    w0, w1 = (F32(1) - fx)[None, None, :], fx[None, None, :]
    v0, v1 = (F32(1) - fy)[None, :, None], fy[None, :, None]
    with np.errstate(all="ignore"):
        rows = (src[:, :, x0] * w0).astype(F32) + (src[:, :, x1] * w1).astype(F32)
        rows = rows.astype(F32)
        out = (rows[:, y0] * v0).astype(F32) + (rows[:, y1] * v1).astype(F32)
    return out.astype(F32)


def colourise(ids):
    """(…) uint8 class ids -> (…, 3) uint8; an id above 20 is black."""
    ids = np.asarray(ids)
    table = np.concatenate([PALETTE, np.zeros((256 - len(PALETTE), 3), dtype=np.uint8)])
    return table[ids]


def norm_u8(frames):
    """(T, h, w, 3) uint8 -> (3, T, h, w) fp32: (v / 255 - 0.5) * 2, each step in fp32."""
    v = np.asarray(frames).astype(F32)
    v = ((v / F32(255)).astype(F32) - F32(0.5)).astype(F32) * F32(2)
    return np.ascontiguousarray(v.astype(F32).transpose(3, 0, 1, 2))


def colour_stream(images, hw_out):
    u8 = resize_u8_linear(images, hw_out)
    return norm_u8(u8), u8


def semantic_stream(ids, hw_out):
    u8 = resize_u8_linear(colourise(ids), hw_out)
    return norm_u8(u8), u8


def depth_stream(depth, hw_out):
    d = resize_f32_linear(depth, hw_out)
    d = np.minimum(np.maximum(d, F32(0)), F32(100))
    d = (((d / F32(100)).astype(F32) - F32(0.5)).astype(F32) * F32(2)).astype(F32)
    return np.ascontiguousarray(np.broadcast_to(d[None], (3,) + d.shape))


def choose_label(train_labels, u):
    """The label of an item for the draw u in [0, 1)."""
    if len(train_labels) == 1:
        return train_labels[0]
    if len(train_labels) == 2:
        return train_labels[0] if u > 0.5 else train_labels[1]
    if u < 0.25:
        return "depth"
    return "semantic" if u < 0.5 else "color"
