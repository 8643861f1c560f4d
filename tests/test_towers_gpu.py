"""The image tower on the GPU (csrc/towers.hip, mudg_amd/engine/clip.py, mudg_amd/towers.py) against tests/clip_reference.py.  The file
runs in the default build directly and in fp16, bf16x3 and bf16x6 in child processes of its own (the operand type is fixed per process).

  attention      mudg_short_attention called directly.  gather: q row i is the +-4 code of key pi(i), all weight on that key, O = V[pi(i)]
                 bit for bit; uniform: q = k = 0, every key weighs 1 / N: O is the mean of V (exactly V where V is constant over the
                 keys); random operands block by block within 3 x the distance of the rounding emulation from the unrounded definition
                 (bf16x6: or 4 x the distance of fp32 arithmetic); NaN-filled gaps; repeat runs; refusals.
  preprocessing  torch.equal with the fp32 definition, image and patch matrix.
  tower          the CLIPVisionModel fixture, the real width, batch independence.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

import clip_reference as cr
from attention_reference import through
from helpers import ChildRuns, cached_oracle, golden, record_parity, rel_l2, seeded_sd
from mudg_amd import hip, ops
from test_backward_kernels_gpu import NAN, base_of, check, filled_operand, gapped
from test_operand_modes_gpu import MODE, value
from test_towers_cpu import ATTN_B as B, ATTN_HEADS as HEADS, ATTN_SHAPES, PRE_SHAPES, attn_qkv, pre_image

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = (hip.operand_dtype(), hip.planes())
# one operand rounding of the mode, relative (tests/test_operand_modes_gpu.py: test_cast_round_trip_is_exact_to_the_modes_precision)
EPS = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "bf16x3": 2.0 ** -17, "bf16x6": 2.0 ** -24}[MODE]
CHILD = os.environ.get("MUDG_PARITY_CHILD") == "1"
IDS = [f"d{d}-N{n}" for d, n in ATTN_SHAPES]


def bound_of(name, emu, plain, want):
    """3 x the rel-L2 distance of the rounding emulation from the unrounded fp64 definition; bf16x6 alone: or 4 x that of fp32 arithmetic
    (its pieces carry fp32's own 24 bits: the emulation sits below what any fp32 accumulation reaches)."""
    d_emu, d_f32 = rel_l2(emu, want), rel_l2(plain, want)
    bound = max(3.0 * d_emu, 4.0 * d_f32) if MODE == "bf16x6" else 3.0 * d_emu
    print(f"[towers {MODE}] {name}: rel-L2 from fp64 of the rounding emulation {d_emu:.3e}, of fp32 {d_f32:.3e}; bound {bound:.3e}")
    return bound


# ------------------------------------------------------------------------------------------------ attention
def run_attention(qkv32, d, n, dev, out=None):
    qkv = qkv32 if qkv32.is_cuda else qkv32.float().contiguous().to(dev)
    return ops.short_attention(qkv, out, batch=B, heads=HEADS, n=n, d=d)


def codes(n, d, g):
    """n rows of +-4 of width d, any two of which differ in at least 12 places: a row's score against itself is 16 d, against any other
    at most 16 (d - 24) — with scale d^-1/2 a gap of 384 / sqrt(d) >= 42 nats, so every other key weighs below e^-42 < 2^-60."""
    c = torch.where(torch.rand((n, d), generator=g) < 0.5, -1.0, 1.0)
    for _ in range(64):
        dots = c @ c.t() - float(d) * torch.eye(n)
        bad = (dots.max(1).values > d - 24).nonzero().flatten()
        if bad.numel() == 0:
            return c * 4.0
        c[bad] = torch.where(torch.rand((bad.numel(), d), generator=g) < 0.5, -1.0, 1.0)
    raise AssertionError("no code set found")


@functools.lru_cache(maxsize=None)
def gather_problem(d, n):
    """(qkv, want): per (image, head) the keys are distinct codes, q row i is the code of key pi(i) (a random permutation: every key is
    some row's target), V is +-(1 .. 64) / 8: exact in every operand type and never zero."""
    g = torch.Generator().manual_seed(77 * d + n)
    c = HEADS * d
    qkv, want = torch.zeros((B * n, 3 * c)), torch.zeros((B * n, c))
    for b in range(B):
        for h in range(HEADS):
            rows, hs = slice(b * n, (b + 1) * n), slice(h * d, (h + 1) * d)
            k = codes(n, d, g)
            v = torch.randint(1, 65, (n, d), generator=g).float() / 8.0
            v = torch.where(torch.rand(v.shape, generator=g) < 0.5, -v, v)
            pi = torch.randperm(n, generator=g)
            qkv[rows, hs], qkv[rows, c + h * d:c + (h + 1) * d], qkv[rows, 2 * c + h * d:2 * c + (h + 1) * d] = k[pi], k, v
            want[rows, hs] = v[pi]
    return qkv, want


@pytest.mark.parametrize("d,n", ATTN_SHAPES, ids=IDS)
def test_one_matching_key_returns_its_value_row_bit_for_bit(cuda, d, n):
    qkv, want = gather_problem(d, n)
    got = value(run_attention(qkv, d, n, cuda))
    wrong = (got != want.double()).any(1).nonzero().flatten().tolist()
    assert not wrong, f"d={d} N={n}: {len(wrong)} wrong rows, first {wrong[:8]} (row = image * N + query)"


@pytest.mark.parametrize("d,n", ATTN_SHAPES, ids=IDS)
def test_zero_q_and_k_return_the_mean_of_v(cuda, d, n):
    c = HEADS * d
    g = torch.Generator().manual_seed(5 * d + n)
    # V constant over the keys of an (image, head, channel): the mean is that constant, exactly
    const = (torch.randint(-48, 49, (B, 1, c), generator=g).float() / 8.0).expand(B, n, c).reshape(B * n, c)
    qkv = torch.zeros((B * n, 3 * c))
    qkv[:, 2 * c:] = const
    assert torch.equal(value(run_attention(qkv, d, n, cuda)), const.double())
    # V varying: the mean of multiples of 1/8 is one exact fp32 division, then one operand rounding
    v = torch.randint(-48, 49, (B * n, c), generator=g).float() / 8.0
    qkv[:, 2 * c:] = v
    got = value(run_attention(qkv, d, n, cuda))
    mean = v.double().reshape(B, n, c).mean(1, keepdim=True).expand(B, n, c).reshape(B * n, c)
    assert bool(((got - mean).abs() <= (EPS + 2.0 ** -24) * mean.abs()).all()), float(((got - mean).abs() / mean.abs().clamp_min(1e-30)).max())


@pytest.mark.parametrize("d,n", ATTN_SHAPES, ids=IDS)
def test_random_operands_against_the_fp64_definition(cuda, d, n):
    qkv = attn_qkv(d, n)
    kw = dict(batch=B, heads=HEADS, n=n, d=d)
    want = cr.short_attention(qkv, **kw)
    emu = cr.short_attention(qkv, round_to=RT, **kw)
    plain = cr.short_attention(qkv, dtype=torch.float32, **kw)
    out = run_attention(qkv, d, n, cuda)
    check(f"short attention d={d} N={n}", value(out), want, bound_of(f"short attention d={d} N={n}", emu, plain, want), rb=32, cb=d)
    assert torch.equal(value(run_attention(qkv, d, n, cuda)), value(out))                  # a repeat run is bit-equal


@pytest.mark.parametrize("d,n", [(80, 257), (64, 77), (80, 17)], ids=["d80-N257", "d64-N77", "d80-N17"])
def test_packed_views_with_nan_gaps(cuda, d, n):
    c = HEADS * d
    qkv = attn_qkv(d, n)
    dense = value(run_attention(qkv, d, n, cuda))
    qv = gapped(qkv, 3 * c + 5, cuda)                                                    # fp32 rows 3 C + 5 wide, an odd stride
    big = filled_operand(B * n + 4, c + 8, cuda, NAN)
    out = big[2:2 + B * n, :c]
    run_attention(qv, d, n, cuda, out=out)
    assert torch.equal(value(out), dense)
    base, ld = base_of(big), base_of(big).shape[1] // hip.planes()
    assert all(bool(torch.isnan(base[:, p * ld + c:(p + 1) * ld]).all()) for p in range(hip.planes()))
    assert bool(torch.isnan(base[:2]).all()) and bool(torch.isnan(base[-2:]).all())
    assert bool(torch.isnan(base_of(qv)[:, 3 * c:]).all())


def test_attention_refuses_what_it_does_not_implement(cuda):
    lib = hip.lib()
    for d, n, short in ((80, 289, 0), (48, 64, 0), (80, 64, 8)):
        c = HEADS * d
        qkv = torch.zeros((B * n, 3 * c - short), dtype=torch.float32, device=cuda)
        out = ops.empty_rows(B * n, c, None, cuda)
        out.fill_(7.0)
        desc = ops.short_attention_desc(qkv.data_ptr(), out.data_ptr(), batch=B, heads=HEADS, n=n, d=d, ldqkv=qkv.stride(0), ldo=out.stride(0))
        assert lib.mudg_short_attention_ok(ctypes.byref(desc)) == 0
        assert lib.mudg_short_attention(ctypes.byref(desc), None) == -1 and lib.mudg_last_error()
        with pytest.raises(hip.MudgError):
            ops.short_attention(qkv, out, batch=B, heads=HEADS, n=n, d=d)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())                                                   # nothing was launched


# ------------------------------------------------------------------------------------------------ preprocessing
@functools.lru_cache(maxsize=None)
def pre_want(shape, antialias=True):
    return cr.preprocess(pre_image(shape), antialias)


def same_image_and_patches(name, image, patches, want):
    wi, wp = torch.from_numpy(want[0]), through(RT)(torch.from_numpy(want[1]))
    differ = int((image.cpu() != wi).sum())
    print(f"[towers {MODE}] {name}: {differ} of {wi.numel()} image values differ")
    assert image.dtype == torch.float32 and torch.equal(image.cpu(), wi), (name, differ)
    assert torch.equal(value(patches), wp.double()), (name, int((value(patches) != wp.double()).sum()))


@pytest.mark.parametrize("shape", PRE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_preprocessing_is_the_definition(cuda, shape):
    x = torch.from_numpy(pre_image(shape)).to(cuda)
    patches, image = ops.clip_preprocess(x, return_image=True)
    same_image_and_patches(f"preprocess {shape}", image, patches, pre_want(shape))
    again = ops.clip_preprocess(x)                                                        # without the image, and again
    assert torch.equal(base_of(again), base_of(patches))


def test_preprocessing_special_cases(cuda):
    zero = torch.zeros((1, 3, 320, 512), dtype=torch.float32, device=cuda)
    image = ops.clip_preprocess(zero, return_image=True)[1].cpu().numpy()
    for c in range(3):
        assert (image[0, c] == (np.float32(0.5) - cr.MEAN[c]) / cr.STD[c]).all()
    shape = (1, 320, 512)
    x = torch.from_numpy(pre_image(shape)).to(cuda)
    patches, image = ops.clip_preprocess(x, antialias=False, return_image=True)
    same_image_and_patches("preprocess without antialias", image, patches, pre_want(shape, False))
    assert not torch.equal(image.cpu(), torch.from_numpy(pre_want(shape)[0]))
    # destinations inside NaN-filled buffers
    big_p = filled_operand(256 + 6, cr.KPAD + 8, cuda, NAN)
    big_i = torch.full((3, 3, 224, 224), NAN, dtype=torch.float32, device=cuda)
    p, im = ops.clip_preprocess(x, patches=big_p[3:259, :cr.KPAD], image=big_i[1:2], return_image=True)
    same_image_and_patches("preprocess into NaN-filled buffers", im, p, pre_want(shape))
    base, ld = base_of(big_p), base_of(big_p).shape[1] // hip.planes()
    assert all(bool(torch.isnan(base[:, pl * ld + cr.KPAD:(pl + 1) * ld]).all()) for pl in range(hip.planes()))
    assert bool(torch.isnan(base[:3]).all()) and bool(torch.isnan(base[259:]).all())
    assert bool(torch.isnan(big_i[0]).all()) and bool(torch.isnan(big_i[2]).all())
    with pytest.raises(hip.MudgError):
        ops.clip_preprocess(x.cpu())


# ------------------------------------------------------------------------------------------------ the tower
def build_tower(width, layers, heads, sd, dev):
    from mudg_amd.towers import FrozenOpenCLIPImageEmbedderV2
    tower = FrozenOpenCLIPImageEmbedderV2(width=width, layers=layers, heads=heads, embed_dim=64, text_leftovers=False)
    visual = {"model.visual." + k: v for k, v in sd.items()}
    for k, v in tower.state_dict().items():                  # ln_post and proj are not on the path
        visual.setdefault(k, torch.zeros_like(v))
    tower.load_state_dict(visual, strict=True)
    return tower.to(dev)


@functools.lru_cache(maxsize=None)
def fixture_tower():
    g = golden("clip_tower.pt")
    return g, seeded_sd(g["param_shapes"], g["seed"], g["checksum"])


def test_tower_matches_the_clip_vision_model_fixture(cuda):
    from mudg_amd.engine import clip
    g, sd = fixture_tower()
    cfg = g["config"]
    tower = build_tower(cfg["width"], cfg["layers"], cfg["heads"], sd, cuda)
    p32 = torch.from_numpy(cr.patches_of(g["image"].float().numpy()))
    patches = ops.cast_rows(p32.to(cuda), ops.empty_rows(p32.shape[0], cr.KPAD, None, cuda))
    got = clip.forward_patches(tower, patches)
    want = cr.tower(sd, patches=p32, heads=cfg["heads"])
    assert rel_l2(want, g["tokens"]) <= 1e-6
    emu = cr.tower(sd, patches=p32, heads=cfg["heads"], round_to=RT)
    plain = cr.tower(sd, patches=p32, heads=cfg["heads"], dtype=torch.float32)
    bound = bound_of("tower, fixture configuration", emu, plain, want)
    err = rel_l2(got, g["tokens"])
    print(f"[towers {MODE}] tower at width 160, 2 layers against the CLIPVisionModel tokens: rel-L2 {err:.3e}, bound {bound:.3e}")
    record_parity(MODE, "clip_tower_fixture", err, bound=bound)
    assert got.shape == (2, 257, 160) and got.dtype == torch.float32 and bool(torch.isfinite(got).all()) and err <= bound
    assert torch.equal(clip.forward_patches(tower, patches), got)


def test_tower_at_the_real_width(cuda):
    """1280 wide, 16 heads of 80, MLP 5120, 2 layers, B = 1, from a raw image: the 3840- and 5120-wide GEMMs, 16 heads, M = 257."""
    width, layers, heads, seed = 1280, 2, 16, 4242
    sd = seeded_sd(cr.visual_shapes(width, layers, heads, embed_dim=64), seed)
    x = pre_image((1, 36, 64))
    image = cr.preprocess(x)[0]
    want, _ = cached_oracle(f"clip_tower_w{width}_l{layers}_s{seed}_36x64", lambda: cr.tower(sd, image, heads=heads))
    emu = cr.tower(sd, image, heads=heads, round_to=RT)
    plain = cr.tower(sd, image, heads=heads, dtype=torch.float32)
    bound = bound_of("tower, real width", emu, plain, want)
    tower = build_tower(width, layers, heads, sd, cuda)
    got = tower(torch.from_numpy(x).to(cuda))
    err = rel_l2(got, want)
    print(f"[towers {MODE}] tower at width 1280, 2 layers against the fp64 definition: rel-L2 {err:.3e}, bound {bound:.3e}")
    record_parity(MODE, "clip_tower_real_width", err, bound=bound)
    assert got.shape == (1, 257, 1280) and bool(torch.isfinite(got).all()) and err <= bound


def test_a_batch_of_three_equals_three_calls_of_one(cuda):
    g, sd = fixture_tower()
    cfg = g["config"]
    tower = build_tower(cfg["width"], cfg["layers"], cfg["heads"], sd, cuda)
    x = torch.from_numpy(pre_image((3, 40, 72))).to(cuda)
    whole = tower(x)
    assert whole.shape == (3, 257, 160)
    for i in range(3):
        assert torch.equal(tower(x[i:i + 1])[0], whole[i]), i
    assert not torch.equal(whole[0], whole[1])
    with pytest.raises(RuntimeError, match="GPU"):
        tower(x.cpu())


# ------------------------------------------------------------------------------------------------ the path
def test_a_real_tower_on_the_tiny_driver_model(cuda):
    """tests/test_batch_input_gpu.py's tiny model with a real tower (width 1280, 1 layer) where the fake one stood, and a Resampler
    whose embedding_dim takes its tokens: synthesize_windows (guided: the unconditional branch embeds the all-zero image) and
    get_batch_input run, return finite tensors of the right shapes and repeat bit for bit."""
    from helpers import cfgs
    from lvdm.modules.encoders.resampler import Resampler
    from test_batch_input_gpu import build_model, make_batch
    from virtual_render.virtual_pose_render import synthesize_windows
    g = golden("batch_input.pt")
    model = build_model(g, cuda)
    d, L = g["driver"], g["unet_cfg"]["temporal_length"]
    res = Resampler(**dict(d["resampler"], embedding_dim=1280))
    res.load_state_dict(seeded_sd({k: tuple(v.shape) for k, v in res.state_dict().items()}, 31), strict=True)
    model.image_proj_model = res.to(cuda).eval()
    model.embedder = build_tower(1280, 1, 16, seeded_sd(cr.visual_shapes(1280, 1, 16, embed_dim=64), 32), cuda)
    seen = {"zero": 0, "image": 0, "shapes": set()}

    def watch(module, args, output):
        seen["zero" if float(args[0].abs().sum()) == 0.0 else "image"] += 1
        seen["shapes"].add(tuple(output.shape[1:]))
        assert bool(torch.isfinite(output).all())

    model.embedder.register_forward_hook(watch)
    px, sm = d["pixels"], cfgs.SAMPLER
    gen = torch.Generator().manual_seed(9)
    clip_ = lambda: (torch.rand((3, 3, L, px, px), generator=gen) * 2 - 1).to(cuda)
    wins = [{"sparse": clip_(), "dense": clip_(), "sparse_depth": clip_(), "class_label": torch.tensor([[0], [500], [1]])}]

    def synth():
        torch.manual_seed(4)
        return synthesize_windows(model, wins, [3, 4, L, px // 8, px // 8], video_length=L, ddim_steps=2, ddim_eta=1.0,
                                  unconditional_guidance_scale=sm["cfg_scale"], fs=sm["fs"], timestep_spacing=sm["spacing"],
                                  guidance_rescale=sm["guidance_rescale"])[0]

    first = synth()
    assert first.shape == (3, 1, 3, L, px, px) and bool(torch.isfinite(first).all())
    assert seen["zero"] >= 1 and seen["image"] >= 1 and seen["shapes"] == {(257, 1280)}, seen
    assert torch.equal(synth(), first)
    batch = make_batch(g, cuda)

    def batch_input():
        torch.manual_seed(5)
        with torch.no_grad():
            return model.get_batch_input(batch, random_uncond=False)

    z, sparse_z, cond = batch_input()
    ctx = cond["c_crossattn"][0]
    assert z.shape == (g["B"], 4, L, px // 8, px // 8) and ctx.shape[0] == g["B"] and ctx.shape[2] == g["unet_cfg"]["context_dim"]
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(ctx).all()) and bool(torch.isfinite(cond["c_concat"][0]).all())
    z2, _, cond2 = batch_input()
    assert torch.equal(z2, z) and torch.equal(cond2["c_crossattn"][0], ctx)


# ------------------------------------------------------------------------------------------------ the other operand builds
if not CHILD:
    CHILD_MODES = [m for m in ("fp16", "bf16x3", "bf16x6") if m != MODE]

    @pytest.fixture(scope="module")
    def children():
        runs = ChildRuns(workers=len(CHILD_MODES))
        for mode in CHILD_MODES:
            env = dict(os.environ, MUDG_PARITY_CHILD="1", MUDG_OPERAND=mode)
            runs.submit(mode, [sys.executable, "-m", "pytest", "tests/test_towers_gpu.py", "-m", "gpu", "-q", "-s", "-p", "no:cacheprovider"], ROOT, env, 900)
        yield runs
        runs.shutdown()

    @pytest.mark.parametrize("mode", CHILD_MODES)
    def test_this_file_in_the_other_operand_builds(cuda, mode, children):
        rc, stdout = children.result(mode)
        print("\n".join(l for l in stdout.splitlines() if "rel-L2" in l or "passed" in l or "failed" in l or l.startswith("[child")))
        assert rc == 0, stdout[-6000:]
