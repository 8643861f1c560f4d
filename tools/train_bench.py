#!/usr/bin/env python3
"""One training step (p_losses -> backward -> AdamW) of the full 1.44 B-parameter MDM UNet on ONE MI355X: seconds per step, peak
memory.  `python tools/train_bench.py [512|1024] [steps] [ckpt] [stage2] [b4] [acc2] [json]` — `ckpt` turns activation checkpointing on
(use_checkpoint); `stage2` applies what the reference's stage-2 training config adds to a step (configs/stage2-1024_mdm_waymo/
config.yaml): the stages' temporal transformers frozen (temporal_frozen), the gradient 2-norm clipped to 0.5; `b4` = the
reference's per-GPU batch of 4 clips (config.yaml:113-135), `acc2` = its accumulate_grad_batches 2 (two micro-batches per
optimiser step).  All parameters trainable and no clipping otherwise (the heavier step).  FLOP accounting: 3 x the forward per
clip, whatever is frozen.  After the timed steps one more step runs with the contraction families bracketed by hipEvents
(forward GEMMs / convs / attention and the input-gradient GEMMs that run on the same kernels): the `roofline` of the json.

`--ema` (anywhere after the step count): after the plain steps the same number of steps runs with the averaged weights
(lvdm.ema.LitEma over the UNet) updated inside the optimiser's launch (AdamW.step(ema=...): mudg_adamw_ema_multi), reported next to
the plain step of the same run, together with the achieved TB/s of mudg_ema_multi (3 x 4 bytes per parameter) and mudg_swap_multi
(4 x 4 bytes per parameter) on their own (the launches on their prebuilt tables, 20 repeats between two events).

`--scaler` (anywhere after the step count; meant for MUDG_OPERAND=fp16): after the plain steps, `steps` pairs of (plain step, step under a
mudg_amd.train.step.LossScaler: scaled loss, the scaled norm pass, AdamW.step(scaler=...), update()) run alternating in the same process; both
lists of seconds are reported with their spread (max - min).  The pairs share one optimiser, so the plain steps in between advance the host's
step count only: a timing run, not a training run.  `--scaler=1` starts at scale 1 instead of 2^16: the same launches on the plain step's own
gradient values, which separates what the launches cost from what the larger operand values cost.

`python tools/train_bench.py --log-images [512|1024]`: one LatentVisualDiffusion.log_images call from a pixel batch (B = 1, 50 DDIM
steps, guidance 7.5, the towers' stand-ins of --from-pixels) in seconds, after a 2-step warm-up call, next to 100 sampler steps of the
same model in the same process (two 50-step sample_log runs on the conditioning log_images built).

`python tools/train_bench.py --from-pixels [512 1024] [json]`: one step from a PIXEL batch per resolution (B = 1: 3 streams x 16 frames through
the VAE encoder, conditioning dropout, Resampler, then the step above).  Reports get_batch_input's milliseconds (five repeats after a
warm-up call) next to the same work written with three encode_first_stage calls + torch.cat / torch.where — what a caller could write
before get_batch_input existed — timed the same way in the same process, and get_batch_input's share of the whole step.  The CLIP towers
are outside this package: device-resident stand-ins of the towers' output shapes take their place and cost nothing."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mudg_amd import configs, factory

RESAMPLER_MDM = {"target": "lvdm.modules.encoders.resampler.Resampler",          # the image_proj_stage_config of the MDM training configs
                 "params": dict(dim=1024, depth=4, dim_head=64, heads=12, num_queries=16, embedding_dim=1280, output_dim=1024, ff_mult=4, video_length=16)}
PIXELS = {"512": (320, 512), "1024": (576, 1024)}


class _Tower(torch.nn.Module):
    """A stand-in for a frozen CLIP tower: fixed tokens of the tower's output shape, already on the device."""

    def __init__(self, rows, null=None):
        super().__init__()
        self.rows, self.null = rows, null

    def encode(self, prompts):
        return self.null if list(prompts) == [""] else self.rows

    def forward(self, x):
        return self.rows


def _timed(fn, repeats=5):
    fn()                                                    # warm-up: packed weights, kernel plans, allocator
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def from_pixels(res, dev):
    model = factory.build_synthetic_model(res, dev, seed=123, overrides={"image_proj_stage_config": RESAMPLER_MDM, "first_stage_key": "dense_frames",
                                                                         "uncond_prob": 0.05}).train()
    g = torch.Generator(device=dev).manual_seed(7)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    model.cond_stage_model = _Tower(rn(1, 77, 1024), rn(1, 77, 1024))
    model.embedder = _Tower(rn(1, 257, 1280))
    h, w = PIXELS[res]
    clip = lambda: rn(1, 3, 16, h, w).clamp(-1, 1)
    batch = {"dense_frames": clip(), "sparse_frames": clip(), "sparse_depth": clip(), "class_label": torch.tensor([[500]], device=dev),
             "caption": ["a street"], "fps": torch.tensor([10], device=dev)}
    p = model.uncond_prob

    def by_hand():                                          # the same work without get_batch_input: three encodes, cat, where
        z = model.encode_first_stage(batch["dense_frames"])
        sparse_z, depth_z = model.encode_first_stage(batch["sparse_frames"]), model.encode_first_stage(batch["sparse_depth"])
        cat = torch.cat([sparse_z, depth_z], 1)
        r = torch.rand(1, device=dev)
        emb, null = model.get_learned_conditioning(batch["caption"]), model.get_learned_conditioning([""])
        prompt = torch.where((r < 2 * p)[:, None, None], null, emb)
        keep = 1 - ((r >= p).float() * (r < 3 * p).float())[:, None, None, None]
        with torch.no_grad():
            tokens = model.embedder(keep * batch["sparse_frames"][:, :, 0])
        return z, cat, torch.cat([prompt, model.image_proj_model(tokens)], 1)

    hand = _timed(by_hand)
    new = _timed(lambda: model.get_batch_input(batch, random_uncond=True, return_fs=True, return_class_label=True))
    model.learning_rate = 1e-5
    opt = model.configure_optimizers()

    def one_step():
        opt.zero_grad(set_to_none=False)
        model.training_step(batch).backward()
        opt.step()

    step_ms = _timed(one_step, repeats=3)
    med = lambda v: sorted(v)[len(v) // 2]
    return {"workload": f"MDM{res} training step from a pixel batch: get_batch_input (3 x 16 frames of {h} x {w}) -> p_losses -> backward -> AdamW, B = 1",
            "get_batch_input_ms": [round(v, 2) for v in new], "by_hand_ms": [round(v, 2) for v in hand],
            "get_batch_input_ms_median": round(med(new), 2), "by_hand_ms_median": round(med(hand), 2),
            "by_hand_spread_ms": round(max(hand) - min(hand), 2), "step_ms": [round(v, 1) for v in step_ms],
            "share_of_step": round(med(new) / med(step_ms), 4),
            "by_hand": "three encode_first_stage calls + torch.cat / torch.where + the same towers and Resampler, same process, timed first"}


def log_images_bench(res, dev):
    model = factory.build_synthetic_model(res, dev, seed=123, overrides={"image_proj_stage_config": RESAMPLER_MDM, "first_stage_key": "dense_frames",
                                                                         "uncond_prob": 0.05}).eval()
    g = torch.Generator(device=dev).manual_seed(7)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    model.cond_stage_model = _Tower(rn(1, 77, 1024), rn(1, 77, 1024))
    model.embedder = _Tower(rn(1, 257, 1280))
    h, w = PIXELS[res]
    clip = lambda: rn(1, 3, 16, h, w).clamp(-1, 1)
    batch = {"dense_frames": clip(), "sparse_frames": clip(), "sparse_depth": clip(), "class_label": torch.tensor([[500]], device=dev),
             "caption": ["a street"], "fps": torch.tensor([10], device=dev)}
    kw = dict(ddim_eta=0.0, unconditional_guidance_scale=7.5)

    def timed(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    model.log_images(batch, ddim_steps=2, **kw)              # warm-up: packed weights, kernel plans, allocator
    calls = [timed(lambda: model.log_images(batch, ddim_steps=50, **kw)) for _ in range(3)]
    # the sampler alone on the same conditioning: 2 x 50 guided steps
    z, _, c, fs, label = model.get_batch_input(batch, random_uncond=False, return_fs=True, return_class_label=True)
    zero = torch.zeros_like(batch["dense_frames"][:, :, 0])
    uc = {"c_concat": c["c_concat"], "c_crossattn": [torch.cat([model.get_learned_conditioning([""]), model.image_proj_model(model.embedder(zero))], 1)]}
    run = lambda: model.sample_log(cond=c, batch_size=1, ddim=True, ddim_steps=50, eta=0.0, unconditional_guidance_scale=7.5,
                                   unconditional_conditioning=uc, fs=fs.long(), class_label=label)
    run()
    hundred = timed(lambda: (run(), run()))
    t_in = timed(lambda: model.get_batch_input(batch, random_uncond=False, return_first_stage_outputs=True))
    return {"workload": f"MDM{res} log_images: one sample, 50 DDIM steps, guidance 7.5, eta 0, from a pixel batch (3 x 16 frames of {h} x {w})",
            "log_images_s": [round(v, 3) for v in calls], "sampler_100_steps_s": round(hundred, 3),
            "get_batch_input_with_reconst_s": round(t_in, 3),
            "note": "log_images = get_batch_input (3 encodes + the decode of reconst) + 50 guided steps + the decode of samples"}


if "--log-images" in sys.argv:
    import json
    with torch.no_grad():
        for r_ in [a for a in sys.argv[1:] if a in PIXELS] or ["512"]:
            print(json.dumps(log_images_bench(r_, torch.device("cuda:0"))), flush=True)
    sys.exit(0)

if "--from-pixels" in sys.argv:
    import json
    for r_ in [a for a in sys.argv[1:] if a in PIXELS] or ["512", "1024"]:
        print(json.dumps(from_pixels(r_, torch.device("cuda:0"))), flush=True)
        torch.cuda.empty_cache()
    sys.exit(0)

res = sys.argv[1] if len(sys.argv) > 1 else "512"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
ckpt = "ckpt" in sys.argv[3:]
stage2 = "stage2" in sys.argv[3:]
B = 4 if "b4" in sys.argv[3:] else 1
ACC = 2 if "acc2" in sys.argv[3:] else 1
dev = torch.device("cuda:0")
model = factory.build_synthetic_model(res, dev, seed=123).train()
unet = model.model.diffusion_model
for m in unet.modules():
    if hasattr(m, "use_checkpoint"):
        m.use_checkpoint = ckpt
    if isinstance(getattr(m, "checkpoint", None), bool):
        m.checkpoint = ckpt
if stage2:
    for m in unet.modules():
        if type(m).__name__ == "TemporalTransformer" and m is not unet.init_attn[0]:
            m._frozen_model()
inp = factory.synthetic_inputs(model, res, B, dev, seed=123)
model.learning_rate = 1e-5
opt = model.configure_optimizers()
from mudg_amd.train import step
clip = step.GradientClipper([p for g in opt.param_groups for p in g["params"]], 0.5) if stage2 else None
batch = dict(x_start=inp["x_T"], cond=inp["cond"], t=torch.tensor([500, 120, 870, 333][:B], device=dev), class_label=inp["class_label"], fs=inp["fs"])
torch.cuda.reset_peak_memory_stats()
times, losses = [], []
EMA = "--ema" in sys.argv[3:]
ema = None                                   # set for the second block of steps
SCALER = next((a for a in sys.argv[3:] if a == "--scaler" or a.startswith("--scaler=")), None)
scaler = None                                # set for every other step of the --scaler block
def one_step():
    opt.zero_grad(set_to_none=False)         # multi-tensor fill; gradient tensors (and the pointer tables built on them) persist
    for _ in range(ACC):
        loss = model.training_step(batch)
        ((loss if scaler is None else scaler.scale(loss)) / ACC).backward()
    if scaler is not None:
        norm = scaler.norm_pass(clip.params if clip is not None else [p for g in opt.param_groups for p in g["params"]],
                                clip.max_norm if clip is not None else None)
        opt.step(ema=ema, scaler=scaler)
        scaler.update()
        return loss, norm
    norm = clip() if clip is not None else None
    if ema is not None:
        opt.step(ema=ema)
    else:
        opt.step()
    return loss, norm


for i in range(steps + 1):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    loss, norm = one_step()
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t0)
    losses.append(float(loss.detach()))
    print(f"step {i}: loss {losses[-1]:.5f}  {times[-1]:.2f} s" + (f"  grad norm {float(norm[0]):.3f}" if norm is not None else ""), flush=True)
ema_report = None
if EMA:
    from lvdm.ema import LitEma
    ema = LitEma(model.model).to(dev)
    ema_times = []
    for i in range(steps + 1):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        loss, norm = one_step()
        torch.cuda.synchronize()
        ema_times.append(time.perf_counter() - t0)
        print(f"step {i} (fused average): loss {float(loss.detach()):.5f}  {ema_times[-1]:.2f} s", flush=True)
    from mudg_amd.train import kernels as K_
    pairs_ = ema.pairs()
    nparam = sum(s_.numel() for _, s_ in pairs_)
    tab_e, n_e = ema._table(("ema", len(pairs_)), pairs_)          # the kernels alone, on their prebuilt tables: no host work per call
    tab_s, n_s = ema._table(("swap", len(pairs_)), pairs_)
    def _tbs(fn, bytes_per_param, reps=20):
        fn(); torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record(); torch.cuda.synchronize()
        ms = a.elapsed_time(b) / reps
        return round(ms, 3), round(bytes_per_param * nparam / (ms / 1e3) / 1e12, 2)
    keep = [p.detach().clone() for p in model.model.parameters()]
    ema_ms, ema_tbs = _tbs(lambda: K_.ema_multi_(tab_e, n_e, 1e-4), 12)
    swap_ms, swap_tbs = _tbs(lambda: (K_.swap_multi_(tab_s, n_s), K_.swap_multi_(tab_s, n_s)), 32)        # an even count: the weights end where they were
    assert all(torch.equal(a_, b_) for a_, b_ in zip(keep, model.model.parameters()))
    del keep
    ema_report = {"s_per_step_plain": round(min(times[1:]), 4), "s_per_step_fused_average": round(min(ema_times[1:]), 4), "averaged_parameters": nparam,
                  "ema_multi_ms": ema_ms, "ema_multi_tb_per_s": ema_tbs, "swap_multi_ms": round(swap_ms / 2, 3), "swap_multi_tb_per_s": swap_tbs}
    print("averaged weights:", ema_report, flush=True)
    ema = None
scaler_report = None
if SCALER:
    the_scaler = step.LossScaler(**({"init_scale": float(SCALER.split("=")[1])} if "=" in SCALER else {}))
    pair = {"plain": [], "scaled": []}
    for i in range(steps + 1):                                         # pair 0 warms the scaled path up (record, chunk table) and is not reported
        for name in ("plain", "scaled"):
            scaler = the_scaler if name == "scaled" else None
            torch.cuda.synchronize(); t0 = time.perf_counter()
            loss, norm = one_step()
            torch.cuda.synchronize()
            if i:
                pair[name].append(time.perf_counter() - t0)
            print(f"pair {i} {name}: loss {float(loss.detach()):.5f}  {time.perf_counter() - t0:.3f} s", flush=True)
    scaler = None
    scaler_report = {"plain_s": [round(v, 4) for v in pair["plain"]], "scaled_s": [round(v, 4) for v in pair["scaled"]],
                     "plain_spread_s": round(max(pair["plain"]) - min(pair["plain"]), 4), "scaled_spread_s": round(max(pair["scaled"]) - min(pair["scaled"]), 4),
                     "scaled_minus_plain_median_s": round(sorted(pair["scaled"])[len(pair["scaled"]) // 2] - sorted(pair["plain"])[len(pair["plain"]) // 2], 4),
                     "loss_scale": the_scaler.get_scale(), "optimizer_steps_taken": the_scaler.taken_steps(), "operand": __import__("mudg_amd.hip").hip.operand_name()}
    print("loss scaling:", scaler_report, flush=True)
from mudg_amd import hip
hip.prof_reset(); hip.prof_enable((1 << len(hip.FAM_NAMES)) - 1)
one_step()
torch.cuda.synchronize()
fams = [hip.prof_collect(i) for i in range(len(hip.FAM_NAMES))]
hip.prof_enable(0)
mf = [f for f in fams if f["family"] in ("gemm", "conv3x3", "tconv3", "attention") and f["launches"]]
dom = max(mf, key=lambda f: f["ms"]) if mf else None
roof = None if dom is None else {"kernel": dom["family"], "bound": "mfma", "achieved": round(dom["flops"] / (dom["ms"] / 1e3) / 1e12, 1), "peak": 2500.0,
                                 "unit": "TFLOP/s", "frac": round(dom["flops"] / (dom["ms"] / 1e3) / 1e12 / 2500.0, 4), "ms_per_step": round(dom["ms"], 2),
                                 "launches_per_step": dom["launches"], "measured": "hipEvents on the launch stream over one more step; the family's "
                                 "forward and input-gradient launches (weight gradients and the attention backward have kernels of their own)"}
fl = 3 * configs.UNET_TFLOP[res] * B * ACC
best = min(times[1:])
if "json" in sys.argv[3:]:
    import json
    print(json.dumps({"workload": f"MDM{res} training step: p_losses -> backward -> AdamW, full 1.44 B-parameter UNet, B = {B}, 16 frames"
                                  + (f", {ACC} micro-batches per optimiser step" if ACC > 1 else ""),
                      "s_per_step": round(best, 4), "steps": steps, "tflops_per_s": round(fl / best, 1), "tflop_per_step": round(fl, 1),
                      "flop_accounting": "3 x the forward per clip", "batch": B, "accumulate": ACC, "roofline": roof, "checkpointing": ckpt, "stage2_settings": stage2, **({"averaged_weights": ema_report} if ema_report else {}), **({"loss_scaling": scaler_report} if scaler_report else {}),
                      "peak_memory_gib": round(torch.cuda.max_memory_allocated() / 2**30, 1), "loss_first_last": [round(losses[0], 5), round(losses[-1], 5)]}))
    sys.exit(0)
print(f"MDM{res} training step (B = {B}" + (f" x {ACC} micro-batches" if ACC > 1 else "") + f", 16 frames, checkpointing {'on' if ckpt else 'off'}{', stage-2 settings' if stage2 else ''}): {best:.2f} s = {fl / best:.1f} TFLOP/s of the "
      f"{fl:.1f} TFLOP a forward + backward costs (3 x forward); peak memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")
