#!/usr/bin/env python3
"""Capture the training-from-a-data-batch fixture from the REFERENCE implementation: LatentVisualDiffusion.get_batch_input and
shared_step (ddpm3d.py:1056-1149) on the tiny model of make_golden.py's driver golden.

Run in the build container only:   python tests/golden/make_golden_batch.py
The reference is imported exactly as make_golden.py imports it (that module is loaded for its stubs and helpers; none of its
goldens is rewritten).  A seeded batch of B = 4 clips goes through the reference's get_batch_input on the CPU with torch.rand
replaced by the recorded vector r = [0.02, 0.07, 0.12, 0.60] — with uncond_prob 0.05 one sample in each dropout case: text
dropped, both dropped, image dropped, none — and once with random_uncond=False; then through the reference's shared_step, whose
timesteps and noise are recorded.  The image tower is the per-sample fake of towers_batch.py.  Only data is stored
(tests/golden/batch_input.pt); weights are re-derived from seeding.py on both sides."""
import importlib.util
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mg = _load("make_golden")           # puts the reference on sys.path and installs the no-math stubs
import torch                        # noqa: E402

cfgs, seeding = mg.cfgs, mg.seeding
R = [0.02, 0.07, 0.12, 0.60]
B = 4
CPU_SEED = 31
INPUT_SEED = cfgs.SEED + 11
DIFF = dict(cfgs.DIFFUSION, first_stage_key="dense_frames", uncond_prob=0.05)


def build():
    from lvdm.modules.encoders.resampler import Resampler
    towers, towers_batch = _load("towers"), _load("towers_batch")
    d = cfgs.DRIVER
    model = mg.build_diffusion(cfgs.UNET_B, DIFF)
    unet_shapes, unet_cks = mg.reseed(model.model.diffusion_model, cfgs.SEED)
    vae_shapes, vae_cks = mg.reseed(model.first_stage_model, cfgs.SEED + 1)
    model.image_proj_model = Resampler(**d["resampler"]).eval()
    rs_shapes, rs_cks = mg.reseed(model.image_proj_model, cfgs.SEED + 5)
    model.embedder = towers_batch.PerSampleImageTower(d["clip_tokens"], d["clip_dim"], d["tower_seed_img"])
    model.cond_stage_model = towers.FakeTextTower(cfgs.UNET_B["context_dim"], d["tower_seed_txt"])
    meta = {"unet_cfg": cfgs.UNET_B, "diffusion_cfg": DIFF, "vae_ddconfig": cfgs.VAE_DD, "seed": cfgs.SEED, "driver": d,
            "unet_checksum": unet_cks, "vae_checksum": vae_cks, "resampler_checksum": rs_cks, "unet_param_shapes": unet_shapes,
            "vae_param_shapes": vae_shapes, "resampler_param_shapes": rs_shapes}
    return model, meta


def make_batch():
    """The data batch; the tests rebuild it from the same seeds (tests/test_batch_input_gpu.py)."""
    T, px = cfgs.UNET_B_SHAPE["T"], cfgs.DRIVER["pixels"]
    clip = lambda name: seeding.seeded_input(name, (B, 3, T, px, px), INPUT_SEED, 0.5).clamp(-1, 1)
    return {"dense_frames": clip("bi_dense"), "sparse_frames": clip("bi_sparse"), "sparse_depth": clip("bi_depth"),
            "class_label": torch.tensor([0, 500, 1, 0], dtype=torch.long)[:, None], "caption": ["a street"] * B,
            "fps": torch.full((B,), 10, dtype=torch.long)}


def main():
    model, meta = build()
    batch = make_batch()
    T = cfgs.UNET_B_SHAPE["T"]
    flat = lambda x: x.permute(0, 2, 1, 3, 4).reshape(B * T, x.shape[1], *x.shape[3:])
    moments = {k: model.first_stage_model.encode(flat(batch[k])).parameters.clone()
               for k in ("dense_frames", "sparse_frames", "sparse_depth")}
    r = torch.tensor(R)
    real_rand = torch.rand
    outs = {}
    for tag, uncond in (("dropout", True), ("full", False)):
        torch.rand = lambda *a, **k: r.clone()
        try:
            torch.manual_seed(CPU_SEED)
            z, sparse_z, cond, fs, label = model.get_batch_input(batch, random_uncond=uncond, return_fs=True, return_class_label=True)
        finally:
            torch.rand = real_rand
        outs[tag] = {"z": z.clone(), "sparse_z": sparse_z.clone(), "c_concat": cond["c_concat"][0].clone(),
                     "c_crossattn": cond["c_crossattn"][0].clone(), "fs": fs.clone(), "class_label": label.clone()}
    seen = {}
    orig_q = model.q_sample

    def q_tapped(x_start, t, noise=None):
        seen.update(t=t.clone(), noise=noise.clone())
        return orig_q(x_start=x_start, t=t, noise=noise)

    model.q_sample = q_tapped
    torch.rand = lambda *a, **k: r.clone()
    try:
        torch.manual_seed(CPU_SEED)
        loss, loss_dict = model.shared_step(batch, random_uncond=True)
    finally:
        torch.rand = real_rand
    path = os.path.join(HERE, "batch_input.pt")
    torch.save(dict(meta, B=B, r=r, cpu_seed=CPU_SEED, input_seed=INPUT_SEED, moments=moments, outs=outs, t=seen["t"],
                    noise=seen["noise"], loss=loss.clone(), loss_dict={k: v.clone() for k, v in loss_dict.items()}), path)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
