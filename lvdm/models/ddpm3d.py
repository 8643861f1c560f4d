"""Latent video diffusion model at the drop-in boundary (reference: lvdm/models/ddpm3d.py).

What the denoising path needs from the reference's Lightning classes, without Lightning: the schedule buffers
(DDPM.register_schedule 123-186, scale_arr 522-527), the conditioning plumbing (LatentDiffusion.apply_model 723-739,
DiffusionWrapper.forward 1309-1324), the v-parameterisation helpers (239-251), first-stage decode (646-671) and the
constructor surface of LatentVisualDiffusion (1033-1055) so MuDG's YAML configs instantiate it unchanged and its
checkpoints load with the same key prefixes (model.diffusion_model.*, first_stage_model.*, image_proj_model.*).
The training step (p_losses, configure_optimizers, training_step) is delegated to mudg_amd.train.  What the
reference's loop does around a step is here too, without Lightning: the averaged weights (use_ema: lvdm/ema.py, ema_scope,
on_train_batch_end, the *_ema entries of validation_step) and log_images / sample_log (1186-1265, 996-1005), which
main/callbacks.py's ImageLogger calls.  The Lightning loop itself and the data pipeline are not built.
"""
from contextlib import contextmanager
from functools import partial

import numpy as np
import torch
import torch.nn as nn

from lvdm.basics import disabled_train
from lvdm.common import default, extract_into_tensor
from lvdm.models.utils_diffusion import make_beta_schedule, rescale_zero_terminal_snr
from utils.utils import instantiate_from_config


def _cfg_get(cfg, key, fallback=None):
    """Configs arrive as OmegaConf nodes, dicts or attr-dicts."""
    if cfg is None:
        return fallback
    if isinstance(cfg, dict) or hasattr(cfg, "keys"):
        try:
            return cfg[key]
        except (KeyError, TypeError):
            return fallback
    return getattr(cfg, key, fallback)


def _make_grid(tensor, nrow=8, padding=2, pad_value=0.0):
    """torchvision.utils.make_grid for a batch (N, C, H, W) with its defaults (no normalisation): cell k at row k // nrow, column
    k % nrow, top-left corner (row (H + padding) + padding, column (W + padding) + padding) of a (C, rows (H + padding) + padding,
    columns (W + padding) + padding) canvas filled with pad_value; a one-channel batch is repeated to three channels, a batch of
    one image is returned as that image.  (torchvision is not a dependency of this package.)"""
    if tensor.dim() != 4:
        raise ValueError(f"_make_grid lays out a (N, C, H, W) batch, got {tuple(tensor.shape)}")
    if tensor.shape[1] == 1:
        tensor = torch.cat((tensor, tensor, tensor), 1)
    if tensor.shape[0] == 1:
        return tensor.squeeze(0)
    nmaps = tensor.shape[0]
    xmaps = min(nrow, nmaps)
    ymaps = -(-nmaps // xmaps)
    height, width = tensor.shape[2] + padding, tensor.shape[3] + padding
    grid = tensor.new_full((tensor.shape[1], height * ymaps + padding, width * xmaps + padding), pad_value)
    for k in range(nmaps):
        y, x = divmod(k, xmaps)
        grid[:, y * height + padding:(y + 1) * height, x * width + padding:(x + 1) * width] = tensor[k]
    return grid


class DiffusionWrapper(nn.Module):
    """Routes conditioning into the UNet.  'hybrid' (MuDG): latent channels = [x | c_concat...] and context =
    cat(c_crossattn).  The channel concat is not materialised: the pieces go to the UNet as a list and are written
    side by side by the layout kernel."""

    def __init__(self, diff_model_config, conditioning_key):
        super().__init__()
        self.diffusion_model = instantiate_from_config(diff_model_config)
        self.conditioning_key = conditioning_key

    def forward(self, x, t, c_label=None, c_concat: list = None, c_crossattn: list = None, c_adm=None, s=None,
                mask=None, **kwargs):
        key = self.conditioning_key
        ctx = None
        if c_crossattn is not None:
            ctx = c_crossattn[0] if len(c_crossattn) == 1 else torch.cat(list(c_crossattn), 1)
        if key is None:
            return self.diffusion_model(x, t)
        if key == "concat":
            return self.diffusion_model([x] + list(c_concat), t, **kwargs)
        if key == "crossattn":
            return self.diffusion_model(x, t, context=ctx, **kwargs)
        if key == "hybrid":
            return self.diffusion_model([x] + list(c_concat), t, c_label=c_label, context=ctx, **kwargs)
        raise NotImplementedError(f"conditioning_key '{key}' is not on the MuDG path")


class DDPM(nn.Module):
    def __init__(self, unet_config, timesteps=1000, beta_schedule="linear", loss_type="l2", ckpt_path=None,
                 ignore_keys=[], load_only_unet=False, monitor=None, use_ema=True, first_stage_key="image",
                 image_size=256, channels=3, log_every_t=100, clip_denoised=True, linear_start=1e-4, linear_end=2e-2,
                 cosine_s=8e-3, given_betas=None, original_elbo_weight=0., v_posterior=0., l_simple_weight=1.,
                 conditioning_key=None, parameterization="eps", scheduler_config=None, use_positional_encodings=False,
                 learn_logvar=False, logvar_init=0., rescale_betas_zero_snr=False):
        super().__init__()
        assert parameterization in ["eps", "x0", "v"], 'currently only supporting "eps" and "x0" and "v"'
        self.parameterization = parameterization
        self.cond_stage_model = None
        self.clip_denoised, self.log_every_t = clip_denoised, log_every_t
        self.first_stage_key, self.channels = first_stage_key, channels
        self.temporal_length = _cfg_get(_cfg_get(unet_config, "params"), "temporal_length")
        self.image_size = [image_size, image_size] if isinstance(image_size, int) else image_size
        self.use_positional_encodings = use_positional_encodings
        self.model = DiffusionWrapper(unet_config, conditioning_key)
        self.use_ema = bool(use_ema)
        if self.use_ema:
            from lvdm.ema import LitEma
            self.model_ema = LitEma(self.model)
        self.rescale_betas_zero_snr = rescale_betas_zero_snr
        self.v_posterior, self.original_elbo_weight, self.l_simple_weight = v_posterior, original_elbo_weight, l_simple_weight
        if monitor is not None:
            self.monitor = monitor
        self.register_schedule(given_betas=given_betas, beta_schedule=beta_schedule, timesteps=timesteps,
                               linear_start=linear_start, linear_end=linear_end, cosine_s=cosine_s)
        self.given_betas, self.beta_schedule, self.timesteps, self.cosine_s = given_betas, beta_schedule, timesteps, cosine_s
        self.loss_type = loss_type
        if loss_type != "l2":
            raise NotImplementedError("only the l2 loss of the MuDG configs is implemented")
        # ddpm3d.py:118-121,173-186: per-timestep log-variance (a constant unless learn_logvar) and the vlb weights (ones for v)
        self.learn_logvar = learn_logvar
        if learn_logvar:
            raise NotImplementedError("learn_logvar is off in every MuDG config and not implemented")
        with torch.device("cpu"):       # a plain attribute, as in the reference: real memory even under torch.device("meta")
            self.logvar = torch.full(fill_value=float(logvar_init), size=(self.num_timesteps,))
        if ckpt_path is not None:
            self.init_from_ckpt(ckpt_path, ignore_keys=ignore_keys, only_model=load_only_unet)

    @property
    def device(self):
        return self.betas.device

    def register_schedule(self, given_betas=None, beta_schedule="linear", timesteps=1000, linear_start=1e-4,
                          linear_end=2e-2, cosine_s=8e-3):
        with torch.device("cpu"):       # host math even when the model is being built under torch.device("meta")
            self._register_schedule(given_betas, beta_schedule, timesteps, linear_start, linear_end, cosine_s)

    def _register_schedule(self, given_betas, beta_schedule, timesteps, linear_start, linear_end, cosine_s):
        betas = given_betas if given_betas is not None else make_beta_schedule(
            beta_schedule, timesteps, linear_start=linear_start, linear_end=linear_end, cosine_s=cosine_s)
        if self.rescale_betas_zero_snr:
            betas = rescale_zero_terminal_snr(betas)
        abar = np.cumprod(1. - betas, axis=0)
        self.num_timesteps = int(betas.shape[0])
        self.linear_start, self.linear_end = linear_start, linear_end
        f32 = partial(torch.tensor, dtype=torch.float32)
        for name, val in (("betas", betas), ("alphas_cumprod", abar),
                          ("alphas_cumprod_prev", np.append(1., abar[:-1])),
                          ("sqrt_alphas_cumprod", np.sqrt(abar)),
                          ("sqrt_one_minus_alphas_cumprod", np.sqrt(1. - abar)),
                          ("log_one_minus_alphas_cumprod", np.log(np.maximum(1. - abar, 1e-300)))):
            self.register_buffer(name, f32(val))
        # kept for state_dict compatibility with the reference's checkpoints (not used by v-prediction sampling)
        prev = np.append(1., abar[:-1])
        with np.errstate(divide="ignore", invalid="ignore"):
            post_var = (1 - self.v_posterior) * betas * (1. - prev) / (1. - abar) + self.v_posterior * betas
            coef1 = betas * np.sqrt(prev) / (1. - abar)
            coef2 = (1. - prev) * np.sqrt(1. - betas) / (1. - abar)
        zeros = torch.zeros(self.num_timesteps)
        if self.parameterization != "v":
            self.register_buffer("sqrt_recip_alphas_cumprod", f32(np.sqrt(1. / abar)))
            self.register_buffer("sqrt_recipm1_alphas_cumprod", f32(np.sqrt(1. / abar - 1)))
        else:
            self.register_buffer("sqrt_recip_alphas_cumprod", zeros.clone())
            self.register_buffer("sqrt_recipm1_alphas_cumprod", zeros.clone())
        self.register_buffer("posterior_variance", f32(post_var))
        self.register_buffer("posterior_log_variance_clipped", f32(np.log(np.maximum(post_var, 1e-20))))
        self.register_buffer("posterior_mean_coef1", f32(coef1))
        self.register_buffer("posterior_mean_coef2", f32(coef2))
        # ddpm3d.py:173-186 (training only, not persistent): weights of the vlb term — ones for v-prediction
        if self.parameterization == "eps":
            with np.errstate(divide="ignore", invalid="ignore"):
                lvlb = betas ** 2 / (2 * post_var * (1. - betas) * (1. - abar))
        elif self.parameterization == "x0":
            lvlb = 0.5 * np.sqrt(abar) / (2. * 1 - abar)
        else:
            lvlb = np.ones_like(betas)
        lvlb = np.array(lvlb, dtype=np.float64)
        lvlb[0] = lvlb[1]
        self.register_buffer("lvlb_weights", f32(lvlb), persistent=False)

    @contextmanager
    def ema_scope(self, context=None):
        """Inside the scope the network runs on the averaged weights (ddpm3d.py:188-201).  Here: one in-place exchange of weights and
        shadows on entry and one on exit (LitEma.swap) instead of the reference's store / copy_to / restore — the training weights
        come back bit for bit and no third copy of the parameters is held; while the scope is open the shadow buffers hold the
        training weights.  The exchange bumps the version counters of the parameters, so packed operand weights, captured graphs
        and cached contexts follow.  Without use_ema: nothing happens."""
        if self.use_ema:
            self.model_ema.swap(self.model)
        try:
            yield None
        finally:
            if self.use_ema:
                self.model_ema.swap(self.model)

    def on_train_batch_end(self, *args, **kwargs):
        """ddpm3d.py:407-409: one update of the averaged weights (a loop that hands model_ema to mudg_amd.train.step.training_step
        has had it inside the optimiser's launch already and does not call this)."""
        if self.use_ema:
            self.model_ema(self.model)

    def init_from_ckpt(self, path, ignore_keys=list(), only_model=False):
        sd = torch.load(path, map_location="cpu")
        sd = sd.get("state_dict", sd)
        for k in list(sd.keys()):
            if any(k.startswith(ik) for ik in ignore_keys):
                del sd[k]
        return (self.model if only_model else self).load_state_dict(sd, strict=False)

    # ---- v-parameterisation (ddpm3d.py:239-251): elementwise with per-sample schedule scalars -> one HIP launch each
    def _combine(self, ca, x, cb, y, t):
        from mudg_amd import ops
        return ops.lincomb(x, y, ca.to(x.device)[t], cb.to(x.device)[t])

    def predict_start_from_z_and_v(self, x_t, t, v):
        return self._combine(self.sqrt_alphas_cumprod, x_t, -self.sqrt_one_minus_alphas_cumprod, v, t)

    def predict_eps_from_z_and_v(self, x_t, t, v):
        return self._combine(self.sqrt_alphas_cumprod, v, self.sqrt_one_minus_alphas_cumprod, x_t, t)

    def q_sample(self, x_start, t, noise=None):
        if noise is None:
            noise = torch.randn_like(x_start)
        return self._combine(self.sqrt_alphas_cumprod, x_start, self.sqrt_one_minus_alphas_cumprod, noise, t)

    def get_v(self, x, noise, t):
        # ddpm3d.py:310-314: sqrt(abar_t) noise - sqrt(1 - abar_t) x
        return self._combine(self.sqrt_alphas_cumprod, noise, -self.sqrt_one_minus_alphas_cumprod, x, t)

    # ---- training (reference ddpm3d.py:741-802, 1267-1300): the step itself lives in mudg_amd.train
    def p_losses(self, x_start, cond, t, noise=None, **kwargs):
        from mudg_amd.train import step
        return step.p_losses(self, x_start, cond, t, noise=noise, **kwargs)

    def configure_optimizers(self):
        """AdamW over the trainable UNet (+ image-projection: the Resampler trains through mudg_amd.train.resampler) parameters at
        `self.learning_rate`, as ddpm3d.py:1267-1300; the update runs on the HIP kernel (mudg_amd.train.step.AdamW has
        torch.optim.AdamW's semantics and defaults).  What the reference can also put into the optimiser but this build does not
        train raises instead of being dropped silently."""
        from mudg_amd.train import step
        if getattr(self, "cond_stage_trainable", False):
            raise NotImplementedError("cond_stage_trainable: the text tower has no HIP backward (frozen in every MuDG config)")
        if getattr(self, "learn_logvar", False):
            raise NotImplementedError("learn_logvar is off in every MuDG config")
        if getattr(self, "use_scheduler", False):
            raise NotImplementedError("use_scheduler: build the LambdaLR of configure_schedulers around the returned optimiser")
        params = [p for p in self.model.parameters() if p.requires_grad]
        proj = getattr(self, "image_proj_model", None)
        if getattr(self, "image_proj_model_trainable", False) and proj is not None:
            params.extend(proj.parameters())
        return step.AdamW(params, lr=getattr(self, "learning_rate", 1e-4))

    def training_step(self, batch, batch_idx=0):
        """A batch that carries `x_start` = dict(x_start=latents (B, 4, T, H, W), cond={c_crossattn, c_concat}, t=(B,) long,
        + apply_model kwargs) — the tensors the reference's shared_step / get_batch_input hand to p_losses — goes straight to
        p_losses.  Any other batch is a DATA batch (pixels, caption, class label, frame rate) and takes the reference's own route
        (ddpm3d.py:790-802): shared_step(batch, random_uncond=self.classifier_free_guidance).  Returns the loss; call .backward() and
        the optimizer as Lightning would."""
        if "x_start" not in batch:
            loss, _ = self.shared_step(batch, random_uncond=getattr(self, "classifier_free_guidance", False))
            return loss
        kw = {k: v for k, v in batch.items() if k not in ("x_start", "cond", "t", "noise")}
        loss, _ = self.p_losses(batch["x_start"], batch["cond"], batch["t"], noise=batch.get("noise"), **kw)
        return loss

    @torch.no_grad()
    def validation_step(self, batch, batch_idx=0):
        """shared_step without a graph; returns the loss_dict.  With use_ema the batch is evaluated a second time under ema_scope()
        and those entries join the dictionary with '_ema' appended to their keys (ddpm3d.py:398-405, which logs both)."""
        _, loss_dict = self.shared_step(batch)
        if not self.use_ema:
            return loss_dict
        with self.ema_scope():
            _, loss_dict_ema = self.shared_step(batch)
        return dict(loss_dict, **{key + "_ema": loss_dict_ema[key] for key in loss_dict_ema})

    def forward(self, x, c, **kwargs):
        """The training entry (ddpm3d.py:711-715): draw one timestep per sample, apply the dynamic rescale of the latents when the
        config enables it (`use_dynamic_rescale`: scale_arr[t], base_scale 0.3 / 0.7 in the MDM configs), then p_losses.
        Returns (loss, loss_dict)."""
        t = torch.randint(0, self.num_timesteps, (x.shape[0],), device=x.device).long()
        if getattr(self, "use_dynamic_rescale", False):
            x = x * extract_into_tensor(self.scale_arr.to(x.device), t, x.shape)
        return self.p_losses(x, c, t, **kwargs)

    def shared_step(self, batch, random_uncond=None, **kwargs):
        raise NotImplementedError("shared_step from a data batch (VAE-encoding the frames, CLIP towers, random conditioning dropout) is "
                                  "built for LatentVisualDiffusion only (get_batch_input): call p_losses / training_step with latents")


class LatentDiffusion(DDPM):
    def __init__(self, first_stage_config, cond_stage_config, num_timesteps_cond=None, cond_stage_key="caption",
                 cond_stage_trainable=False, cond_stage_forward=None, conditioning_key=None, uncond_prob=0.2,
                 uncond_type="empty_seq", scale_factor=1.0, scale_by_std=False, encoder_type="2d", only_model=False,
                 noise_strength=0, use_dynamic_rescale=False, base_scale=0.7, turning_step=400, interp_mode=False,
                 fps_condition_type="fs", perframe_ae=False, logdir=None, rand_cond_frame=False,
                 en_and_decode_n_samples_a_time=None, *args, **kwargs):
        self.num_timesteps_cond = default(num_timesteps_cond, 1)
        self.scale_by_std = scale_by_std
        assert self.num_timesteps_cond <= kwargs["timesteps"]
        if self.num_timesteps_cond != 1:
            raise NotImplementedError("num_timesteps_cond > 1 is not on the MuDG path")
        ckpt_path = kwargs.pop("ckpt_path", None)
        ignore_keys = kwargs.pop("ignore_keys", [])
        super().__init__(conditioning_key=default(conditioning_key, "crossattn"), *args, **kwargs)
        self.cond_stage_trainable, self.cond_stage_key = cond_stage_trainable, cond_stage_key
        self.noise_strength, self.use_dynamic_rescale = noise_strength, use_dynamic_rescale
        self.interp_mode, self.fps_condition_type, self.perframe_ae = interp_mode, fps_condition_type, perframe_ae
        self.logdir, self.rand_cond_frame = logdir, rand_cond_frame
        self.en_and_decode_n_samples_a_time = en_and_decode_n_samples_a_time
        ddc = _cfg_get(_cfg_get(first_stage_config, "params"), "ddconfig")
        mult = _cfg_get(ddc, "ch_mult")
        self.num_downs = len(mult) - 1 if mult is not None else 0
        if scale_by_std:
            self.register_buffer("scale_factor", torch.tensor(scale_factor))
        else:
            self.scale_factor = scale_factor
        self.base_scale, self.turning_step = base_scale, turning_step
        if use_dynamic_rescale:
            self._register_scale_arr()
        self.instantiate_first_stage(first_stage_config)
        self.instantiate_cond_stage(cond_stage_config)
        self.first_stage_config, self.cond_stage_config = first_stage_config, cond_stage_config
        self.clip_denoised = False
        self.cond_stage_forward = cond_stage_forward
        assert encoder_type in ["2d", "3d"]
        self.encoder_type = encoder_type
        self.uncond_prob, self.classifier_free_guidance = uncond_prob, uncond_prob > 0
        assert uncond_type in ["zero_embed", "empty_seq"]
        self.uncond_type = uncond_type
        self.restarted_from_ckpt = False
        if ckpt_path is not None:
            self.init_from_ckpt(ckpt_path, ignore_keys, only_model=only_model)
            self.restarted_from_ckpt = True

    def _register_scale_arr(self):
        # ddpm3d.py:522-527: 1 -> base_scale over `turning_step` steps, then flat (length turning_step + T)
        arr = np.concatenate((np.linspace(1.0, self.base_scale, self.turning_step),
                              np.full(self.num_timesteps, self.base_scale)))
        self.register_buffer("scale_arr", torch.tensor(arr, dtype=torch.float32, device="cpu"))

    def rebuild_schedules(self, device=None):
        """Recompute every schedule buffer from the stored hyper-parameters (they are pure functions of the config).
        Needed after constructing under torch.device('meta') + to_empty(), where buffers carry no data."""
        self.register_schedule(given_betas=self.given_betas, beta_schedule=self.beta_schedule,
                               timesteps=self.timesteps, linear_start=self.linear_start,
                               linear_end=self.linear_end, cosine_s=self.cosine_s)
        if self.use_dynamic_rescale:
            self._register_scale_arr()
        if device is not None:
            for name, buf in list(self.named_buffers(recurse=False)):
                self.register_buffer(name, buf.to(device))
        return self

    def _freeze(self, model):
        model = model.eval()
        model.train = disabled_train.__get__(model)
        for p in model.parameters():
            p.requires_grad = False
        return model

    def instantiate_first_stage(self, config):
        self.first_stage_model = self._freeze(instantiate_from_config(config))

    def instantiate_cond_stage(self, config):
        model = instantiate_from_config(config)
        self.cond_stage_model = model if self.cond_stage_trainable else self._freeze(model)

    def get_learned_conditioning(self, c):
        """Text embedding via the configured cond stage (OpenCLIP in MuDG's configs — outside this path's scope; any
        module with .encode / __call__ returning (B, 77, D) works)."""
        m = self.cond_stage_model
        if self.cond_stage_forward is None:
            return m.encode(c) if callable(getattr(m, "encode", None)) else m(c)
        return getattr(m, self.cond_stage_forward)(c)

    def get_first_stage_encoding(self, encoder_posterior, noise=None):
        """scale_factor * posterior.sample() (ddpm3d.py:611-618); the scale rides in the sampling kernel."""
        if isinstance(encoder_posterior, torch.Tensor):
            from mudg_amd import ops
            return ops.lincomb(encoder_posterior, encoder_posterior,
                               torch.full((encoder_posterior.shape[0],), float(self.scale_factor), device=encoder_posterior.device),
                               torch.zeros(encoder_posterior.shape[0], device=encoder_posterior.device))
        return encoder_posterior.sample(noise=noise, scale=float(self.scale_factor))

    @torch.no_grad()
    def encode_first_stage(self, x):
        """(B, 3, T, H, W) or (N, 3, H, W) pixels -> scaled latents (ddpm3d.py:620-644).  With perframe_ae the
        reference encodes and samples frame by frame; the CPU noise draws happen in that same order here, while the
        encoder itself runs on batches of frames (they are independent)."""
        five = x.dim() == 5
        if five:
            b, c, t, h, w = x.shape
            frames = x.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w)
        else:
            frames = x
        posterior = self.first_stage_model.encode(frames)
        n, c2, hh, ww = posterior.parameters.shape
        if self.perframe_ae:
            noise = torch.cat([torch.randn((1, c2 // 2, hh, ww)) for _ in range(n)], 0)
        else:
            noise = torch.randn((n, c2 // 2, hh, ww))
        z = self.get_first_stage_encoding(posterior, noise=noise)
        if five:
            z = z.reshape(b, t, c2 // 2, hh, ww).permute(0, 2, 1, 3, 4)
        return z

    @torch.no_grad()
    def decode_core(self, z, **kwargs):
        """z (B, C, T, h, w) or (N, C, h, w) latents -> pixels; divides by scale_factor and decodes frame by frame
        (perframe_ae) — every frame is independent, so batching only changes launch counts."""
        from mudg_amd.engine import vae
        return vae.decode_latents(self.first_stage_model, z, 1.0 / float(self.scale_factor), self.perframe_ae)

    def decode_first_stage(self, z, **kwargs):
        return self.decode_core(z, **kwargs)

    differentiable_decode_first_stage = decode_first_stage

    @torch.no_grad()
    def sample_log(self, cond, batch_size, ddim, ddim_steps, **kwargs):
        """ddpm3d.py:996-1005: a DDIM run of `ddim_steps` steps over (channels, temporal_length, *image_size) latents; every other
        keyword argument goes to DDIMSampler.sample.  Returns (samples, intermediates)."""
        if not ddim:
            raise NotImplementedError("sample_log(ddim=False): the ancestral sampler is not on the MuDG path; pass ddim_steps")
        from lvdm.models.samplers.ddim import DDIMSampler
        shape = (self.channels, self.temporal_length, *self.image_size)
        return DDIMSampler(self).sample(ddim_steps, batch_size, shape, cond, verbose=False, **kwargs)

    @torch.no_grad()
    def _get_denoise_row_from_list(self, samples, desc=""):
        """ddpm3d.py:804-827: decode every recorded latent and lay the results out as torchvision's make_grid does with its default
        padding: images (n, b, c, h, w) one row per sample, n columns; videos (n, b, c, t, h, w) one row per (sample, recorded
        step), t columns."""
        rows = torch.stack([self.decode_first_stage(zd.to(self.device)) for zd in samples])
        if rows.dim() == 5:
            n = rows.shape[0]
            return _make_grid(rows.permute(1, 0, 2, 3, 4).flatten(0, 1), nrow=n)
        if rows.dim() == 6:
            t = rows.shape[3]
            cells = rows.permute(1, 0, 3, 2, 4, 5).flatten(0, 2)          # (b n t) c h w
            return _make_grid(cells, nrow=t)
        raise ValueError(f"decoded latents of {rows.dim() - 1} dimensions")

    def apply_model(self, x_noisy, t, cond, **kwargs):
        if not isinstance(cond, dict):
            cond = {("c_concat" if self.model.conditioning_key == "concat" else "c_crossattn"):
                    cond if isinstance(cond, list) else [cond]}
        label = kwargs.get("class_label", None)
        if label is None:
            raise TypeError("apply_model needs class_label=(B, 1) (0 colour / 500 depth / 1 semantic)")
        out = self.model(x_noisy, t, label[:, 0], **cond, **kwargs)
        return out[0] if isinstance(out, tuple) else out


class LatentVisualDiffusion(LatentDiffusion):
    def __init__(self, img_cond_stage_config, image_proj_stage_config, freeze_embedder=True,
                 image_proj_model_trainable=True, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.image_proj_model_trainable = image_proj_model_trainable
        self.embedder = instantiate_from_config(img_cond_stage_config)
        if freeze_embedder:
            self.embedder = self._freeze(self.embedder)
        self.image_proj_model = instantiate_from_config(image_proj_stage_config)
        if not image_proj_model_trainable:
            self.image_proj_model = self._freeze(self.image_proj_model)

    # ---- training from a data batch (reference ddpm3d.py:1056-1149): everything under it already runs on HIP; this joins it
    def _batch_keys(self, with_fs=True):
        keys = [self.first_stage_key, "sparse_frames", "sparse_depth", "class_label", self.cond_stage_key]
        if with_fs:
            keys.append("frame_stride" if self.fps_condition_type == "fs" else "fps")
        return keys

    def _require_batch(self, batch, keys):
        missing = [k for k in keys if k not in batch]
        if missing:
            raise NotImplementedError(f"the batch lacks the data entries {missing}: a data batch carries {self._batch_keys()} "
                                      "(making them from Waymo items is the dataset's work, not built here); latents go to "
                                      "p_losses / training_step(dict(x_start=..., cond=..., t=...))")

    @staticmethod
    def get_input(batch, k):
        return batch[k].to(memory_format=torch.contiguous_format).float()

    def _uncond_draw(self, n, device):
        """The one random draw of the conditioning dropout (ddpm3d.py:1084): B uniforms made ON the device, where they stay."""
        return torch.rand(n, device=device)

    @torch.no_grad()
    def _encode_streams(self, x, sparse_x, sparse_depth):
        """The three encode_first_stage calls of get_batch_input as one: the frames of all streams go through the encoder as one
        frame batch, the posterior noise is drawn on the CPU generator in the reference's order (dense, sparse colour, sparse depth;
        frame by frame when perframe_ae), and one launch samples all three posteriors straight into z (B, 4, T, h, w) and
        c_concat (B, 8, T, h, w) = [sparse_z | sparse_depth_z]."""
        from mudg_amd import ops
        from mudg_amd.engine import vae
        if x.dim() != 5 or x.shape != sparse_x.shape or x.shape != sparse_depth.shape:
            raise ValueError(f"get_batch_input: the three streams must be (B, 3, T, H, W) clips of one shape, got {tuple(x.shape)}, "
                             f"{tuple(sparse_x.shape)}, {tuple(sparse_depth.shape)}")
        b, t = x.shape[0], x.shape[2]
        moments = vae.encode_moments(self.first_stage_model, [x, sparse_x, sparse_depth])
        n, c2, hh, ww = moments[0].shape
        if self.perframe_ae:
            noise = torch.cat([torch.randn((1, c2 // 2, hh, ww)) for _ in range(3 * n)], 0)
        else:
            noise = torch.cat([torch.randn((n, c2 // 2, hh, ww)) for _ in range(3)], 0)
        # the one host-to-device transfer of get_batch_input: from page-locked memory and asynchronous, so the host does not wait
        noise = noise.reshape(3, n, c2 // 2, hh, ww).pin_memory().to(x.device, non_blocking=True)
        return ops.posterior_assemble(*moments, noise, b, t, float(self.scale_factor))

    @torch.no_grad()
    def _cond_dropout(self, random_num, cond_emb, null_prompt, sparse_x, frame):
        """prompt_mask / input_mask of ddpm3d.py:1087-1100 applied in one launch: (prompt rows, the image the tower sees)."""
        from mudg_amd import ops
        return ops.cond_dropout(random_num, self.uncond_prob, cond_emb.detach(), null_prompt, sparse_x, frame)

    def get_batch_input(self, batch, random_uncond, return_first_stage_outputs=False, return_original_cond=False,
                        return_fs=False, return_cond_frame=False, return_original_input=False, return_sparse_input=False,
                        return_class_label=False, **kwargs):
        """A data batch -> [z, sparse_z, cond, (xrec), (cond_input), (fs), (cond_frame), (x), (sparse_x), (class_label)] as the
        reference's method of the same name.  With random_uncond the text / both / the key-frame image are dropped for
        r < p / p <= r < 2p / 2p <= r < 3p (p = uncond_prob); the draw and the masks never leave the device.  `sparse_z` is the
        view c_concat[:, :4] of the assembled conditioning."""
        self._require_batch(batch, self._batch_keys(with_fs=return_fs))
        x = self.get_input(batch, self.first_stage_key)
        sparse_x = self.get_input(batch, "sparse_frames")
        class_label = self.get_input(batch, "class_label")
        sparse_depth = self.get_input(batch, "sparse_depth")
        if self.encoder_type != "2d":
            raise NotImplementedError("encoder_type '3d' is not on the MuDG path")

        z, latent_cond = self._encode_streams(x, sparse_x, sparse_depth)
        sparse_z = latent_cond[:, :z.shape[1]]

        cond_input = batch[self.cond_stage_key]
        with torch.set_grad_enabled(torch.is_grad_enabled() and self.cond_stage_trainable):
            if isinstance(cond_input, (dict, list)):
                cond_emb = self.get_learned_conditioning(cond_input)
            else:
                cond_emb = self.get_learned_conditioning(cond_input.to(self.device))
            null_prompt = self.get_learned_conditioning([""])
        if random_uncond:
            random_num = self._uncond_draw(x.size(0), x.device)
        else:
            random_num = torch.ones(x.size(0), device=x.device)         # nothing dropped: full text and image conditioning

        cond_frame_index = 0
        if self.rand_cond_frame:
            assert self.rand_cond_frame is False, "random condition frame is not supported"
        prompt_imb, img = self._cond_dropout(random_num, cond_emb, null_prompt, sparse_x, cond_frame_index)
        with torch.no_grad():
            img_emb = self.embedder(img)                                    # b l c
        with torch.set_grad_enabled(torch.is_grad_enabled() and self.image_proj_model_trainable):
            img_emb = self.image_proj_model(img_emb)

        cond = {}
        if self.model.conditioning_key == "hybrid":
            if self.interp_mode:
                # starting frame + (L - 2 empty frames) + ending frame
                img_cat_cond = torch.zeros_like(z)
                img_cat_cond[:, :, 0] = z[:, :, 0]
                img_cat_cond[:, :, -1] = z[:, :, -1]
            else:
                img_cat_cond = latent_cond
            cond["c_concat"] = [img_cat_cond]                               # b c t h w
        cond["c_crossattn"] = [torch.cat([prompt_imb, img_emb], dim=1)]     # along the sequence

        out = [z, sparse_z, cond]
        if return_first_stage_outputs:
            out.append(self.decode_first_stage(z))
        if return_original_cond:
            out.append(cond_input)
        if return_fs:
            out.append(self.get_input(batch, "frame_stride" if self.fps_condition_type == "fs" else "fps"))
        if return_cond_frame:
            out.append(x[:, :, cond_frame_index, ...].unsqueeze(2))
        if return_original_input:
            out.append(x)
        if return_sparse_input:
            out.append(sparse_x)
        if return_class_label:
            out.append(class_label)
        return out

    @torch.no_grad()
    def log_images(self, batch, sample=True, ddim_steps=50, ddim_eta=1., plot_denoise_rows=False, unconditional_guidance_scale=1.0,
                   mask=None, **kwargs):
        """What the training loop's ImageLogger logs (ddpm3d.py:1186-1265), for the FIRST sample of the batch: `image_condition` (its
        key frame), `reconst` (decode of its encoded clip), `condition` (caption + "_fs=<frame rate>"), and with `sample` the
        decoded `samples` of a DDIM run from the batch's conditioning under ema_scope() — guided against the unconditional branch
        (null prompt by uncond_type, the all-zero image through embedder and image_proj_model, c_concat shared) when
        unconditional_guidance_scale != 1 — plus, with plot_denoise_rows, `denoise_row` (the recorded pred_x0 list decoded and laid
        out by _get_denoise_row_from_list).  x0=z, fs and class_label ride to the sampler among the keyword arguments; so does
        everything else the caller passes (x_T=..., and split=..., which the UNet ignores), as in the reference.
        One stated difference: the one-sample cut is made on a shallow copy, the caller's batch is not modified."""
        sampled_img_num = 1
        batch = {key: (value if key == "tasks" else value[:sampled_img_num]) for key, value in batch.items()}
        use_ddim = ddim_steps is not None
        log = dict()
        z, sparse_z, c, xrec, xc, fs, cond_x, sparse, class_label = self.get_batch_input(
            batch, random_uncond=False, return_first_stage_outputs=True, return_original_cond=True, return_fs=True,
            return_cond_frame=True, return_sparse_input=True, return_class_label=True)
        n = xrec.shape[0]
        log["image_condition"] = cond_x
        log["reconst"] = xrec
        log["condition"] = [content + "_fs=" + str(rate) for content, rate in zip(xc, fs.tolist())]
        kwargs.update({"fs": fs.long()})
        kwargs.update({"class_label": class_label})
        if not sample:
            return log
        uc = None
        if unconditional_guidance_scale != 1.0:
            c_emb, c_cat = (c["c_crossattn"][0], c["c_concat"][0] if "c_concat" in c else None) if isinstance(c, dict) else (c, None)
            if self.uncond_type == "empty_seq":
                uc_prompt = self.get_learned_conditioning(n * [""])
            elif self.uncond_type == "zero_embed":
                uc_prompt = torch.zeros_like(c_emb)
            uc_img = self.image_proj_model(self.embedder(torch.zeros_like(xrec[:, :, 0])))      # the all-zero image: b c h w -> b l c
            uc = torch.cat([uc_prompt, uc_img], dim=1)
            if isinstance(c, dict):                      # hybrid: the latents the UNet reads beside x are those of the conditional pass
                uc = {"c_concat": [c_cat], "c_crossattn": [uc]}
        with self.ema_scope("Plotting"):
            samples, z_denoise_row = self.sample_log(cond=c, batch_size=n, ddim=use_ddim, ddim_steps=ddim_steps, eta=ddim_eta,
                                                     unconditional_guidance_scale=unconditional_guidance_scale,
                                                     unconditional_conditioning=uc, x0=z, **kwargs)
        log["samples"] = self.decode_first_stage(samples)
        if plot_denoise_rows:
            log["denoise_row"] = self._get_denoise_row_from_list(z_denoise_row["pred_x0"])
        return log

    def shared_step(self, batch, random_uncond=None, **kwargs):
        """ddpm3d.py:1056-1062: get_batch_input, then forward() (random t, dynamic rescale, p_losses) with fs / sparse_x /
        class_label among the keyword arguments.  random_uncond None = self.classifier_free_guidance.  Returns (loss, loss_dict)."""
        if random_uncond is None:
            random_uncond = self.classifier_free_guidance
        x, sparse_x, c, fs, class_label = self.get_batch_input(batch, random_uncond=random_uncond, return_fs=True,
                                                               return_class_label=True)
        kwargs.update({"fs": fs.long()})
        kwargs.update({"sparse_x": sparse_x})
        kwargs.update({"class_label": class_label})
        return self(x, c, **kwargs)

