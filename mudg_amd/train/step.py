"""The training step around the UNet: v-prediction loss (p_losses), gradient-norm clipping and AdamW on HIP kernels, data-parallel
gradient all-reduce.

Reference: lvdm/models/ddpm3d.py:741-802 (p_losses), :1267-1300 (configure_optimizers -> torch.optim.AdamW(params, lr)),
main/utils_train.py:126-137 (data-parallel strategy: one process per GPU, gradients averaged after backward)."""
import torch

from . import functions as F_
from . import kernels as K


def _logvar_on(model, dev):
    """model.logvar — a plain tensor on the host, as in the reference — on the device: uploaded once (a blocking copy) and again only
    when it was replaced or written, so that a step does not wait for the device."""
    src = model.logvar
    if src.device == dev:
        return src
    hit = model.__dict__.get("_mudg_logvar")
    if hit is None or hit[0] is not src or hit[1] != src._version or hit[2].device != dev:
        hit = (src, src._version, src.to(dev))
        model.__dict__["_mudg_logvar"] = hit
    return hit[2]


def p_losses(model, x_start, cond, t, noise=None, **kwargs):
    """LatentDiffusion.p_losses: q_sample -> UNet (with an autograd graph) -> target by parameterisation -> per-sample MSE ->
    loss = l_simple_weight * mean(mse / exp(logvar_t) + logvar_t) + original_elbo_weight * mean(lvlb_weights[t] * mse).
    Returns (loss, loss_dict) with the reference's dictionary keys."""
    if getattr(model, "learn_logvar", False):
        raise NotImplementedError("learn_logvar is off in every MuDG config")
    if noise is None:
        # offset noise (ddpm3d.py:742-747): the per-(sample, channel, frame) term is drawn FIRST, then the full-size noise — the
        # reference's order, so that a seeded run draws the same numbers
        offset = None
        if model.noise_strength > 0:
            b, c, f = x_start.shape[:3]
            offset = torch.randn(b, c, f, 1, 1, device=x_start.device)
        noise = torch.randn_like(x_start)
        if offset is not None:
            noise = noise + model.noise_strength * offset
    x_start, noise = x_start.float().contiguous(), noise.float().contiguous()
    x_noisy = model.q_sample(x_start=x_start, t=t, noise=noise)
    model_output = model.apply_model(x_noisy, t, cond, **kwargs)
    if model.parameterization == "x0":
        target = x_start
    elif model.parameterization == "eps":
        target = noise
    elif model.parameterization == "v":
        target = model.get_v(x_start, noise, t)
    else:
        raise NotImplementedError(model.parameterization)
    dev = x_start.device
    b = x_start.shape[0]
    logvar_t = _logvar_on(model, dev)[t].float()
    lvlb_t = model.lvlb_weights.to(dev)[t].float()
    # per-sample coefficients of the mse (host-sized vectors of B numbers, like the DDIM step's coefficients)
    w = (model.l_simple_weight / torch.exp(logvar_t) + model.original_elbo_weight * lvlb_t) / b
    weighted, mse_b = F_.WeightedMSE.apply(model_output.float(), target, w)
    loss = weighted + model.l_simple_weight * logvar_t.mean()          # (a device scalar: no host round trip; 0 in every MuDG config)
    prefix = "train" if model.training else "val"
    loss_dict = {f"{prefix}/loss_simple": mse_b.mean(), f"{prefix}/loss_vlb": (lvlb_t * mse_b).mean(), f"{prefix}/loss": loss.detach()}
    return loss, loss_dict


class AdamW(torch.optim.Optimizer):
    """torch.optim.AdamW semantics (decoupled weight decay, bias correction) with the update done on the HIP kernel, fp32 moments
    next to fp32 master weights.  All tensors of a parameter group are updated by ONE launch (mudg_adamw_multi over a device table
    of (parameter, gradient, moment, moment, count) chunks; the table is rebuilt only when a tensor moved), instead of one launch
    per tensor — 1520 for the UNet.  After the update every parameter's autograd version counter is bumped: the kernel writes
    through raw pointers, and the inference side (packed operand weights, captured hipGraphs, cached K / V^T of a prepared
    context) recognises changed weights by (data_ptr, _version).

    step(ema=LitEma): the averaged weights are updated in the SAME launch (mudg_adamw_ema_multi: the average reads the new value out
    of the register it was computed in — one read and one write of the shadow on top of the AdamW traffic).  `num_updates` advances
    once per step; parameters the average does not track take the plain launch, tracked parameters the optimiser did not step
    (no gradient) get their shadow moved by mudg_ema_multi: after the call every shadow has had exactly LitEma.forward's update.
    The average names its parameters by identity (those of the model it was built on): an optimiser that holds none of them is an
    error, not a silent plain step.

    step(scaler=LossScaler): the launches become mudg_adamw_scaled_multi / mudg_adamw_scaled_ema_multi.  They consume the SCALED
    gradient as (g * inv_scale) * clip coefficient (the coefficient of the scaler's norm pass, which must have run), skip the
    update on the device when that pass found an overflow, and take their bias corrections from the scaler record's count of
    steps actually taken: the host makes no decision that depends on the flag and never waits for it.  state["step"] then counts
    ATTEMPTS; state_dict() reports the taken count (one device read there) and load_state_dict() restores it, so a resumed run
    has the same bias corrections.  One count serves the whole optimiser: parameters at different step counts (the per-tensor
    fallback) raise NotImplementedError under a scaler.  Version counters are bumped on a skipped step too (a spurious refresh of
    a weight cache is harmless; not bumping would need the flag)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._tables = {}                                 # group index -> (key, device table, chunk count)
        self._ema_tables = {}                             # group index -> (key, fused table, count, plain table, count)
        self._scaler = None                               # the LossScaler whose record holds this optimiser's taken-step count

    def _bind(self, scaler):
        """Before the first scaled launch (and again after load_state_dict): every stepped parameter must be at the same step
        count, and that count — all of them taken, as far as the host knows — becomes the record's."""
        seen = {self.state[p].get("step", 0) for group in self.param_groups for p in group["params"] if p.grad is not None}
        if len(seen) > 1:
            raise NotImplementedError("AdamW.step(scaler=...): the parameters are at different step counts "
                                      f"({sorted(seen)[:4]}); the scaler record holds ONE count of taken steps for the bias "
                                      "corrections, so the per-tensor fallback cannot run under a loss scale")
        if seen and self._scaler is not scaler:
            scaler._set_taken(seen.pop(), next(p for group in self.param_groups for p in group["params"]).device)
            self._scaler = scaler

    def state_dict(self):
        sd = super().state_dict()
        if self._scaler is not None:                      # attempts -> steps taken (a device read: checkpoints only)
            taken = self._scaler.taken_steps()
            sd["state"] = {k: (dict(st, step=taken) if "step" in st else st) for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._scaler = None                               # the next scaled step writes the loaded count into the record

    def _table_ema(self, gi, ps, shadows):
        """Two tables for a group stepped with an average: rows (p, g, m, v, shadow, count) for the tracked parameters and the
        rows of _table for the rest (either may be empty: None)."""
        key = tuple((p.data_ptr(), p.grad.data_ptr(), self.state[p]["exp_avg"].data_ptr(), self.state[p]["exp_avg_sq"].data_ptr(),
                     p.numel(), shadows[id(p)].data_ptr() if id(p) in shadows else 0) for p in ps)
        hit = self._ema_tables.get(gi)
        if hit is not None and hit[0] == key:
            return hit[1:]
        cols = lambda p: (p, p.grad, self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"])
        fused = [cols(p) + (shadows[id(p)],) for p in ps if id(p) in shadows]
        plain = [cols(p) for p in ps if id(p) not in shadows]
        hit = (key,) + (K.chunk_table(fused) if fused else (None, 0)) + (K.chunk_table(plain) if plain else (None, 0))
        self._ema_tables[gi] = hit
        return hit[1:]

    def _table(self, gi, ps):
        # the table bakes in the addresses of the moments too: load_state_dict (or any reassignment of state[p][...]) replaces them
        key = tuple((p.data_ptr(), p.grad.data_ptr(), self.state[p]["exp_avg"].data_ptr(), self.state[p]["exp_avg_sq"].data_ptr(),
                     p.numel()) for p in ps)
        hit = self._tables.get(gi)
        if hit is not None and hit[0] == key:
            return hit[1], hit[2]
        table, n = K.chunk_table([(p, p.grad, self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"]) for p in ps])
        self._tables[gi] = (key, table, n)
        return table, n

    @torch.no_grad()
    def step(self, closure=None, ema=None, scaler=None):
        loss = None
        if scaler is not None and not scaler.enabled:
            scaler = None
        shadows, omd, averaged = None, None, set()
        if ema is not None:
            shadows = ema.shadow_map()
            if shadows and not any(id(p) in shadows for group in self.param_groups for p in group["params"]):
                raise RuntimeError("AdamW.step(ema=...): none of the optimiser's parameters is tracked by this average — it was built "
                                   "on another model instance")
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if scaler is not None:
            scaler._check_step(self)
            self._bind(scaler)
        for gi, group in enumerate(self.param_groups):
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            steps = set()
            for p in ps:
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("mudg AdamW updates contiguous fp32 parameters on the GPU")
                if p.grad.dtype != torch.float32 or not p.grad.is_contiguous():
                    p.grad = p.grad.float().contiguous()
                st = self.state[p]
                if not st:
                    st["step"], st["exp_avg"], st["exp_avg_sq"] = 0, torch.zeros_like(p), torch.zeros_like(p)
                st["step"] += 1
                steps.add(st["step"])
            hyper = dict(lr=group["lr"], betas=group["betas"], eps=group["eps"], weight_decay=group["weight_decay"])
            if ema is not None and len(steps) == 1:
                tracked = [p for p in ps if id(p) in shadows]
                if tracked:
                    ema._check([(p, shadows[id(p)]) for p in tracked])
                fused, nf, plain, npl = self._table_ema(gi, ps, shadows)
                step = steps.pop()
                if omd is None:                           # after every check that can raise: a failed step leaves num_updates alone
                    omd = ema.begin_update()
                if nf and scaler is not None:
                    K.adamw_scaled_ema_multi_(fused, nf, scaler._rec, scaler._stat, one_minus_decay=omd, **hyper)
                elif nf:
                    K.adamw_ema_multi_(fused, nf, step=step, one_minus_decay=omd, **hyper)
                if npl and scaler is not None:
                    K.adamw_scaled_multi_(plain, npl, scaler._rec, scaler._stat, **hyper)
                elif npl:
                    K.adamw_multi_(plain, npl, step=step, **hyper)
                for p in tracked:
                    averaged.add(id(p))
                    torch.autograd.graph.increment_version(shadows[id(p)])
            elif len(steps) == 1:
                table, n = self._table(gi, ps)
                if scaler is not None:
                    K.adamw_scaled_multi_(table, n, scaler._rec, scaler._stat, **hyper)
                else:
                    K.adamw_multi_(table, n, step=steps.pop(), **hyper)
            else:                                         # parameters that joined the group at different times: one launch each
                for p in ps:
                    st = self.state[p]
                    K.adamw_(p.data, p.grad, st["exp_avg"], st["exp_avg_sq"], step=st["step"], **hyper)
            for p in ps:
                torch.autograd.graph.increment_version(p)
        if ema is not None:                               # tracked parameters no fused launch covered: the average alone
            if omd is None:
                omd = ema.begin_update()
            ema.update([(p, s) for p, s in ema.pairs() if id(p) not in averaged], omd)
        return loss


class GradientClipper:
    """torch.nn.utils.clip_grad_norm_(params, max_norm) (2-norm) as the reference's trainer applies it between backward and the
    optimiser step (configs/stage2-1024_mdm_waymo/config.yaml: gradient_clip_val 0.5, gradient_clip_algorithm norm), on HIP
    kernels and without a host round trip: the norm and the clip coefficient stay on the device.  The chunk table is rebuilt
    only when a gradient tensor moved."""

    def __init__(self, params, max_norm):
        self.params = [p for p in params if p.requires_grad]
        self.max_norm = float(max_norm)
        self._key, self._table, self._partial = None, None, None

    @torch.no_grad()
    def __call__(self):
        """Scales the gradients in place; returns the device tensor [norm, coefficient]."""
        from .. import hip
        grads = [p.grad for p in self.params if p.grad is not None]
        if not grads:
            return None
        for g in grads:
            if not g.is_cuda or g.dtype != torch.float32 or not g.is_contiguous():
                raise RuntimeError("GradientClipper works on contiguous fp32 gradients on the GPU")
        key = tuple((g.data_ptr(), g.numel()) for g in grads)
        dev = grads[0].device
        if key != self._key:
            self._table, n = K.chunk_table([(g,) for g in grads])
            self._partial = torch.empty(n, dtype=torch.float64, device=dev)
            self._key = key
        out = torch.empty(2, dtype=torch.float32, device=dev)
        hip.check(hip.lib().mudg_clip_grad_norm(self._table.data_ptr(), self._table.shape[0], self._partial.data_ptr(), self.max_norm,
                                                out.data_ptr(), torch.cuda.current_stream().cuda_stream), "mudg_clip_grad_norm")
        return out


class LossScaler:
    """torch.amp.GradScaler for the fp16 operand build, on the device from end to end (the reference trains with precision: 16,
    i.e. a GradScaler with its defaults: scale 2^16, x2 every 2000 good steps, x0.5 and a skipped optimiser step on overflow).
    Why: an output gradient below 2^-25 becomes an exact zero as an fp16 MFMA operand and everything upstream of it gets no
    gradient; multiplied by the scale it is in range, and the optimiser divides the scale out again in fp32.

    The state is ONE 16-byte device record — fp32 scale, int32 growth tracker, the overflow flag of the current step, an int32
    count of steps actually taken — that only kernels read and write:
        scale(loss)        loss * scale, a device multiply that autograd carries
        norm_pass(...)     mudg_scaled_grad_norm: [norm of the UNSCALED gradients, clip coefficient] and the overflow flag (set
                           iff any gradient is inf or NaN); no write pass, the gradients STAY SCALED in .grad
        optimizer.step(scaler=self)   unscales, clips, skips and counts on the device (AdamW above)
        update()           mudg_loss_scale_update: back off on overflow, grow after growth_interval good steps
    unscale_(tensors) is an explicit extra launch for callers who want to LOOK at unscaled gradients (pass copies: the
    optimiser unscales by itself and refuses gradients that were already unscaled).  get_scale(), state_dict() and
    taken_steps() read the device and are for logging and checkpoints.  state_dict() / load_state_dict() use torch's keys, so a
    scaler state out of a Lightning checkpoint loads here and one made here loads into torch.  enabled=False makes every method
    the identity (and step(scaler=...) the plain step): one training script serves all builds.

    Several ranks: the norm pass runs after the gradient all-reduce, and a non-finite value on any rank is non-finite in the
    averaged bucket on every rank, so all ranks skip together without a collective of their own."""

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True):
        if enabled and not (growth_factor > 1.0 and 0.0 < backoff_factor < 1.0 and growth_interval > 0 and init_scale > 0.0):
            raise ValueError("LossScaler: growth_factor > 1, 0 < backoff_factor < 1, growth_interval > 0, init_scale > 0")
        self.enabled = bool(enabled)
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self._init_scale, self._init_tracker, self._init_taken = float(init_scale), 0, 0
        self._rec, self._scale = None, None               # the record as int32 [4]; its first word as an fp32 scalar view
        self._stat = None                                 # [norm, coefficient] of this step's norm pass
        self._key, self._table, self._partial = None, None, None
        self._unscaled = set()                            # addresses unscale_() has written since the last update()

    def _record(self, device):
        if self._rec is None:
            host = torch.zeros(4, dtype=torch.int32)
            host.view(torch.float32)[0] = self._init_scale
            host[1], host[3] = self._init_tracker, self._init_taken
            self._rec = host.to(device)
            self._scale = self._rec.view(torch.float32)[0]
        elif self._rec.device != torch.device(device):
            raise RuntimeError(f"LossScaler: the record lives on {self._rec.device}, got a tensor on {device}")
        return self._rec

    def _set_taken(self, n, device):
        self._record(device)[3].fill_(int(n))

    def scale(self, loss):
        if not self.enabled:
            return loss
        self._record(loss.device)
        return loss * self._scale

    def _chunks(self, tensors):
        """(key, device table of (address, count) rows) over `tensors`."""
        for g in tensors:
            if not g.is_cuda or g.dtype != torch.float32 or not g.is_contiguous():
                raise RuntimeError("LossScaler works on contiguous fp32 gradients on the GPU")
        return tuple((g.data_ptr(), g.numel()) for g in tensors), K.chunk_table([(g,) for g in tensors])[0]

    @torch.no_grad()
    def norm_pass(self, params, max_norm=None):
        """The scaled norm pass over the gradients of `params` (after backward and the all-reduce, once per optimiser step).
        Returns the device tensor [unscaled norm, clip coefficient]; max_norm None: the coefficient is 1.  The chunk table is
        rebuilt only when a gradient tensor moved."""
        if not self.enabled:
            return None
        grads = [p.grad for p in params if p.grad is not None]
        if not grads:
            return None
        rec = self._record(grads[0].device)
        key = tuple((g.data_ptr(), g.numel()) for g in grads)
        if key != self._key:
            _, self._table = self._chunks(grads)
            self._partial = torch.empty(self._table.shape[0], dtype=torch.float64, device=grads[0].device)
            self._key = key
        if max_norm is not None and not max_norm > 0:
            raise ValueError("LossScaler.norm_pass: max_norm must be positive (None: no clipping)")
        self._stat = K.scaled_grad_norm(self._table, self._table.shape[0], self._partial, None if max_norm is None else float(max_norm), rec)
        return self._stat

    @torch.no_grad()
    def unscale_(self, tensors):
        """g <- g * float(1 / scale) in place on every tensor (or parameter's .grad) given: one extra launch, for inspection."""
        if not self.enabled:
            return
        grads = [t.grad if isinstance(t, torch.nn.Parameter) else t for t in tensors]
        grads = [g for g in grads if g is not None]
        if not grads:
            return
        rec = self._record(grads[0].device)
        _, table = self._chunks(grads)
        K.unscale_multi_(table, table.shape[0], rec)
        self._unscaled.update(g.data_ptr() for g in grads)

    def _check_step(self, optimizer):
        if self._stat is None:
            raise RuntimeError("optimizer.step(scaler=...): run scaler.norm_pass(params, max_norm) after backward first — it finds "
                               "the overflow flag and the clip coefficient the step reads")
        if self._unscaled and any(p.grad is not None and p.grad.data_ptr() in self._unscaled
                                  for group in optimizer.param_groups for p in group["params"]):
            raise RuntimeError("optimizer.step(scaler=...): these gradients were already unscaled by scaler.unscale_(); the step "
                               "unscales by itself — call unscale_ on copies")

    def update(self):
        """After optimizer.step(scaler=...): the scale for the next step, the taken-step count, the flag cleared."""
        if not self.enabled or self._rec is None:
            return
        K.loss_scale_update_(self._rec, self.growth_factor, self.backoff_factor, self.growth_interval)
        self._stat = None
        self._unscaled.clear()

    # ------------------------------------------------------------------ host reads: logging and checkpoints only
    def get_scale(self):
        if not self.enabled:
            return 1.0
        return self._init_scale if self._rec is None else float(self._scale)

    def taken_steps(self):
        return self._init_taken if self._rec is None else int(self._rec[3])

    def state_dict(self):
        if not self.enabled:
            return {}
        return {"scale": self.get_scale(), "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": self._init_tracker if self._rec is None else int(self._rec[1])}

    def load_state_dict(self, state_dict):
        if not self.enabled:
            return
        if len(state_dict) == 0:
            raise RuntimeError("The source state dict is empty, possibly because it was saved from a disabled instance of GradScaler.")
        self.growth_factor, self.backoff_factor = float(state_dict["growth_factor"]), float(state_dict["backoff_factor"])
        self.growth_interval = int(state_dict["growth_interval"])
        self._init_scale, self._init_tracker = float(state_dict["scale"]), int(state_dict["_growth_tracker"])
        if self._rec is not None:
            self._rec.view(torch.float32)[0].fill_(self._init_scale)
            self._rec[1].fill_(self._init_tracker)


class GradientAllReducer:
    """Data-parallel gradient averaging: the gradients of `params` are packed into flat fp32 buckets of about `bucket_mb` MiB (one
    collective per bucket instead of one per tensor: xGMI rings are per-link bound, large messages amortise their latency),
    all-reduced over `group` (RCCL when the tensors are on GPUs, gloo on CPU) and unpacked.  The bucket layout is a function of
    the parameter list only, so every rank issues the same collectives in the same order.

    overlap=True: the collectives run UNDER the backward pass.  Buckets are filled in reverse parameter order (the order gradients
    become final in); a post-accumulate-grad hook per parameter counts its bucket down and, when the bucket is complete and every
    earlier-launched bucket has been launched (same order on every rank), packs it and starts its all-reduce asynchronously —
    RCCL runs it on its own stream beside the remaining backward kernels.  Calling the reducer after backward() launches whatever
    did not complete by itself (a parameter that received no gradient contributes zeros — and holds back its bucket and the ones
    after it until then: the launch order is fixed), waits, and unpacks.  With gradient
    accumulation (the reference's trainer: accumulate_grad_batches 2) set `.sync = False` for all but the last micro-batch: the
    hooks then do nothing and the gradients keep accumulating locally, as under DDP's no_sync.

    Accumulation under a LossScaler: the scale is constant over the window; the norm pass, the step and update() run once, after
    the last micro-batch:
        reducer.zero_grad()
        for i, micro in enumerate(window):
            reducer.sync = i == len(window) - 1
            scaler.scale(loss_of(micro) / len(window)).backward()
        reducer()                                         # the all-reduce; the overflow check comes AFTER it: every rank sees the
        scaler.norm_pass(params, max_norm)                # same averaged buckets, so every rank skips or steps together
        optimizer.step(ema=ema, scaler=scaler)
        scaler.update()"""

    def __init__(self, params, bucket_mb=64, group=None, always=False, overlap=False):
        self.params = [p for p in params if p.requires_grad]
        self.group, self.always = group, always          # always: run the collectives even in a one-rank group (tests)
        self.overlap, self.sync = overlap, True
        limit = int(bucket_mb * (1 << 20)) // 4
        order = list(reversed(self.params)) if overlap else self.params
        self.buckets, cur, n = [], [], 0
        for p in order:
            if cur and n + p.numel() > limit:
                self.buckets.append(cur)
                cur, n = [], 0
            cur.append(p)
            n += p.numel()
        if cur:
            self.buckets.append(cur)
        # Persistent flat buckets; every parameter's .grad is a VIEW into its bucket (as DDP's gradient_as_bucket_view): backward
        # accumulates straight into the bucket, the collective runs on it in place, nothing is packed, unpacked or allocated per
        # step.  (Round 3 allocated 5.8 GB of zeros and issued 2 x 1520 copies per step.)  A parameter that receives no gradient:
        # with several ranks it keeps its zeros (its contribution to the average; it then sees weight decay only, as under DDP's
        # bucket views); in a one-rank job it gets .grad = None back (see _touched below).
        # Gradients must ARRIVE THROUGH AUTOGRAD ACCUMULATION (the post-accumulate hook is what marks a parameter as touched) or be
        # ASSIGNED as a tensor of their own (p.grad = g: recognised by its address and copied into the bucket).  A gradient written
        # by hand INTO the bucket view (p.grad.add_(...) without a backward pass) is indistinguishable from the view's zeros
        # without a device read, and a one-rank job drops it — do not do that.
        self.flats = [torch.zeros(sum(p.numel() for p in b), dtype=torch.float32, device=b[0].device) for b in self.buckets]
        self._views = {}
        for flat, bucket in zip(self.flats, self.buckets):
            off = 0
            for p in bucket:
                self._views[id(p)] = flat[off:off + p.numel()].view_as(p)
                off += p.numel()
        self.attach()
        self._works = {}                                  # bucket index -> (work, needs scaling)
        self._pending = [len(b) for b in self.buckets]
        self._next = 0                                    # buckets are launched strictly in index order
        self._hooks = []
        # Which parameters actually received a gradient since the last finished step.  In a one-rank job a parameter that never did
        # gets .grad = None back when the reducer is called (below): torch.optim.AdamW — and this package's — then skips it (no
        # state, no step count, no weight decay), exactly as without a reducer.  With several ranks every parameter keeps its
        # bucket view (another rank may have touched it; the zeros of this one are its contribution), as under DDP's bucket views.
        self._touched = set()
        where = {id(p): i for i, b in enumerate(self.buckets) for p in b}
        for p in self.params:
            self._hooks.append(p.register_post_accumulate_grad_hook(lambda q, i=where[id(p)]: self._ready(i, id(q))))

    def attach(self):
        """Point every parameter's .grad at its slice of the flat buckets (keeping a gradient that is already there)."""
        with torch.no_grad():
            for p in self.params:
                v = self._views[id(p)]
                if p.grad is None:
                    p.grad = v
                elif p.grad.data_ptr() != v.data_ptr():
                    v.copy_(p.grad)
                    p.grad = v

    def zero_grad(self):
        """One fill per bucket instead of one per tensor; use it instead of optimizer.zero_grad(set_to_none=True), which would
        detach the gradients from the buckets (attach() repairs that at the cost of a copy per tensor)."""
        for flat in self.flats:
            flat.zero_()
        self.attach()

    def _active(self):
        import torch.distributed as dist
        return dist.is_available() and dist.is_initialized() and (dist.get_world_size(self.group) > 1 or self.always)

    def _launch(self, i):
        import torch.distributed as dist
        for p in self.buckets[i]:                         # a gradient replaced behind the reducer's back: bring it home first
            g, v = p.grad, self._views[id(p)]
            if g is None:
                v.zero_()
                p.grad = v
            elif g.data_ptr() != v.data_ptr():
                v.copy_(g)
                p.grad = v
        flat = self.flats[i]
        if dist.get_backend(self.group) == "nccl":        # RCCL averages in the collective itself
            self._works[i] = (dist.all_reduce(flat, op=dist.ReduceOp.AVG, group=self.group, async_op=True), False)
        else:                                             # gloo (CPU tests): sum, then scale
            self._works[i] = (dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group, async_op=True), True)

    def _ready(self, i, pid=None):
        self._touched.add(pid)
        if not self.overlap or not self.sync or not self._active():
            return
        self._pending[i] -= 1
        while self._next < len(self.buckets) and self._pending[self._next] <= 0:
            self._launch(self._next)
            self._next += 1

    def __call__(self):
        """After backward(): finish the gradient averaging (in place, in the buckets).  Returns the number of collectives."""
        import torch.distributed as dist
        if not self.sync:
            return 0
        if not self._active():                            # one rank: nothing to average; untouched parameters get grad None back
            for p in self.params:
                if id(p) in self._touched:
                    continue
                g, v = p.grad, self._views[id(p)]
                if g is not None and g.data_ptr() != v.data_ptr():      # assigned by hand (no accumulation hook fired): keep it, in the bucket
                    v.copy_(g)
                    p.grad = v
                else:
                    p.grad = None
            self._touched.clear()
            return 0
        self._touched.clear()
        world = dist.get_world_size(self.group)
        for i in range(self._next, len(self.buckets)):    # not launched under backward (or overlap off): now, in order
            self._launch(i)
        for i in range(len(self.buckets)):
            work, scale = self._works[i]
            work.wait()
            if scale:
                self.flats[i] /= world
        self._works.clear()
        self._pending = [len(b) for b in self.buckets]
        self._next = 0
        return len(self.buckets)

    def remove_hooks(self):
        for h in self._hooks:
            h.remove()
        self._hooks = []


def training_step(model, x_start, cond=None, t=None, optimizer=None, reducer=None, noise=None, clipper=None, ema=None, scaler=None,
                  **kwargs):
    """One optimisation step as the reference's trainer runs it: zero_grad -> p_losses -> backward -> (gradient all-reduce) ->
    (gradient-norm clipping) -> AdamW.  Returns (loss, loss_dict); with a clipper, loss_dict["grad_norm"] is the device scalar.
    `x_start` may instead be a DATA batch (a dict of pixels, caption, class label, frame rate: LatentVisualDiffusion.get_batch_input);
    the loss then comes from model.shared_step(batch, random_uncond=model.classifier_free_guidance), `cond` and `t` stay None.
    `ema` (a lvdm.ema.LitEma, e.g. model.model_ema): the averaged weights are updated inside the optimiser's launch — what
    on_train_batch_end() does in a loop that does not pass it; pass it OR call on_train_batch_end(), not both.
    `scaler` (a LossScaler; the reference's precision: 16): zero_grad -> loss -> scaler.scale(loss).backward() -> (all-reduce) -> the
    scaled norm pass (it replaces the clipper's own: same max_norm, no write pass) -> optimizer.step(ema=..., scaler=scaler) ->
    scaler.update().  loss_dict gains "loss_scale" (the scale this step ran at, a device scalar) and "grad_norm" is the norm of the
    UNSCALED gradients; .grad is left scaled.  The returned loss is the unscaled one.  Without a scaler (or with a disabled one)
    nothing changes: the same launches, the same bits."""
    if scaler is not None and not scaler.enabled:
        scaler = None
    if optimizer is None:
        raise TypeError("training_step needs the optimizer")
    if reducer is not None:
        reducer.zero_grad()                               # one fill per bucket; the gradients stay views into the buckets
    else:
        optimizer.zero_grad(set_to_none=False)            # (multi-tensor fill; the clipper's and AdamW's pointer tables stay valid)
    if isinstance(x_start, dict):
        if cond is not None or t is not None or noise is not None:
            raise TypeError("training_step: a data batch brings its own conditioning; the timesteps and the noise are drawn in forward()")
        loss, info = model.shared_step(x_start, random_uncond=model.classifier_free_guidance, **kwargs)
    else:
        loss, info = p_losses(model, x_start, cond, t, noise=noise, **kwargs)
    if scaler is not None:
        scaler.scale(loss).backward()
    else:
        loss.backward()
    if reducer is not None:
        reducer()
    if scaler is not None:
        params = clipper.params if clipper is not None else [p for group in optimizer.param_groups for p in group["params"]]
        stat = scaler.norm_pass(params, clipper.max_norm if clipper is not None else None)
        info = dict(info, loss_scale=scaler._scale.clone())           # (update() below rewrites the record in place)
        if stat is not None:
            info["grad_norm"] = stat[0]
        optimizer.step(ema=ema, scaler=scaler)
        scaler.update()
        return loss.detach(), info
    if clipper is not None:
        stat = clipper()
        if stat is not None:
            info = dict(info, grad_norm=stat[0])
    if ema is not None:
        optimizer.step(ema=ema)
    else:
        optimizer.step()
    return loss.detach(), info
