"""Exponential moving average of the trainable weights at the drop-in boundary (reference: lvdm/ema.py, LitEma).

Same constructor (its spelling `use_num_upates` included), buffers and state_dict keys: `decay`, `num_updates` and one shadow buffer
per trainable parameter, named by the parameter name with the dots removed (`m_name2s_name`).  What differs is where the
arithmetic runs: the decay of a step, min(decay, (1 + n) / (10 + n)) in fp32, is computed on the host exactly as the reference
computes it and handed to ONE launch of mudg_ema_multi over all shadows (a device table of (shadow, parameter, count) chunks,
rebuilt only when a tensor moved) — shadow - (1 - decay) * (shadow - parameter), every operation rounded on its own, the bits of
the reference on the CPU.  CPU tensors take the same arithmetic in torch, so the class works in host tests.

Two additions serve this project's training step: `swap(model)` exchanges weights and shadows in place (mudg_swap_multi; what
ema_scope does on entry and on exit instead of store / copy_to / restore, which clone every parameter), and `begin_update()` /
`shadow_map()` let mudg_amd.train.step.AdamW fold the average into its own launch.

`decay` and `num_updates` live on the model's device like every buffer; the host keeps a mirror of both so that a step does not
wait for the device.  load_state_dict() refreshes the mirror; code that writes into the buffers by hand calls `resync()`."""
import torch
from torch import nn


def _increment_versions(tensors):
    for t in tensors:
        torch.autograd.graph.increment_version(t)


class LitEma(nn.Module):
    def __init__(self, model, decay=0.9999, use_num_upates=True):
        super().__init__()
        if decay < 0.0 or decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")
        self.m_name2s_name = {}
        self.register_buffer("decay", torch.tensor(decay, dtype=torch.float32))
        self.register_buffer("num_updates", torch.tensor(0 if use_num_upates else -1, dtype=torch.int))
        for name, p in model.named_parameters():
            if p.requires_grad:
                s_name = name.replace(".", "")          # '.' is not allowed in buffer names
                self.m_name2s_name[name] = s_name
                self.register_buffer(s_name, p.clone().detach().data)
        self.collected_params = []
        self.__dict__["_model"] = model                  # (not a submodule: the average does not own the network)
        self._host = None                                # (decay as a CPU fp32 tensor, num_updates as an int)
        self._tables = {}
        self._own = None                                 # the (parameter, shadow) pairs of that model, walked once

    # ------------------------------------------------------------------ host mirror of the two scalars
    def resync(self):
        self._host, self._own = None, None

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._host = None

    def _apply(self, fn, *args, **kwargs):                # .to() / .cuda() replace the buffer tensors
        out = super()._apply(fn, *args, **kwargs)
        self._own, self._tables = None, {}
        return out

    def _scalars(self):
        if self._host is None:
            self._host = (self.decay.detach().float().cpu(), int(self.num_updates))
        return self._host

    def begin_update(self):
        """Advance `num_updates` and return this update's (1 - decay) as the fp32 value the reference multiplies with."""
        decay, n = self._scalars()
        if n >= 0:
            n += 1
            self.num_updates += 1
            count = torch.tensor(n, dtype=torch.int)
            decay = min(decay, (1 + count) / (10 + count))       # fp32, as lvdm/ema.py:30 computes it
            self._host = (self._host[0], n)
        return float(1.0 - decay)

    # ------------------------------------------------------------------ the pairs and their chunk tables
    def _pairs(self, model):
        shadows = dict(self.named_buffers())
        pairs = []
        for key, p in model.named_parameters():
            if p.requires_grad:
                pairs.append((p, shadows[self.m_name2s_name[key]]))
            else:
                assert key not in self.m_name2s_name
        return pairs

    def pairs(self):
        """The (parameter, shadow) pairs of the model the average was built on.  Walked once and kept: the walk costs a pass over
        named_parameters() and named_buffers() (1520 tensors each for the UNet), which a training step should not pay.  Moving the
        average (.to()) drops the list; a parameter or buffer REPLACED by hand on either side needs `resync()`."""
        if self._own is None:
            self._own = (self._pairs(self._model), None)
            self._own = (self._own[0], {id(p): s for p, s in self._own[0]})
        return self._own[0]

    def shadow_map(self):
        """{id(parameter): shadow} of those pairs (for the fused optimiser launch)."""
        self.pairs()
        return self._own[1]

    @staticmethod
    def _check(pairs):
        for p, s in pairs:
            if s.device != p.device or s.dtype != torch.float32 or p.dtype != torch.float32 or s.shape != p.shape \
                    or not s.is_contiguous() or not p.is_contiguous():
                raise RuntimeError("LitEma works on contiguous fp32 parameters with their shadows on the same device "
                                   f"(got {tuple(p.shape)} {p.dtype} on {p.device}, shadow {tuple(s.shape)} {s.dtype} on {s.device})")

    def _table(self, tag, pairs):
        from mudg_amd.train import kernels as K
        key = tuple((p.data_ptr(), s.data_ptr(), p.numel()) for p, s in pairs)
        hit = self._tables.get(tag)
        if hit is None or hit[0] != key:
            hit = (key,) + K.chunk_table([(s, p) for p, s in pairs])
            self._tables[tag] = hit
        return hit[1], hit[2]

    # ------------------------------------------------------------------ the reference's interface
    @torch.no_grad()
    def update(self, pairs, one_minus_decay):
        """shadow <- shadow - one_minus_decay * (shadow - parameter) over `pairs` of (parameter, shadow)."""
        if not pairs:
            return
        self._check(pairs)
        if pairs[0][0].is_cuda:
            from mudg_amd.train import kernels as K
            table, n = self._table(("ema", len(pairs)), pairs)
            K.ema_multi_(table, n, one_minus_decay)
            _increment_versions(s for _, s in pairs)
        else:
            omd = torch.tensor(one_minus_decay, dtype=torch.float32)
            for p, s in pairs:
                s.sub_(omd * (s - p))

    def forward(self, model):
        self.update(self._pairs(model), self.begin_update())

    @torch.no_grad()
    def copy_to(self, model):
        for p, s in self._pairs(model):
            p.data.copy_(s.data)
            torch.autograd.graph.increment_version(p)

    def store(self, parameters):
        """Save the current parameters for restoring later (a clone of each: ema_scope uses swap() instead)."""
        self.collected_params = [param.clone() for param in parameters]

    @torch.no_grad()
    def restore(self, parameters):
        """Restore the parameters stored with `store`."""
        for c_param, param in zip(self.collected_params, parameters):
            param.data.copy_(c_param.data)
            torch.autograd.graph.increment_version(param)

    # ------------------------------------------------------------------ the in-place exchange behind ema_scope
    @torch.no_grad()
    def swap(self, model):
        """Weights and shadows change places, in place: twice is the identity, bit for bit, and no copy of the parameters is held.
        The version counters of both sides are bumped (the kernel writes through raw pointers): packed operand weights, captured
        graphs and cached contexts are keyed on (data_ptr, _version)."""
        pairs = self._pairs(model)
        if not pairs:
            return
        self._check(pairs)
        if pairs[0][0].is_cuda:
            from mudg_amd.train import kernels as K
            table, n = self._table(("swap", len(pairs)), pairs)
            K.swap_multi_(table, n)
        else:
            for p, s in pairs:
                held = p.detach().clone()
                p.data.copy_(s)
                s.copy_(held)
        _increment_versions(t for pair in pairs for t in pair)
