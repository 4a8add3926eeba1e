"""The optimizer step of the reference's training recipe (must3r/engine/train.py), native: what runs between ``loss`` and the next forward::

    param_groups = get_parameter_groups(decoder, 0, args.weight_decay)
    optimizer = AdamW(param_groups, lr=args.lr, betas=(0.9, 0.95))
    loss_scaler = LossScaler()
    load_model(args, args.resume, encoder, decoder, optimizer, loss_scaler)          # a checkpoint of either side
    for it, batch in enumerate(loader):
        if it % accum_iter == 0:
            adjust_learning_rate(optimizer, epoch + it / len(loader), args)
        loss = criterion(decoder(...)) / accum_iter
        norm = loss_scaler(loss, optimizer, parameters=decoder.parameters(), update_grad=(it + 1) % accum_iter == 0)
        if (it + 1) % accum_iter == 0:
            optimizer.zero_grad()
    save_model(args, epoch, encoder, decoder, optimizer, loss_scaler, "last")

``AdamW`` is ``torch.optim.AdamW`` on two launches of ``must3r_hip_optim_adamw`` (include/must3r_hip.h "ABI 21, additive"): one table of all parameter tensors,
one pass over parameters and moments.  ``LossScaler`` is croco's ``NativeScalerWithGradNormCount`` (a ``torch.amp.GradScaler``, an unscale, a global L2 norm,
optionally a clip, the step and the update) on ``must3r_hip_optim_norm``: one pass over the gradients leaves the norm, the non-finite flag and the coefficient
``inv_scale * clip`` in a device record and updates the scale on the device; the step reads the record.  Nothing here waits for the GPU: there is no ``.item()``,
the skipped step of an overflow is a branch inside the kernels.

``.grad`` IS LEFT AS BACKWARD WROTE IT: the unscale and the clip are a factor inside the step kernel, not a read-modify-write of every gradient.  After
``loss_scaler(...)`` a gradient still carries the loss scale and is not clipped; the returned norm is that of the unscaled gradients, before the clip, as
croco's.

Sums run in a fixed order (no atomics): equal states and gradients give equal bits.  The parameters are written through raw pointers, so every updated
parameter gets ``torch.autograd.graph.increment_version``: the native modules re-mirror their weights when ``_version`` moves (model/_hip_module.py).
"""
import ctypes as C
import math
import os

import torch

from . import _lib
from ._train_common import _ptr, _scratch, _stream

_ALIGN = 4   # elements: every tensor's slice of a flat state buffer starts 16-byte aligned


def _flat(numel, device, dtype=torch.float32):
    """A zeroed flat state buffer (the moments of all parameters, or their step counts)."""
    return torch.zeros((numel,), dtype=dtype, device=device)


class AdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` for fp32 parameters on the GPU: the same ``param_groups`` (``lr``, ``betas``, ``eps``, ``weight_decay`` and any extra key, such as
    ``lr_scale``), the same ``state`` (``step`` a 0-dim fp32 tensor, ``exp_avg``, ``exp_avg_sq``) and therefore the same ``state_dict()``;
    ``load_state_dict()`` takes what any torch AdamW saved.  The moments of all parameters live in two flat buffers and the step counts in a third;
    ``state[p]`` holds views.  State dicts can be loaded and saved on any device; a step on CPU parameters raises.  A parameter whose ``.grad`` is ``None`` is skipped as torch skips it: no decay, no step count.  ``.grad`` is never written."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False):
        if amsgrad:
            raise NotImplementedError("AdamW: amsgrad is not built")
        if maximize:
            raise NotImplementedError("AdamW: maximize is not built")
        if isinstance(lr, torch.Tensor):
            raise ValueError("AdamW: lr is a host number here")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        self._layout = None
        # the keys of torch.optim.AdamW's groups, so that a state dict of either loads into the other; the switches between torch's implementations mean nothing here
        defaults = dict(torch.optim.AdamW([torch.zeros(1)]).defaults)
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False)
        super().__init__(params, defaults)
        self.steps_taken = 0

    # -- layout ---------------------------------------------------------------------------------
    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        g = self.param_groups[-1]
        if g.get("amsgrad") or g.get("maximize"):
            raise NotImplementedError("AdamW: amsgrad and maximize are not built")
        for p in g["params"]:
            if p.dtype != torch.float32 or p.is_sparse or p.layout != torch.strided:
                raise TypeError(f"AdamW: parameters are dense fp32 tensors; got {p.dtype}, {p.layout}")
            if not p.is_contiguous() or p.numel() == 0:
                raise TypeError("AdamW: parameters are contiguous and not empty")
        self._layout = None

    def _params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def _ensure_layout(self):
        """The flat buffers and the cached descriptor arrays; existing state (of a loaded state dict, or from before ``add_param_group``) moves into them."""
        if self._layout is not None:
            return self._layout
        params = self._params()
        if not params:
            raise ValueError("AdamW: no parameters")
        dev = params[0].device
        if any(p.device != dev for p in params):
            raise ValueError("AdamW: all parameters live on one device")
        offs, total = [], 0
        for p in params:
            offs.append(total)
            total += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        m, v, steps = _flat(total, dev), _flat(total, dev), _flat((len(params) + _ALIGN - 1) // _ALIGN * _ALIGN, dev)
        views = []
        for i, (p, o) in enumerate(zip(params, offs)):
            views.append((m[o:o + p.numel()].view(p.shape), v[o:o + p.numel()].view(p.shape), steps[i]))
        tab = (_lib.OptimTensor * len(params))()
        gi = 0
        for k, g in enumerate(self.param_groups):
            for p in g["params"]:
                t = tab[gi]
                t.p, t.m, t.v, t.step = p.data_ptr(), views[gi][0].data_ptr(), views[gi][1].data_ptr(), views[gi][2].data_ptr()
                t.n, t.group = p.numel(), k
                gi += 1
        nbytes = _lib.load().must3r_hip_optim_scratch_bytes(len(params), sum(p.numel() for p in params))
        scratch = _scratch(nbytes, dev)
        control = torch.zeros((4,), dtype=torch.float32, device=dev)
        L = dict(params=params, dev=dev, m=m, v=v, steps=steps, views=views, tab=tab, act=(_lib.OptimTensor * len(params))(),
                 groups=(_lib.OptimGroup * len(self.param_groups))(), scratch=scratch, nbytes=nbytes, control=control,
                 index={id(p): i for i, p in enumerate(params)})
        self._layout = L
        with torch.no_grad():
            for i, p in enumerate(params):
                if p in self.state and len(self.state[p]):
                    self._adopt(i, p, self.state[p])
        return L

    def _adopt(self, i, p, st):
        """state[p] becomes views of the flat buffers, holding the values it held"""
        m, v, step = self._layout["views"][i]
        if st.get("exp_avg") is not m:
            m.copy_(st["exp_avg"])
            v.copy_(st["exp_avg_sq"])
            s = st["step"]
            step.copy_(s if isinstance(s, torch.Tensor) else torch.tensor(float(s)))
        st["exp_avg"], st["exp_avg_sq"], st["step"] = m, v, step
        st.pop("max_exp_avg_sq", None)

    def load_state_dict(self, state_dict):
        """What ``torch.optim.AdamW.state_dict()`` gave, of any implementation (``step`` a tensor on the CPU or the device, or a number): the values are copied
        into the flat buffers."""
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            if g.get("amsgrad") or g.get("maximize"):
                raise NotImplementedError("AdamW: amsgrad and maximize are not built")
            g.setdefault("amsgrad", False)
            g.setdefault("maximize", False)
        self._layout = None
        self._ensure_layout()

    # -- the table of one step ------------------------------------------------------------------
    def _table(self, what):
        """``(array, n, updated parameters, tensors to keep alive)``: the cached descriptors with the pointers that moved refreshed (``zero_grad(set_to_none=True)``
        gives new gradients every step); where some parameters have no gradient, the descriptors of the others, compacted"""
        L = self._ensure_layout()
        if L["dev"].type != "cuda":
            raise RuntimeError(f"AdamW.{what}: the parameters must live on the GPU (there is no CPU path); they are on {L['dev']}")
        tab, idx, upd, keep = L["tab"], [], [], []
        for i, p in enumerate(L["params"]):
            g = p.grad
            if g is None:
                continue
            if g.is_sparse or g.dtype != torch.float32 or g.device != L["dev"] or g.shape != p.shape:
                raise RuntimeError(f"AdamW.{what}: gradients are dense fp32 tensors on the parameters' device, of their shape")
            if not g.is_contiguous():
                g = g.contiguous()
                keep.append(g)
            t, pp, gp = tab[i], p.data_ptr(), g.data_ptr()
            if t.p != pp:
                t.p = pp
            if t.g != gp:
                t.g = gp
            idx.append(i)
            upd.append(p)
        if len(idx) == len(L["params"]):
            return tab, len(idx), upd, keep
        act = L["act"]
        for n, i in enumerate(idx):
            act[n] = tab[i]
        return act, len(idx), upd, keep

    def _args(self, tab, n, control):
        L = self._layout
        a = _lib.OptimArgs()
        a.tensors, a.n_tensors = C.cast(tab, C.POINTER(_lib.OptimTensor)), n
        a.control = None if control is None else control.data_ptr()
        a.stream = _stream(L["dev"])
        return a

    def grad_norm(self, max_norm=None, scaler=None):
        """One pass over the gradients (``must3r_hip_optim_norm``): the control record of the next ``step(control=...)`` -- a float32 ``[4]`` device tensor whose
        element 0 is the L2 norm of the unscaled gradients, 1 the coefficient ``inv_scale * clip``, 2 (as int32) the non-finite flag.  ``scaler``: a
        ``LossScaler`` whose scale divides the gradients and is updated in place, on the device.  ``None`` where no parameter has a gradient."""
        tab, n, _, keep = self._table("grad_norm")
        if n == 0:
            return None
        L = self._layout
        a = self._args(tab, n, L["control"])
        a.max_norm = float(max_norm) if max_norm is not None else 0.0
        if scaler is not None and scaler.enabled:
            scale, tracker = scaler._state(L["dev"])
            a.scale, a.growth_tracker = scale.data_ptr(), tracker.data_ptr()
            a.growth_factor, a.backoff_factor, a.growth_interval = scaler.growth_factor, scaler.backoff_factor, scaler.growth_interval
        with torch.cuda.device(L["dev"]):
            _lib.check(_lib.load().must3r_hip_optim_norm(C.byref(a), _ptr(L["scratch"]), L["nbytes"]))
        return L["control"]

    @torch.no_grad()
    def step(self, closure=None, *, control=None):
        """One AdamW step of every parameter that has a gradient.  ``control``: the record ``grad_norm`` returned -- the gradients are multiplied by its
        coefficient inside the kernel, and nothing at all is changed where it flags a non-finite gradient.  ``.grad`` is left as backward wrote it."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        tab, n, upd, keep = self._table("step")
        if n == 0:
            return loss
        L = self._layout
        groups = L["groups"]
        if len(groups) != len(self.param_groups):
            raise RuntimeError("AdamW: the parameter groups changed behind the optimizer")
        for k, g in enumerate(self.param_groups):
            q = groups[k]
            q.lr, q.weight_decay, q.eps = float(g["lr"]), float(g["weight_decay"]), float(g["eps"])
            q.beta1, q.beta2 = float(g["betas"][0]), float(g["betas"][1])
        for p in upd:
            st = self.state[p]
            if len(st) == 0:
                i = L["index"][id(p)]
                st["step"], st["exp_avg"], st["exp_avg_sq"] = L["views"][i][2], L["views"][i][0], L["views"][i][1]
        a = self._args(tab, n, control)
        a.groups, a.n_groups = C.cast(groups, C.POINTER(_lib.OptimGroup)), len(groups)
        with torch.cuda.device(L["dev"]):
            _lib.check(_lib.load().must3r_hip_optim_adamw(C.byref(a), _ptr(L["scratch"]), L["nbytes"]))
        torch.autograd.graph.increment_version(upd)
        self.steps_taken += 1
        return loss


class LossScaler:
    """croco's ``NativeScalerWithGradNormCount`` for this module's ``AdamW``: ``scaler(loss, optimizer, clip_grad=None, parameters=None, create_graph=False,
    update_grad=True)`` runs ``(loss * scale).backward()`` and, with ``update_grad``, the norm pass and the step; it returns the L2 norm of the unscaled
    gradients (before the clip) as a 0-dim device tensor, ``None`` without ``update_grad``.  The scale follows ``torch.amp.GradScaler`` (65536, x2 after 2000
    clean steps, x0.5 on a non-finite gradient, which also skips the step), updated on the device: nothing here reads a value back.  ``enabled=False``: scale 1,
    no updates (a non-finite gradient still skips the step).  The norm is taken over the optimizer's parameters that have a gradient; ``parameters`` is
    accepted for the reference's call sites.  ``state_dict()`` has ``GradScaler``'s keys."""
    state_dict_key = "amp_scaler"

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True):
        if enabled and (growth_factor <= 1.0 or not 0.0 < backoff_factor < 1.0 or growth_interval < 1):
            raise ValueError("LossScaler: growth_factor > 1, 0 < backoff_factor < 1 and growth_interval >= 1 are required")
        self.enabled = bool(enabled)
        self.init_scale, self.growth_factor, self.backoff_factor = float(init_scale), float(growth_factor), float(backoff_factor)
        self.growth_interval = int(growth_interval)
        self._scale = self._tracker = None
        self._init_tracker = 0

    def _state(self, device):
        if self._scale is None or self._scale.device != device:
            scale = torch.full((1,), self.init_scale, dtype=torch.float32, device=device) if self._scale is None else self._scale.to(device)
            tracker = torch.full((1,), self._init_tracker, dtype=torch.int32, device=device) if self._tracker is None else self._tracker.to(device)
            self._scale, self._tracker = scale, tracker
        return self._scale, self._tracker

    def get_scale(self):
        """the scale as a device tensor ``[1]`` (1 where disabled); reading its value is the caller's synchronisation"""
        return self._scale

    def __call__(self, loss, optimizer, clip_grad=None, parameters=None, create_graph=False, update_grad=True):
        if not isinstance(optimizer, AdamW):
            raise TypeError("LossScaler drives must3r_amd.train_optim.AdamW (the unscale and the clip live in its step kernel); got "
                            f"{type(optimizer).__name__}")
        if self.enabled:
            scale, _ = self._state(loss.device)
            (loss * scale[0]).backward(create_graph=create_graph)
        else:
            loss.backward(create_graph=create_graph)
        if not update_grad:
            return None
        control = optimizer.grad_norm(max_norm=clip_grad, scaler=self)
        if control is None:
            return None
        optimizer.step(control=control)
        return control[0].clone()

    def state_dict(self):
        if not self.enabled:
            return {}
        return {"scale": float(self._scale) if self._scale is not None else self.init_scale, "growth_factor": self.growth_factor,
                "backoff_factor": self.backoff_factor, "growth_interval": self.growth_interval,
                "_growth_tracker": int(self._tracker) if self._tracker is not None else self._init_tracker}

    def load_state_dict(self, state_dict):
        if not self.enabled:
            return
        if len(state_dict) == 0:
            raise RuntimeError("The source state dict is empty, possibly because it was saved from a disabled instance of GradScaler.")
        self.init_scale = float(state_dict["scale"])
        self.growth_factor, self.backoff_factor = float(state_dict["growth_factor"]), float(state_dict["backoff_factor"])
        self.growth_interval = int(state_dict["growth_interval"])
        self._init_tracker = int(state_dict["_growth_tracker"])
        if self._scale is not None:
            self._scale.fill_(self.init_scale)
            self._tracker.fill_(self._init_tracker)


# -- must3r/engine/optimizer.py ---------------------------------------------------------------------
def _get_num_layer_for_vit(var_name, depth, offset=0):
    if var_name.startswith("feat_embed") or var_name.startswith("patch_embed"):
        return 0 + offset
    if var_name.startswith("blocks"):
        return int(var_name.split(".")[1]) + 1 + offset
    if var_name.startswith("norm"):   # part of the last block
        return depth + offset
    if any(var_name.startswith(k) for k in ("head", "prediction_head")):
        return depth + 1 + offset
    raise NotImplementedError(var_name)


def get_parameter_groups(model, offset, weight_decay, layer_decay=1.0, skip_list=(), no_lr_scale_list=[]):
    """The reference's parameter groups: no decay for biases, norms and ``skip_list``; with ``layer_decay < 1`` one pair of groups per layer, scaled by
    ``layer_decay ** (depth + offset + 1 - layer)`` (``lr_scale``, applied by ``adjust_learning_rate``), except the names of ``no_lr_scale_list``."""
    names, groups = {}, {}
    depth = None
    assert layer_decay == 1.0 or 0. < layer_decay < 1.
    if layer_decay < 1.:
        depth = model.depth
        num_layers = depth + offset
        layer_decay_values = [layer_decay ** (num_layers + 1 - i) for i in range(num_layers + 2)]
    for name, param in model.named_parameters():
        if not param.requires_grad:
            continue   # frozen weights
        if name.endswith(".bias") or "norm" in name or name in skip_list:
            group_name, this_weight_decay = "no_decay", 0.
        else:
            group_name, this_weight_decay = "decay", weight_decay
        if layer_decay < 1.:
            skip_scale = False
            layer_id = _get_num_layer_for_vit(name, depth, offset)
            group_name = "layer_%d_%s" % (layer_id, group_name)
            if name in no_lr_scale_list:
                skip_scale = True
                group_name = f"{group_name}_no_lr_scale"
        else:
            layer_id, skip_scale = 0, True
        if group_name not in groups:
            scale = 1. if skip_scale else layer_decay_values[layer_id]
            names[group_name] = {"weight_decay": this_weight_decay, "params": [], "lr_scale": scale}
            groups[group_name] = {"weight_decay": this_weight_decay, "params": [], "lr_scale": scale}
        groups[group_name]["params"].append(param)
        names[group_name]["params"].append(name)
    return list(groups.values())


def adjust_learning_rate(optimizer, epoch, args):
    """Half-cycle cosine after a linear warm-up (``args.lr``, ``args.min_lr``, ``args.warmup_epochs``, ``args.epochs``; ``epoch`` may be fractional): every
    group gets the rate times its ``lr_scale``.  Returns the unscaled rate."""
    if epoch < args.warmup_epochs:
        lr = args.lr * epoch / args.warmup_epochs
    else:
        lr = args.min_lr + (args.lr - args.min_lr) * 0.5 * (1. + math.cos(math.pi * (epoch - args.warmup_epochs) / (args.epochs - args.warmup_epochs)))
    for g in optimizer.param_groups:
        g["lr"] = lr * g.get("lr_scale", 1)
    return lr


# -- must3r/engine/io.py --------------------------------------------------------------------------
def save_model(args, epoch, encoder, decoder, optimizer, loss_scaler, fname=None):
    """``args.output_dir/checkpoint-<fname or epoch>.pth`` with the reference's keys: encoder, decoder, optimizer, scaler, args, epoch."""
    path = os.path.join(str(args.output_dir), "checkpoint-%s.pth" % (str(epoch) if fname is None else fname))
    torch.save({"encoder": encoder.state_dict(), "decoder": decoder.state_dict(), "optimizer": optimizer.state_dict(),
                "scaler": loss_scaler.state_dict(), "args": args, "epoch": epoch}, path)
    return path


def load_model(args, chkpt_path, encoder, decoder, optimizer, loss_scaler):
    """Resume from a checkpoint of ``save_model`` or of the reference's: sets ``args.start_epoch``."""
    args.start_epoch = 0
    if chkpt_path is None:
        return
    checkpoint = torch.load(chkpt_path, map_location="cpu", weights_only=False)
    encoder.load_state_dict(checkpoint["encoder"], strict=False)
    decoder.load_state_dict(checkpoint["decoder"], strict=False)
    args.start_epoch = checkpoint["epoch"] + 1
    optimizer.load_state_dict(checkpoint["optimizer"])
    if "scaler" in checkpoint:
        loss_scaler.load_state_dict(checkpoint["scaler"])
