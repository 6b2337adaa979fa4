"""The optimiser step on the HIP library.

``Adam`` is a drop-in for ``torch.optim.Adam`` as the reference builds it (semseg.py:106-111, pcdseg.py:133-138:
``lr``, ``betas=(0.9, 0.999)``, ``eps=1e-08``, ``weight_decay``; amsgrad off).  It is a ``torch.optim.Optimizer``, so
``torch.optim.lr_scheduler.StepLR(optimizer, 20, 0.5)`` (semseg.py:113), ``for g in optimizer.param_groups:
g['lr'] = lr`` (pcdseg.py:162-163), ``zero_grad()`` and ``state_dict()`` work as with the original (the state it
saves has torch.optim.Adam's layout).

What differs is the memory layout: the parameters of a group are re-pointed into ONE flat fp32 buffer, their
gradients into another (``parallel.FlatGradBucket`` -- the buffer the data-parallel all-reduce already uses), and
``exp_avg`` / ``exp_avg_sq`` are flat twins, so ``step()`` is a single ``pn2_adam_step`` launch over 28 B/element
instead of ~10 foreach launches over ~150 tensors, and ``zero_grad()`` is one fill (or free: ``fused_zero_grad``).

Construct it BEFORE capturing a step into a hipGraph (graph.GraphedStep): a captured launch holds the parameter
addresses it saw, and construction moves the parameters into the flat buffer.

``SGD`` is the same for ``torch.optim.SGD`` -- the other branch of the reference's ``--optimizer`` switch
(semseg.py:103-104, partseg.py:113, clf.py:72, pcdseg.py:130-131: ``lr=0.01, momentum=0.9``): one ``pn2_sgd_step`` launch
per group over the same flat buffers, the momentum buffer a flat twin that exists only where ``momentum != 0``, the
arithmetic torch's bit for bit, the state torch.optim.SGD's layout.

One semantic difference, by construction: a parameter whose gradient was never written still sees a zero gradient
(torch.optim.Adam and torch.optim.SGD skip ``grad is None`` parameters).  Every parameter of the reference's networks
receives a gradient in every step.
"""
import torch

from . import _lib
from . import pointnet_util
from .parallel import FlatGradBucket

_p = _lib.ptr


class _FlatOptimizer(torch.optim.Optimizer):
    """What Adam and SGD share: the flat parameter / gradient buffers of each group, the device cells of ``device_step``,
    ``sync_lr()``, ``zero_grad()``, ``steps_taken()`` and the checks ``step()`` makes before it launches.  A subclass adds its
    own flat state to the group record in ``_init_group_state`` and launches in ``step()``."""
    _name = "optim"

    def _flatten(self, bucket, fused_zero_grad, device_step):
        self.fused_zero_grad = bool(fused_zero_grad)
        self.device_step = bool(device_step)
        self._grads_clear = False
        self._flat = []
        if bucket is not None and len(self.param_groups) != 1:
            raise ValueError("a shared gradient bucket needs a single parameter group")
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.requires_grad]
            if not ps:
                raise ValueError("parameter group without trainable parameters")
            dev = ps[0].device
            if dev.type != "cuda":
                raise _lib.Pn2Error("%s: parameters must live on the GPU (the HIP library is the only "
                                    "implementation)" % self._name)
            if any(p.dtype != torch.float32 or p.device != dev for p in ps):
                raise TypeError("%s: float32 parameters on one device expected" % self._name)
            total = sum(p.numel() for p in ps)
            flat_p = torch.empty(total, device=dev, dtype=torch.float32)
            off = 0
            for p in ps:                                     # re-point the parameters into the flat buffer
                n = p.numel()
                view = flat_p[off:off + n].view(p.shape)
                view.copy_(p.data)
                p.data = view
                off += n
            if bucket is not None:
                if [id(p) for p in bucket.params] != [id(p) for p in ps]:
                    raise ValueError("bucket and optimizer must hold the same parameters in the same order")
                flat_g = bucket.flat
                self._bucket = bucket
            else:
                flat_g = _GradViews(ps).flat
            rec = {"params": ps, "p": flat_p, "g": flat_g, "t": 0, "lr_dev": None, "step_dev": None}
            self._init_group_state(group, rec)
            if self.device_step:
                rec["lr_dev"] = torch.full((1,), float(group["lr"]), device=dev, dtype=torch.float32)
                rec["step_dev"] = torch.zeros(2, device=dev, dtype=torch.int64)
            self._flat.append(rec)

    @staticmethod
    def _views(flat, ps):
        """The slices of a flat twin, shaped as the parameters."""
        out, off = [], 0
        for p in ps:
            n = p.numel()
            out.append(flat[off:off + n].view(p.shape))
            off += n
        return out

    def _init_group_state(self, group, rec):
        raise NotImplementedError

    def sync_lr(self):
        """Copy every group's ``lr`` to its device cell (device_step mode; call outside graph capture)."""
        for group, rec in zip(self.param_groups, self._flat):
            if rec["lr_dev"] is not None:
                rec["lr_dev"].fill_(float(group["lr"]))

    def _before_launch(self):
        """The checks of ``step()`` that do not depend on the update rule."""
        if getattr(self, "_bucket", None) is not None:
            self._bucket.wait_reduced()               # an all-reduce on the bucket's comm stream must have landed
        if torch.cuda.is_current_stream_capturing() and any(rec["step_dev"] is None for rec in self._flat):
            # a captured launch would bake the host step count and learning rate in as kernel-argument constants:
            # every replay would then repeat the SAME step count and lr, silently
            raise _lib.Pn2Error("%s.step() under stream capture needs device_step=True (step count and lr "
                                "in device memory); with host-side values every graph replay would reuse this step's"
                                % self._name)

    def _check_alias(self, rec):
        for p in rec["params"]:
            if p.grad is None or p.grad.data_ptr() < rec["g"].data_ptr() or \
                    p.grad.data_ptr() >= rec["g"].data_ptr() + rec["g"].numel() * 4:
                raise _lib.Pn2Error("%s: a parameter's .grad no longer aliases the flat gradient buffer "
                                    "(use zero_grad(), not `p.grad = None`)" % self._name)

    def _after_launch(self):
        self._grads_clear = self.fused_zero_grad
        pointnet_util.bump_param_generation()       # parameters written through raw pointers: eval-mode folds are stale

    def zero_grad(self, set_to_none=False):
        """One fill per group (the flat buffers stay attached: ``set_to_none`` is ignored)."""
        if self._grads_clear:                                # the last step() already cleared them; only once
            self._grads_clear = False
            return
        for rec in self._flat:
            rec["g"].zero_()

    def steps_taken(self):
        """Host view of the step count per group (device_step mode reads the device cell: synchronises)."""
        return [int(rec["step_dev"][0]) if rec["step_dev"] is not None else rec["t"] for rec in self._flat]

    def _set_steps_taken(self, rec, t):
        rec["t"] = t
        if rec["step_dev"] is not None:
            rec["step_dev"][0] = t


class Adam(_FlatOptimizer):
    _name = "optim.Adam"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *,
                 bucket=None, fused_zero_grad=False, device_step=False):
        """``bucket``: an existing FlatGradBucket over the same parameters in the same order (single group) to share
        its gradient buffer.  ``fused_zero_grad``: ``step()`` also clears the gradients (the next ``zero_grad()``
        becomes a no-op).  ``device_step``: the step count and the learning rate live in device memory, so a
        captured ``step()`` can be replayed from a hipGraph; call ``sync_lr()`` after changing ``param_groups``."""
        if amsgrad:
            raise NotImplementedError("amsgrad is not used by the reference and not implemented")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay:
            raise ValueError("lr, eps and weight_decay must be non-negative")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("betas must lie in [0, 1)")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._flatten(bucket, fused_zero_grad, device_step)

    def _init_group_state(self, group, rec):
        ps = rec["params"]
        rec["m"], rec["v"] = torch.zeros_like(rec["p"]), torch.zeros_like(rec["p"])
        for p, m, v in zip(ps, self._views(rec["m"], ps), self._views(rec["v"], ps)):
            self.state[p] = {"step": torch.tensor(0.0), "exp_avg": m, "exp_avg_sq": v}     # torch.optim.Adam's state, as views

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib, st = _lib.load(), _lib.stream()
        self._before_launch()
        for group, rec in zip(self.param_groups, self._flat):
            self._check_alias(rec)
            rec["t"] += 1
            b1, b2 = group["betas"]
            _lib.check(lib.pn2_adam_step(_p(rec["p"]), _p(rec["g"]), _p(rec["m"]), _p(rec["v"]), rec["p"].numel(),
                                         float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                         float(group["weight_decay"]), rec["t"], _p(rec["lr_dev"]), _p(rec["step_dev"]),
                                         int(self.fused_zero_grad), st), "pn2_adam_step")
        self._after_launch()
        return loss

    def state_dict(self):
        for rec, taken in zip(self._flat, self.steps_taken()):
            for p in rec["params"]:
                self.state[p]["step"] = torch.tensor(float(taken))
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """Accepts a torch.optim.Adam (or this class's) state dict; moments are copied into the flat buffers."""
        views = {p: (self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"]) for rec in self._flat for p in rec["params"]}
        super().load_state_dict(state_dict)
        for rec in self._flat:
            t = 0
            for p in rec["params"]:
                s = self.state.get(p, {})
                m, v = views[p]
                if "exp_avg" in s:
                    m.copy_(s["exp_avg"])
                    v.copy_(s["exp_avg_sq"])
                    t = int(float(s.get("step", 0)))
                self.state[p] = {"step": torch.tensor(float(t)), "exp_avg": m, "exp_avg_sq": v}
            self._set_steps_taken(rec, t)
        self.sync_lr()


class SGD(_FlatOptimizer):
    _name = "optim.SGD"

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 foreach=None, differentiable=False, fused=None, bucket=None, fused_zero_grad=False, device_step=False):
        """torch.optim.SGD's signature (``foreach`` and ``fused`` are accepted and ignored: there is one implementation)
        plus ``bucket``, ``fused_zero_grad`` and ``device_step`` as on ``Adam``.  The momentum buffer of a group is a flat
        twin of its parameters, allocated only where the group's ``momentum != 0`` (setting a non-zero momentum on such a
        group later starts it from a zero buffer)."""
        if differentiable:
            raise NotImplementedError("differentiable=True is not used by the reference and not implemented")
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov, maximize=maximize, foreach=foreach, differentiable=False,
                                      fused=fused))
        self._flatten(bucket, fused_zero_grad, device_step)

    def _init_group_state(self, group, rec):
        rec["buf"] = None
        self._ensure_buffer(group, rec)
        self._publish_state(rec, 0)

    def _ensure_buffer(self, group, rec):
        if group["momentum"] != 0 and rec["buf"] is None:
            rec["buf"] = torch.zeros_like(rec["p"])

    def _publish_state(self, rec, taken):
        """torch.optim.SGD's per-parameter state: the buffer (a view of the flat twin) once a step has been taken, None
        before, no entry without momentum."""
        ps = rec["params"]
        if rec["buf"] is None:
            for p in ps:
                self.state.pop(p, None)
            return
        for p, b in zip(ps, self._views(rec["buf"], ps)):
            self.state[p] = {"momentum_buffer": b if taken >= 1 else None}

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib, st = _lib.load(), _lib.stream()
        self._before_launch()
        for group, rec in zip(self.param_groups, self._flat):
            self._check_alias(rec)
            self._ensure_buffer(group, rec)
            rec["t"] += 1
            buf = rec["buf"] if group["momentum"] != 0 else None
            _lib.check(lib.pn2_sgd_step(_p(rec["p"]), _p(rec["g"]), _p(buf), rec["p"].numel(), float(group["lr"]),
                                        float(group["momentum"]), float(group["dampening"]), float(group["weight_decay"]),
                                        int(bool(group["nesterov"])), int(bool(group["maximize"])), rec["t"],
                                        _p(rec["lr_dev"]), _p(rec["step_dev"]), int(self.fused_zero_grad), st),
                       "pn2_sgd_step")
            if rec["t"] == 1:
                self._publish_state(rec, 1)
        self._after_launch()
        return loss

    def state_dict(self):
        """torch.optim.SGD's layout, plus the steps taken as the extra key ``steps_taken`` of each param group (torch ignores
        it on load; this class resumes from it exactly)."""
        taken = self.steps_taken()
        for rec, t in zip(self._flat, taken):
            self._publish_state(rec, t)
        sd = super().state_dict()
        for group, t in zip(sd["param_groups"], taken):
            group["steps_taken"] = t
        return sd

    def load_state_dict(self, state_dict):
        """Accepts a torch.optim.SGD (or this class's) state dict; momentum buffers are copied into the flat twin and the
        group counts as past its first step, so the next launch does not overwrite them with the gradient."""
        current = self.steps_taken()
        super().load_state_dict(state_dict)
        for group, rec, cur in zip(self.param_groups, self._flat, current):
            self._ensure_buffer(group, rec)
            saved, loaded = group.pop("steps_taken", None), False
            if rec["buf"] is not None:
                for p, view in zip(rec["params"], self._views(rec["buf"], rec["params"])):
                    b = self.state.get(p, {}).get("momentum_buffer")
                    if b is not None:
                        view.copy_(b)
                        loaded = True
            if saved is not None:
                t = int(saved)
            elif loaded:
                t = max(cur, 1)
            elif rec["buf"] is not None:
                t = 0                  # a torch.optim.SGD that has not stepped: its first step clones the gradient
            else:
                t = cur
            self._set_steps_taken(rec, t)
            self._publish_state(rec, t)
        self.sync_lr()


class _GradViews(FlatGradBucket):
    """A FlatGradBucket over an explicit parameter list."""

    def __init__(self, params):
        self.params = list(params)
        dev = self.params[0].device
        self.flat = torch.zeros(sum(p.numel() for p in self.params), device=dev, dtype=torch.float32)
        off = 0
        for p in self.params:
            n = p.numel()
            p.grad = self.flat[off:off + n].view_as(p)
            off += n
