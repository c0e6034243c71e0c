"""Host-side mirror of the reference's ``climategan/optim.py``: ExtraAdam (extragradient Adam), the ``torch.optim`` Adam /
RMSprop its ``get_optimizer`` also builds, and the dynamic loss scaling of ``train.amp`` (``GradScaler``).

Same constructor and the reference's two-phase protocol -- ``extrapolation()`` on even steps, ``step()`` on odd
steps (trainer.py:674-694) -- with the whole update of every parameter tensor fused into ONE HIP launch
(``cgan_extra_adam_multi_tensor``).  State layout follows torch.optim conventions (``state[p] = {step, exp_avg,
exp_avg_sq}``) so ``state_dict()`` round-trips with the reference's checkpoints (``g_opt`` / ``d_opt``,
trainer.py:403-420).

Adam and RMSprop keep torch's constructor defaults and state keys; their update is ONE launch per parameter group
(``cgan_adam_multi_tensor`` / ``cgan_rmsprop_multi_tensor``) with the per-parameter step count on the device, so that a
``GradScaler`` can skip a step on a non-finite gradient without the host ever waiting for the answer.
"""
import ctypes

import torch
from torch.optim import Optimizer

from . import _lib
from ._lib import AdamItem, AmpOptimItem
from .ops import _ptr, _stream, touch


class ExtraAdam(Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        if amsgrad:
            raise NotImplementedError("ExtraAdam: amsgrad=True has no HIP path (the reference never enables it)")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad))
        self.params_copy = {}   # id(p) -> saved parameters (reference: list self.params_copy, optim.py:149)
        self._has_copy = False

    def _run(self, mode):
        lib = _lib.load()
        for group in self.param_groups:
            # parameters whose Adam step count differs (a grad was None at some point) go in separate launches
            by_step = {}
            for p in group["params"]:
                if p.grad is None:
                    # the reference saves a copy of EVERY parameter at the first extrapolation (optim.py:166-168); the
                    # copy of a gradient-less one is read back only if that parameter does receive a gradient by the
                    # following step() (domain batches that differ between the two calls).  Parameters that can never
                    # get one (requires_grad=False: the spectral-norm u / v vectors) are skipped: not observable.
                    if mode == 0 and not self._has_copy and p.requires_grad:
                        self.params_copy[id(p)] = p.data.clone()
                    continue
                if not p.is_cuda or p.dtype != torch.float32 or not p.data.is_contiguous():
                    raise RuntimeError("ExtraAdam (HIP): contiguous fp32 device parameters expected")
                if p.grad.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p.data)
                    st["exp_avg_sq"] = torch.zeros_like(p.data)
                st["step"] += 1
                if mode == 0 and not self._has_copy:
                    self.params_copy[id(p)] = torch.empty_like(p.data)
                by_step.setdefault(st["step"], []).append(p)
            beta1, beta2 = group["betas"]
            for step, ps in by_step.items():
                items = (AdamItem * len(ps))()
                mx = 0
                for i, p in enumerate(ps):
                    st = self.state[p]
                    g = p.grad.data.contiguous()
                    if mode == 1 and id(p) not in self.params_copy:
                        raise RuntimeError("Need to call extrapolation before calling step.")
                    items[i] = AdamItem(p.data.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(),
                                        st["exp_avg_sq"].data_ptr(), self.params_copy[id(p)].data_ptr(), p.numel())
                    mx = max(mx, p.numel())
                # pinned + non_blocking: a pageable copy would make the host wait here for the whole backward pass
                # instead of running ahead into the next forward; the pinned buffer is kept until the next call
                host = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).pin_memory()
                table = host.to(ps[0].device, non_blocking=True)
                self._tables = getattr(self, "_tables", [])[-7:] + [(host, table)]
                if _lib.CALL_LOG is not None:        # p, g, m, v read; p, m, v (+ the saved copy on an extrapolation) written
                    _lib.log_bytes(sum(p.numel() for p in ps) * 4 * (8 if mode == 0 else 7))
                _lib.check(lib.cgan_extra_adam_multi_tensor(_ptr(table), len(ps), mx, mode,
                                                            int(mode == 0 and not self._has_copy), step, group["lr"],
                                                            beta1, beta2, group["eps"], group["weight_decay"],
                                                            _stream()), "cgan_extra_adam_multi_tensor")
                # the kernel wrote the parameters through raw pointers: bump their version counters, or every cached
                # packed weight (norms._PackCache keys on them) stays the one packed before this update
                touch(*ps)

    @torch.no_grad()
    def extrapolation(self):
        """Extrapolation step; saves a copy of the current parameters on the first call (optim.py:153-172)."""
        self._run(0)
        self._has_copy = True

    @torch.no_grad()
    def step(self, closure=None):
        """Update step applied to the parameters saved by ``extrapolation`` (optim.py:174-197)."""
        if not self._has_copy:
            raise RuntimeError("Need to call extrapolation before calling step.")
        loss = closure() if closure is not None else None
        self._run(1)
        self.params_copy = {}
        self._has_copy = False
        return loss


class _FusedOptimizer(Optimizer):
    """What Adam and RMSprop share: the item table of one step (every parameter that has a gradient, all groups in one
    upload), the per-parameter ``step`` scalars as views into device buffers, and check -> update -> finish."""

    _moments = ()            # state keys of the fp32 moment tensors, in the item's (m, v) order; None = unused slot

    def _step_scalar(self, p):
        """A 0-dim fp32 device tensor for ``state[p]["step"]``: a view into one buffer per batch of new parameters."""
        free = getattr(self, "_free_steps", None)
        if not free:
            n = sum(len(g["params"]) for g in self.param_groups)
            free = self._free_steps = list(torch.zeros(max(n, 1), dtype=torch.float32, device=p.device).unbind(0))
        return free.pop()

    def _init_state(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = self._step_scalar(p)
            for key in self._moments:
                if key is not None:
                    st[key] = torch.zeros_like(p.data)
        return st

    def _table(self):
        """(device table, [(group, first item, count, largest numel, parameters)]) over the parameters with a gradient."""
        name = type(self).__name__
        spans, rows = [], []
        for group in self.param_groups:
            ps = []
            for p in group["params"]:
                if p.grad is None:
                    continue                                   # torch skips it: no state change, its step does not advance
                if not p.is_cuda or p.dtype != torch.float32 or not p.data.is_contiguous():
                    raise RuntimeError("%s (HIP): contiguous fp32 device parameters expected" % name)
                if p.grad.is_sparse:
                    raise RuntimeError("%s does not support sparse gradients" % name)
                if p.grad.dtype != torch.float32 or not p.grad.is_contiguous():
                    raise RuntimeError("%s (HIP): contiguous fp32 gradients expected" % name)
                st = self._init_state(p)
                m, v = (st[k].data_ptr() if k is not None else None for k in self._moments)
                rows.append(AmpOptimItem(p.data.data_ptr(), p.grad.data_ptr(), m, v, st["step"].data_ptr(), p.numel()))
                ps.append(p)
            if ps:
                spans.append((group, len(rows) - len(ps), len(ps), max(p.numel() for p in ps), ps))
        if not rows:
            return None, spans
        items = (AmpOptimItem * len(rows))(*rows)
        # pinned + non_blocking, as ExtraAdam's table: the host must not wait for the backward pass here
        host = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).pin_memory()
        table = host.to(spans[0][4][0].device, non_blocking=True)
        self._tables = getattr(self, "_tables", [])[-7:] + [(host, table)]
        return table, spans

    def _launch_update(self, lib, items, count, mx, group, inv_scale, found_inf, stream):
        raise NotImplementedError

    def _check(self, lib, table, spans, inv_scale, write_back, found_inf):
        count = sum(s[2] for s in spans)
        if _lib.CALL_LOG is not None:
            _lib.log_bytes(sum(p.numel() for s in spans for p in s[4]) * 4 * (2 if write_back else 1))
        _lib.check(lib.cgan_grads_nonfinite_check_multi_tensor(_ptr(table), count, max(s[3] for s in spans), inv_scale,
                                                               int(write_back), _ptr(found_inf), _stream()),
                   "cgan_grads_nonfinite_check_multi_tensor")

    @torch.no_grad()
    def unscale_and_check(self, inv_scale, found_inf):
        """``GradScaler.unscale_``: every gradient times ``inv_scale`` in place, ``found_inf`` set on +-inf / NaN."""
        table, spans = self._table()
        if table is not None:
            self._check(_lib.load(), table, spans, inv_scale, True, found_inf)

    @torch.no_grad()
    def step(self, closure=None, *, inv_scale=1.0, found_inf=None, check=False):
        """One update of every parameter that has a gradient.  The keyword arguments are the ``GradScaler``'s: the
        gradients are multiplied by ``inv_scale`` in registers (``p.grad`` stays as it is), ``found_inf`` is the scaler's
        device flag -- set by the check launch when ``check`` -- and a set flag turns the update and the step counters'
        increment into no-ops ON THE DEVICE: nothing here waits for it."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        table, spans = self._table()
        if table is None:
            return loss
        lib = _lib.load()
        if check:
            self._check(lib, table, spans, inv_scale, False, found_inf)
        item = ctypes.sizeof(AmpOptimItem)
        base, flag, stream = table.data_ptr(), (found_inf.data_ptr() if found_inf is not None else None), _stream()
        for group, first, count, mx, ps in spans:
            if _lib.CALL_LOG is not None:
                _lib.log_bytes(sum(p.numel() for p in ps) * 4 * (3 + 2 * sum(k is not None for k in self._moments)))
            self._launch_update(lib, base + first * item, count, mx, group, inv_scale, flag, stream)
        _lib.check(lib.cgan_amp_optim_finish(base, sum(s[2] for s in spans), flag, stream), "cgan_amp_optim_finish")
        # the kernel wrote the parameters through raw pointers: bump their version counters so that cached packed
        # weights are re-packed (after a skipped step the re-pack is harmless)
        touch(*[p for s in spans for p in s[4]])
        return loss

    def load_state_dict(self, state_dict):
        """Accepts ``step`` as an int (old torch: the reference's checkpoints), a float or a tensor on any device
        (current torch) and puts it into this optimizer's device scalars."""
        super().load_state_dict(state_dict)
        for p, st in self.state.items():
            if "step" in st:
                value = st["step"]
                value = float(value.item()) if torch.is_tensor(value) else float(value)
                st["step"] = self._step_scalar(p).fill_(value)
            for key in self._moments:
                if key is not None and key in st and not st[key].is_contiguous():
                    st[key] = st[key].contiguous()


class Adam(_FusedOptimizer):
    """``torch.optim.Adam`` (what the reference's ``get_optimizer`` builds for any name it does not know, and the only
    optimizer of its ``train.amp`` mode): same constructor defaults, same state keys (``step``, ``exp_avg``,
    ``exp_avg_sq``), the update of a parameter group in one HIP launch.  ``step`` is a device scalar (as in torch's own
    capturable / fused Adam) so that a skipped step under the ``GradScaler`` does not advance it."""

    _moments = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        if amsgrad:
            raise NotImplementedError("Adam: amsgrad=True has no HIP path (the reference never enables it)")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad))

    def _launch_update(self, lib, items, count, mx, group, inv_scale, found_inf, stream):
        if group.get("amsgrad", False):
            raise NotImplementedError("Adam: amsgrad=True has no HIP path (the reference never enables it)")
        beta1, beta2 = group["betas"]
        _lib.check(lib.cgan_adam_multi_tensor(items, count, mx, group["lr"], beta1, beta2, group["eps"],
                                              group["weight_decay"], inv_scale, found_inf, stream),
                   "cgan_adam_multi_tensor")


class RMSprop(_FusedOptimizer):
    """``torch.optim.RMSprop`` with the defaults the reference's ``get_optimizer`` leaves in place (alpha 0.99, eps 1e-8,
    no momentum, not centered); state keys ``step`` and ``square_avg``."""

    _moments = (None, "square_avg")

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        if not 0.0 <= alpha:
            raise ValueError("Invalid alpha value: {}".format(alpha))
        if momentum != 0:
            raise NotImplementedError("RMSprop: momentum != 0 has no HIP path (the reference never sets it)")
        if centered:
            raise NotImplementedError("RMSprop: centered=True has no HIP path (the reference never sets it)")
        super().__init__(params, dict(lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, momentum=momentum,
                                      centered=centered))

    def _launch_update(self, lib, items, count, mx, group, inv_scale, found_inf, stream):
        if group.get("momentum", 0) != 0 or group.get("centered", False):
            raise NotImplementedError("RMSprop: momentum / centered have no HIP path (the reference never sets them)")
        _lib.check(lib.cgan_rmsprop_multi_tensor(items, count, mx, group["lr"], group["alpha"], group["eps"],
                                                 group["weight_decay"], inv_scale, found_inf, stream),
                   "cgan_rmsprop_multi_tensor")


class GradScaler:
    """Dynamic loss scaling for ``train.amp``: ``torch.amp.GradScaler``'s rule without its host synchronisation.

    The loss kernels of this package take the gradient scale folded into their host-side arguments
    (``autograd.set_grad_scale(scaler.get_scale())`` replaces ``scaler.scale(loss)``), so the scale has to be known on
    the host; what must NOT happen is the host waiting for the device between the backward and the optimizer, which is
    what torch's ``step`` does (``found_inf.item()``).  Here

      * ``step(opt)`` enqueues check -> update -> finish against a device flag: the update multiplies the gradients by
        ``1 / scale`` in registers and, like the step counters' increment, does nothing when the check found a
        non-finite value;
      * ``update()`` enqueues a copy of the flag into pinned host memory, records an event and clears the flag on the
        stream;
      * the copy is read at the NEXT ``get_scale()`` / ``update()`` / ``state_dict()``, where the scale and the growth
        tracker advance by torch's rule: non-finite -> ``scale *= backoff_factor``, tracker 0; otherwise tracker + 1 and,
        on reaching ``growth_interval``, ``scale *= growth_factor``, tracker 0.

    In the trainer the G update therefore waits at most for its own previous optimizer launch, with the whole D update
    in between.  Under data parallelism ``step`` runs after the reducer's ``finish()``: a non-finite value on one rank
    reaches every rank through the all-reduce's sum, so all ranks skip, and back off, together.

    Only the optimizers of this module that update through the scaler's flag (``Adam``, ``RMSprop``) are accepted.  The
    trainer does not checkpoint its scalers (neither does the reference, trainer.py:403-420): a resumed run starts again
    at ``init_scale``."""

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True):
        if enabled:
            if growth_factor <= 1.0:
                raise ValueError("The growth factor must be > 1.0.")
            if backoff_factor >= 1.0:
                raise ValueError("The backoff factor must be < 1.0.")
        self._enabled = bool(enabled)
        self._scale = float(init_scale)
        self._growth_factor = float(growth_factor)
        self._backoff_factor = float(backoff_factor)
        self._growth_interval = int(growth_interval)
        self._growth_tracker = 0
        self._found_inf = None          # device flag (fp32 [1]): 1.0 once a check saw +-inf / NaN
        self._pending = None            # (pinned copy of the flag, event) of the last update()
        self._stage = {}                # id(optimizer) -> "unscaled" | "stepped" since the last update()
        self.skipped_steps = 0          # resolved steps that found a non-finite gradient

    def is_enabled(self):
        return self._enabled

    def advance(self, found_inf):
        """The host rule for one step's flag (torch's ``_amp_update_scale_``)."""
        if found_inf:
            self._scale *= self._backoff_factor
            self._growth_tracker = 0
            self.skipped_steps += 1
        else:
            self._growth_tracker += 1
            if self._growth_tracker == self._growth_interval:
                self._scale *= self._growth_factor
                self._growth_tracker = 0

    def _resolve(self):
        if self._pending is not None:
            host, event = self._pending
            self._pending = None
            event.synchronize()
            self.advance(host.item() != 0.0)

    def get_scale(self):
        if not self._enabled:
            return 1.0
        self._resolve()
        return self._scale

    def get_growth_tracker(self):
        self._resolve()
        return self._growth_tracker

    def _flag(self, optimizer):
        if self._found_inf is None:
            device = next(p for g in optimizer.param_groups for p in g["params"]).device
            self._found_inf = torch.zeros(1, dtype=torch.float32, device=device)
        return self._found_inf

    @staticmethod
    def _supported(optimizer):
        if not isinstance(optimizer, _FusedOptimizer):
            raise TypeError("GradScaler: %s has no update that can be skipped on the device; use this module's Adam or "
                            "RMSprop (AMP does not work with ExtraAdam)" % type(optimizer).__name__)

    def unscale_(self, optimizer):
        """Divide the optimizer's gradients by the scale in place (and run the non-finite check on them)."""
        if not self._enabled:
            return
        self._supported(optimizer)
        if id(optimizer) in self._stage:
            raise RuntimeError("unscale_() has already been called on this optimizer since the last update()."
                               if self._stage[id(optimizer)] == "unscaled" else "unscale_() is being called after step().")
        scale = self.get_scale()
        optimizer.unscale_and_check(1.0 / scale, self._flag(optimizer))
        self._stage[id(optimizer)] = "unscaled"

    def step(self, optimizer, *args, **kwargs):
        if not self._enabled:
            return optimizer.step(*args, **kwargs)
        self._supported(optimizer)
        stage = self._stage.get(id(optimizer))
        if stage == "stepped":
            raise RuntimeError("step() has already been called since the last update().")
        scale = self.get_scale()
        flag = self._flag(optimizer)
        if stage == "unscaled":
            out = optimizer.step(*args, inv_scale=1.0, found_inf=flag, check=False, **kwargs)
        else:
            out = optimizer.step(*args, inv_scale=1.0 / scale, found_inf=flag, check=True, **kwargs)
        self._stage[id(optimizer)] = "stepped"
        return out

    def update(self, new_scale=None):
        if not self._enabled:
            return
        self._resolve()
        if new_scale is not None:
            self._scale = float(new_scale)
            if self._found_inf is not None:
                self._found_inf.zero_()
            self._stage = {}
            return
        if not self._stage or self._found_inf is None:
            raise RuntimeError("No inf checks were recorded prior to update.")
        host = torch.empty(1, dtype=torch.float32).pin_memory()
        host.copy_(self._found_inf, non_blocking=True)
        event = torch.cuda.Event()
        event.record(torch.cuda.current_stream(self._found_inf.device))
        self._found_inf.zero_()
        self._pending = (host, event)
        self._stage = {}

    def state_dict(self):
        if not self._enabled:
            return {}
        self._resolve()
        return {"scale": self._scale, "growth_factor": self._growth_factor, "backoff_factor": self._backoff_factor,
                "growth_interval": self._growth_interval, "_growth_tracker": self._growth_tracker}

    def load_state_dict(self, state_dict):
        if not self._enabled:
            return
        if len(state_dict) == 0:
            raise RuntimeError("The source state dict is empty, possibly because it was saved from a disabled "
                               "instance of GradScaler.")
        self._resolve()
        self._scale = float(state_dict["scale"])
        self._growth_factor = float(state_dict["growth_factor"])
        self._backoff_factor = float(state_dict["backoff_factor"])
        self._growth_interval = int(state_dict["growth_interval"])
        self._growth_tracker = int(state_dict["_growth_tracker"])


def get_scheduler(optimizer, hyperparameters, iterations=-1):
    """Learning-rate scheduler from ``<model>.opt`` (reference optim.py:10-51): ``constant`` / None -> no scheduler,
    ``step`` -> StepLR(lr_step_size, lr_gamma), ``multi_step`` -> MultiStepLR (``lr_milestones`` a list, or an int
    expanded to ``range(lr_milestones, 1000 or iterations, lr_step_size)``).  Host logic only (it edits
    ``param_groups[i]["lr"]``, which the HIP update reads per launch)."""
    from torch.optim import lr_scheduler

    get = hyperparameters.get if hasattr(hyperparameters, "get") else (lambda k: getattr(hyperparameters, k, None))
    policy, lr_step_size, lr_gamma, milestones = (get(k) for k in ("lr_policy", "lr_step_size", "lr_gamma",
                                                                   "lr_milestones"))
    if policy is None or policy == "constant":
        return None
    if policy == "step":
        return lr_scheduler.StepLR(optimizer, step_size=lr_step_size, gamma=lr_gamma, last_epoch=iterations)
    if policy == "multi_step":
        if isinstance(milestones, int):
            if lr_step_size is None:
                raise AssertionError("multi_step with an int lr_milestones needs lr_step_size")
            milestones = list(range(milestones, 1000 if iterations == -1 else iterations, lr_step_size))
        return lr_scheduler.MultiStepLR(optimizer, milestones=list(milestones), gamma=lr_gamma, last_epoch=iterations)
    # the reference RETURNS (does not raise) the exception object here (optim.py:48-50); callers would fail later on
    # ``scheduler.step()``.  Raising at once is the same failure, earlier.
    raise NotImplementedError("learning rate policy [%s] is not implemented" % policy)


def get_optimizer(net, opt_conf, tasks=None, is_disc=False, iterations=-1):
    """(optimizer, scheduler, lr_names) from ``opts.gen.opt`` / ``opts.dis.opt`` (reference optim.py:54-124): one
    parameter group over ``net.parameters()`` when ``lr`` is a float or holds only ``default``; otherwise one group per
    task with its own learning rate (G: encoder for "m", painter for "p", ``decoders[task]`` for the others; D:
    ``net[task]``).  Group and parameter order are the reference's, so ``state_dict()`` of the optimizer is
    interchangeable with the reference's ``g_opt`` / ``d_opt`` checkpoint entries.  Names as in the reference
    (optim.py:110-121): ``extraadam`` -> ExtraAdam, ``rmsprop`` -> RMSprop, any other -> Adam with
    ``betas=(beta1, 0.999)``; ``novograd`` / ``radam`` raise (see below)."""
    lr_names = []
    lr = opt_conf.lr
    if tasks is None or isinstance(lr, float) or len(lr) == 1:
        lr_default = lr if isinstance(lr, float) else lr.default
        params = net.parameters()
        lr_names.append("full")
    else:
        lr_default = lr.default
        params = []
        for task in tasks:
            task_lr = lr.get(task, lr_default)
            parameters = None
            if not is_disc:
                if task == "m":
                    # the encoder rides on the masker's learning rate, as its own group ahead of decoders["m"]
                    params.append({"params": net.encoder.parameters(), "lr": task_lr})
                    lr_names.append("encoder")
                if task == "p":
                    if hasattr(net, "painter"):
                        parameters = net.painter.parameters()
                        lr_names.append("painter")
                else:
                    parameters = net.decoders[task].parameters()
                    lr_names.append("decoder_%s" % task)
            elif task in net:
                parameters = net[task].parameters()
                lr_names.append("disc_%s" % task)
            if parameters is not None:
                params.append({"params": parameters, "lr": task_lr})
    name = str(opt_conf.optimizer).lower()
    if name == "extraadam":
        opt = ExtraAdam(params, lr=lr_default, betas=(opt_conf.beta1, 0.999))
    elif name in ("novograd", "radam"):
        # the reference takes these two from the torch_optimizer package, which is not available to this project's
        # development or test environment: their arithmetic cannot be pinned against it, so they are refused
        raise NotImplementedError("get_optimizer: %r comes from the torch_optimizer package in the reference; its "
                                  "arithmetic cannot be pinned here because the package is not on the machine -- "
                                  "use Adam, ExtraAdam or RMSprop" % opt_conf.optimizer)
    elif name == "rmsprop":
        opt = RMSprop(params, lr=lr_default)
    else:
        opt = Adam(params, lr=lr_default, betas=(opt_conf.beta1, 0.999))
    return opt, get_scheduler(opt, opt_conf, iterations), lr_names
