"""``Adam``: drop-in for ``torch.optim.Adam`` as the reference training scripts construct it (``*/main.py:308-315``: one
parameter group per tensor, ``lr``, ``weight_decay``), executed as ONE gfx950 launch over all tensors (``mn_adam_step``)
instead of ~7 small kernels per group.  Same update as torch (amsgrad off, L2 weight decay folded into the gradient),
same ``state_dict`` layout (``step``, ``exp_avg``, ``exp_avg_sq``), so checkpoints interchange.

``capturable = True`` keeps the step count AND every group's ``lr`` / ``weight_decay`` in device memory (``mn_adam_step_dev``) so that
``step()`` can be captured in a HIP graph and replayed (micronet_amd.train.GraphedTrainStep): ``refresh_hyper()`` -- called before every
replay -- copies the groups' current ``lr`` / ``weight_decay`` into that device table when the training loop edited them (the reference's
``adjust_learning_rate``, wbwtab/main.py:62-66), ``sync_steps()`` writes the device step count back into ``state``.  betas / eps are
frozen at capture time; changing them afterwards raises.

Per-group key ``l1`` (default 0, >= 0): an L1 sub-gradient ``l1 * sign(p)`` added to the gradient in front of the weight decay, inside the same launch
(``mn_adam_step_l1`` / ``mn_adam_step_l1_dev``) -- the sparse-training step of channel pruning, where the reference runs ``updateBN()`` (pruning/main.py:65-69:
``grad.add_(s * sign(gamma))`` for every BatchNorm, two small launches each) between ``backward()`` and ``step()``.  While EVERY group has ``l1 == 0``,
``step()`` calls exactly the entry points it called before the key existed (``mn_adam_step`` / ``mn_adam_step_dev``): an optimizer that never sets ``l1``
behaves as it always did.  In capturable mode the ``l1`` values live in a device tensor beside the {lr, weight_decay} table, under the same rules: allocated in
the first eager step, refreshed by ``refresh_hyper()``, so editing ``group['l1']`` between replays reaches the captured launch (also from and to 0: whether the
L1 entry point is captured is decided once, by the groups' ``l1`` at the first capturable step)."""
import ctypes as C

import torch

from . import _lib


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, l1=0.0):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1) or weight_decay < 0 or not l1 >= 0:
            raise ValueError("invalid Adam hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, l1=l1))
        for group in self.param_groups:
            self._l1_of(group)
        self.capturable = False
        self._step_dev = None
        self._hyper_dev = {}          # (betas, eps) batch key -> device [n][2] = lr, weight_decay
        self._hyper_host = {}
        self._l1_dev = {}             # (betas, eps) batch key -> device [n] = l1; only when some group had l1 != 0 at the first capturable step
        self._l1_host = {}

    @staticmethod
    def _l1_of(group):
        l1 = float(group.get("l1", 0.0))          # (.get: param_groups of a state_dict written before the key existed)
        if not l1 >= 0:
            raise ValueError("Adam: l1 must be >= 0, got %r" % (group.get("l1"),))
        return l1

    def _host_step(self):
        steps = {int(st["step"]) for st in self.state.values() if st}
        if len(steps) > 1:
            raise _lib.MicronetHipError("capturable Adam needs one common step count for all parameters")
        return steps.pop() if steps else 0

    def sync_steps(self):
        """Copy the device-side step count (advanced by graph replays) into every ``state[p]['step']``."""
        if self._step_dev is not None:
            n = int(self._step_dev.item())
            for st in self.state.values():
                if st:
                    st["step"].fill_(n)

    def state_dict(self):
        self.sync_steps()             # a checkpoint taken between graph replays carries the replayed step count
        return super().state_dict()

    def _hyper_items(self):
        items = {}
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                items.setdefault((float(b1), float(b2), float(group["eps"])), []).append((float(group["lr"]), float(group["weight_decay"]), self._l1_of(group)))
        return items

    def refresh_hyper(self):
        """Bring the device-side {lr, weight_decay} table -- and the ``l1`` table beside it -- up to date with ``param_groups`` (no-op when nothing
        changed; one small host-to-device copy per batch key and table when the schedule moved).  Raises if betas / eps differ from the captured values."""
        if not self._hyper_dev:
            return
        items = self._hyper_items()
        if set(items) != set(self._hyper_dev):
            raise _lib.MicronetHipError("capturable Adam: betas / eps changed after the step was captured; re-capture the step")
        for key, its in items.items():
            vals, l1s = [v[:2] for v in its], [v[2] for v in its]
            if len(vals) != len(self._hyper_host[key]):
                raise _lib.MicronetHipError("capturable Adam: parameter groups changed after capture")
            if vals != self._hyper_host[key]:
                self._hyper_dev[key].copy_(torch.tensor(vals, dtype=torch.float32), non_blocking=False)
                self._hyper_host[key] = vals
            if key in self._l1_dev:
                if l1s != self._l1_host[key]:
                    self._l1_dev[key].copy_(torch.tensor(l1s, dtype=torch.float32), non_blocking=False)
                    self._l1_host[key] = l1s
            elif any(l1s):
                raise _lib.MicronetHipError("capturable Adam: l1 became non-zero after the step was captured without it; re-capture the step")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.get_lib()
        if self.capturable:
            return self._step_capturable(lib, loss)
        # tensors that share (step, betas, eps) go into one launch table
        batches = {}
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse or p.dtype != torch.float32 or not p.is_cuda:
                    raise _lib.MicronetHipError("micronet_amd.optim.Adam handles dense float32 CUDA parameters")
                st = self.state[p]
                if not st:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                if not p.is_contiguous():
                    raise _lib.MicronetHipError("non-contiguous parameter")
                key = (int(st["step"]), float(b1), float(b2), float(group["eps"]), p.device.index)
                batches.setdefault(key, []).append((p, g, st, float(group["lr"]), float(group["weight_decay"]), self._l1_of(group)))
        sparse = any(self._l1_of(group) != 0 for group in self.param_groups)
        for (step, b1, b2, eps, dev), items in batches.items():
            arr = (_lib.AdamTensor * len(items))()
            for i, (p, g, st, lr, wd, _) in enumerate(items):
                arr[i] = _lib.AdamTensor(p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(), lr, wd)
            with torch.cuda.device(dev):
                stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                if sparse:
                    l1 = (C.c_float * len(items))(*[it[5] for it in items])
                    rc = lib.mn_adam_step_l1(arr, l1, len(items), step, b1, b2, eps, stream)
                else:
                    rc = lib.mn_adam_step(arr, len(items), step, b1, b2, eps, stream)
            if rc != 0:
                lib.check(rc, "mn_adam_step_l1" if sparse else "mn_adam_step")
        return loss

    def _step_capturable(self, lib, loss):
        items, dev = {}, None
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    raise _lib.MicronetHipError("capturable Adam: every parameter needs a gradient on every step")
                if p.grad.is_sparse or p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous() or not p.grad.is_contiguous():
                    raise _lib.MicronetHipError("micronet_amd.optim.Adam handles dense contiguous float32 CUDA parameters")
                st = self.state[p]
                if not st:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                dev = p.device
                items.setdefault((float(b1), float(b2), float(group["eps"])), []).append(
                    (p, p.grad, st, float(group["lr"]), float(group["weight_decay"]), self._l1_of(group)))
        if dev is None:
            return loss
        if self._step_dev is None:
            self._step_dev = torch.full((1,), self._host_step(), dtype=torch.int32, device=dev)
        self._step_dev.add_(1)
        for key, its in items.items():
            b1, b2, eps = key
            vals, l1s = [(it[3], it[4]) for it in its], [it[5] for it in its]
            capturing = torch.cuda.is_current_stream_capturing()
            if key not in self._hyper_dev:          # first capturable step (eager warm-up, outside any capture): allocate the tables
                self._hyper_dev[key] = torch.tensor(vals, dtype=torch.float32, device=dev)
                self._hyper_host[key] = vals
                if any(l1s):
                    self._l1_dev[key] = torch.tensor(l1s, dtype=torch.float32, device=dev)
                    self._l1_host[key] = l1s
            elif len(vals) != len(self._hyper_host[key]):
                raise _lib.MicronetHipError("capturable Adam: parameter groups changed after capture")
            elif vals != self._hyper_host[key] and not capturing:
                self._hyper_dev[key].copy_(torch.tensor(vals, dtype=torch.float32))
                self._hyper_host[key] = vals
            sparse = key in self._l1_dev
            if not sparse and any(l1s):
                raise _lib.MicronetHipError("capturable Adam: l1 became non-zero after the first capturable step ran without it; build a new optimizer")
            if sparse and l1s != self._l1_host[key] and not capturing:
                self._l1_dev[key].copy_(torch.tensor(l1s, dtype=torch.float32))
                self._l1_host[key] = l1s
            arr = (_lib.AdamTensor * len(its))()
            for i, (p, g, st, lr, wd, _) in enumerate(its):
                arr[i] = _lib.AdamTensor(p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(), lr, wd)
            with torch.cuda.device(dev):
                stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                if sparse:
                    rc = lib.mn_adam_step_l1_dev(arr, (C.c_float * len(its))(*l1s), len(its), C.c_void_p(self._step_dev.data_ptr()),
                                                 C.c_void_p(self._hyper_dev[key].data_ptr()), C.c_void_p(self._l1_dev[key].data_ptr()), b1, b2, eps, stream)
                else:
                    rc = lib.mn_adam_step_dev(arr, len(its), C.c_void_p(self._step_dev.data_ptr()), C.c_void_p(self._hyper_dev[key].data_ptr()), b1, b2, eps, stream)
            if rc != 0:
                lib.check(rc, "mn_adam_step_l1_dev" if sparse else "mn_adam_step_dev")
        return loss
