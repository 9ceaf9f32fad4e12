"""FusedAdam: torch.optim.Adam's update as ONE HIP launch per step (csrc/optim.hip gn_adam_step), and the one thing an in-place update owes this package.

Why the optimiser lives here.  MLPStack, HipLinear and the UNet's layers evaluate through PACKS of their parameters, and every pack is cached under one
rule: the device and ``_version`` of the module's tensors (``components.mlp.generation``).  torch's own in-place updates bump those versions; a kernel
that writes through a raw pointer does not.  So after the launch ``step()`` bumps the version counter of every updated parameter, exp_avg and
exp_avg_sq (``torch.autograd.graph.increment_version``): every pack of an updated module is rebuilt at its next use -- the inference forward's as the
training forward's -- and a ``backward()`` whose forward ran before the step raises autograd's "modified by an inplace operation" error instead of
differentiating the new values.  Nothing else is kept: ``FusedAdam(model)`` means the model's parameters, and the ``modules=`` keywords of the
constructor and of ``step`` are accepted and need no bookkeeping.

Semantics: torch.optim.Adam's, per parameter group (lr, betas, eps, weight_decay as L2: g + wd * p).  State keys and types are torch's (``step`` a CPU
fp32 scalar tensor, ``exp_avg``, ``exp_avg_sq``) and the groups carry torch's keys, so ``state_dict()`` loads into a torch.optim.Adam over the same
parameters and the reverse; the ``optimizer_states`` of a reference checkpoint fit as they are.  The bias corrections are computed here in fp64 from
``step`` and passed as scalars.  Parameters whose ``grad`` is None are skipped and their ``step`` does not advance.  Refused by name before any launch:
amsgrad / maximize (NotImplementedError), a sparse gradient (NotImplementedError), a parameter or gradient that is not fp32 and contiguous (TypeError).

The launch reads a device table of (p, g, exp_avg, exp_avg_sq, numel, first workgroup, scalar set) entries, uploaded only when a pointer, the parameter
set or the assignment of scalar sets changed since the last step.
"""
import math

import torch

from . import _lib, ops

__all__ = ["FusedAdam"]


def _check_param(p):
    if p.dtype != torch.float32:
        raise TypeError(f"FusedAdam: parameters must be torch.float32, got {p.dtype}")
    if p.is_sparse or not p.is_contiguous():
        raise TypeError("FusedAdam: parameters must be dense and contiguous")


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False, modules=None):
        if isinstance(params, torch.nn.Module):                       # FusedAdam(model): its parameters
            params = params.parameters()
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"FusedAdam: invalid lr / betas / eps / weight_decay: {lr}, {betas}, {eps}, {weight_decay}")
        # torch.optim.Adam's group keys, so that a state dict goes both ways
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)
        self._check_groups()
        for group in self.param_groups:
            for p in group["params"]:
                _check_param(p)
        self._tables = {}                                              # batch number -> (key, device table)

    def _check_groups(self):
        for group in self.param_groups:
            if group.get("amsgrad"):
                raise NotImplementedError("FusedAdam: amsgrad=True is not implemented")
            if group.get("maximize"):
                raise NotImplementedError("FusedAdam: maximize=True is not implemented")
            if group.get("decoupled_weight_decay") or group.get("capturable") or group.get("differentiable"):
                raise NotImplementedError("FusedAdam: decoupled_weight_decay / capturable / differentiable are not implemented")
            if isinstance(group["lr"], torch.Tensor):
                raise NotImplementedError("FusedAdam: a tensor lr is not implemented")

    def _collect(self):
        """-> [(p, grad, state, group)] of this step, everything checked: nothing has been launched or advanced when a check raises"""
        self._check_groups()
        work, dev = [], None
        for group in self.param_groups:
            for p in group["params"]:
                g = p.grad
                if g is None or p.numel() == 0:
                    continue
                _check_param(p)
                if g.is_sparse:
                    raise NotImplementedError("FusedAdam: sparse gradients are not implemented")
                if g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape:
                    raise TypeError("FusedAdam: gradients must be contiguous torch.float32 of the parameter's shape")
                if not p.is_cuda:
                    raise _lib.GarmentNetsHipError("FusedAdam.step needs parameters on the GPU (no CPU fallback)")
                if dev is None:
                    dev = p.device
                elif p.device != dev:
                    raise ValueError("FusedAdam: the parameters of one optimiser must live on one device")
                st = self.state[p]
                for k in ("exp_avg", "exp_avg_sq"):
                    t = st.get(k)
                    if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != p.device or t.shape != p.shape):
                        raise TypeError(f"FusedAdam: {k} must be contiguous torch.float32 of the parameter's shape, on its device")
                work.append((p, g, st, group))
        return work

    @torch.no_grad()
    def step(self, closure=None, modules=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = self._collect()
        if not work:
            return loss
        # the scalar sets: one per (group, step count) in use; the table names them by index
        hypers, hyper_of, rows = [], {}, []
        for p, g, st, group in work:
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["step"] += 1                                  # (a CPU scalar tensor, torch's layout; an int in the checkpoints of older torch)
            step = int(st["step"])
            key = (id(group), step)
            h = hyper_of.get(key)
            if h is None:
                b1, b2 = (float(b) for b in group["betas"])
                h = hyper_of[key] = len(hypers)
                hypers.append((float(group["lr"]), b1, b2, float(group["eps"]), float(group["weight_decay"]), 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)))
            rows.append((p, g, st["exp_avg"], st["exp_avg_sq"], h))
        # one launch; more scalar sets than a launch carries (parameters at many different step counts) are split over launches
        batches, cur, used = [], [], {}
        for row in rows:
            if row[4] not in used and len(used) == _lib.ADAM_MAX_HYPER:
                batches.append((cur, used))
                cur, used = [], {}
            used.setdefault(row[4], len(used))
            cur.append(row)
        batches.append((cur, used))
        for bi, (cur, used) in enumerate(batches):
            self._launch(bi, cur, used, hypers)
        for k in [k for k in self._tables if k >= len(batches)]:
            del self._tables[k]
        torch.autograd.graph.increment_version([t for p, _, m, v, _ in rows for t in (p, m, v)])
        return loss

    def _launch(self, bi, rows, used, hypers):
        entries, blk = [], 0
        for p, g, m, v, h in rows:
            entries.append((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), blk, used[h], 0))
            blk += -(-p.numel() // _lib.ADAM_CHUNK)
        dev = rows[0][0].device
        key = (dev, tuple(entries))
        cached = self._tables.get(bi)
        if cached is None or cached[0] != key:
            host = (_lib.AdamEntry * len(entries))(*[_lib.AdamEntry(*e) for e in entries])
            table = ops._table_dev(host, dev)
            cached = self._tables[bi] = (key, table)
        hy = (_lib.AdamHyper * len(used))()
        for h, i in used.items():
            hy[i] = _lib.AdamHyper(*hypers[h])
        _lib.call("gn_adam_step", ops._p(cached[1]), len(entries), blk, hy, len(used), ops._stream())
