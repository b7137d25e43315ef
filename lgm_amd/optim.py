"""The optimizer tail of the training iteration (main.py:73, 105-109): the global-norm gradient clip and the AdamW
update, over the whole parameter list in three launches (include/lgm_optim.h: k_optim_sqnorm, k_optim_reduce,
k_optim_adamw), with the clip coefficient applied to the gradient inside the update: the scaled gradient is never
written, and the norm never leaves the device.

  AdamW            a torch.optim.Optimizer with torch.optim.AdamW's state (`step` a CPU fp32 tensor, `exp_avg`,
                   `exp_avg_sq`) and param_groups keys, so schedulers drive it and state_dicts go both ways;
                   `max_grad_norm` fuses accelerator.clip_grad_norm_ into the step.
  clip_grad_norm_  drop-in for torch.nn.utils.clip_grad_norm_ (k_optim_sqnorm, k_optim_reduce, k_optim_scale).

GPU tensors run the kernels; CPU tensors take torch's own functional forms.
"""
from __future__ import annotations

import weakref
from typing import Iterable, Optional, Union

import numpy as np
import torch

from . import _native as nat
from ._native import ptr

CHUNK = nat.OPTIM_CHUNK
_ROW = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("numel", "<i4"), ("chunk0", "<i4")])
assert _ROW.itemsize == 40  # include/lgm_optim.h lgm_optim_tensor
_INT_MAX = 2 ** 31 - 1


def _upload(a: np.ndarray, dev: torch.device) -> torch.Tensor:
    """Host bytes -> a device uint8 tensor through a fresh pinned tensor, without a host sync (the pinned block is
    not handed out again before the copy has run: torch's host allocator waits for it)."""
    host = torch.empty(max(a.nbytes, 8), dtype=torch.uint8, pin_memory=True)
    host[:a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1))
    return host.to(dev, non_blocking=True)


class _Lists:
    """The device half of include/lgm_optim.h's data model for one list of tensors: the table, the chunk -> tensor
    array and the partials buffer. The chunk array depends on the numels alone and the table on the pointers: each
    is uploaded again only when it changes."""

    def __init__(self):
        self.numels = None
        self.rows = None
        self.chunk0 = None
        self.nchunks = 0
        self.chunk_tensor = self.table = self.partials = None

    def update(self, rows: list, dev: torch.device):
        """rows: one (p_ptr, g_ptr, m_ptr, v_ptr, numel) per tensor, in table order."""
        numels = [r[4] for r in rows]
        if numels != self.numels or self.chunk_tensor is None or self.chunk_tensor.device != dev:
            if numels and max(numels) > _INT_MAX:
                raise ValueError(f"a tensor of {max(numels)} elements: the kernels index a tensor with 31 bits")
            counts = (np.asarray(numels, np.int64) + (CHUNK - 1)) // CHUNK
            ends = np.cumsum(counts)
            nchunks = int(ends[-1]) if len(numels) else 0
            if nchunks > _INT_MAX:
                raise ValueError(f"{nchunks} chunks of {CHUNK} elements: beyond the 2^31 - 1 of a launch grid")
            self.chunk0 = (ends - counts).astype(np.int32)
            self.chunk_tensor = _upload(np.repeat(np.arange(len(numels), dtype=np.int32), counts), dev)
            self.partials = torch.empty(max(nchunks, 1), dtype=torch.float64, device=dev)
            self.numels, self.nchunks, self.rows = numels, nchunks, None
        if rows != self.rows:
            t = np.empty(len(rows), _ROW)
            if rows:
                a = np.asarray([r[:4] for r in rows], np.uint64)
                t["p"], t["g"], t["m"], t["v"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
                t["numel"], t["chunk0"] = np.asarray(numels, np.int32), self.chunk0
            self.table = _upload(t, dev)
            self.rows = rows

    def grad_norm(self, max_norm: float, dev: torch.device) -> torch.Tensor:
        """k_optim_sqnorm + k_optim_reduce -> device float32 [2]: (norm, coef)."""
        out = torch.empty(2, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            nat.call("lgm_optim_grad_norm", dev, ptr(self.table), len(self.rows), ptr(self.chunk_tensor), self.nchunks,
                     float(max_norm), ptr(self.partials), self.partials.numel() * 8, ptr(out))
        return out

    def scale(self, out: torch.Tensor, dev: torch.device):
        with torch.cuda.device(dev):
            nat.call("lgm_optim_scale", dev, ptr(self.table), len(self.rows), ptr(self.chunk_tensor), self.nchunks,
                     out.data_ptr() + 4)

    def adamw(self, first: int, last: int, out: Optional[torch.Tensor], dev: torch.device, lr, beta1, beta2, eps, wd,
              step):
        """k_optim_adamw on the tensors first .. last - 1 of the table."""
        begin = int(self.chunk0[first])
        end = int(self.chunk0[last]) if last < len(self.rows) else self.nchunks
        if end == begin:
            return
        coef = None if out is None else out.data_ptr() + 4
        with torch.cuda.device(dev):
            nat.call("lgm_optim_adamw", dev, ptr(self.table), len(self.rows), ptr(self.chunk_tensor), begin, end - begin,
                     coef, float(lr), float(beta1), float(beta2), float(eps), float(wd), float(step))


def _dense(t: torch.Tensor) -> bool:
    """The tensor's numel elements lie in one gap-free block of memory (any permutation of the dimensions)."""
    if t.is_contiguous():
        return True
    dims = sorted((st, sz) for st, sz in zip(t.stride(), t.shape) if sz != 1)
    expect = 1
    for st, sz in dims:
        if st != expect:
            return False
        expect *= sz
    return True


def _same_layout(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.shape != b.shape:
        return False
    if a.stride() == b.stride():
        return True
    return all(sa == sb for sa, sb, n in zip(a.stride(), b.stride(), a.shape) if n != 1)  # (a size-1 dim has any stride)


def _meta(p: torch.Tensor, g: torch.Tensor):
    """What the validation of a (parameter, gradient) pair depends on besides the tensor objects themselves."""
    return (p.dtype, p.shape, p.stride(), g.dtype, g.shape, g.stride())


def _check_f32(t: torch.Tensor, what: str):
    if t.is_sparse or t.layout != torch.strided:
        raise RuntimeError(f"lgm_amd.optim: sparse {what}s are not supported")
    if t.dtype != torch.float32:
        raise TypeError(f"lgm_amd.optim: {what}s must be float32, got {t.dtype}")


class AdamW(torch.optim.Optimizer):
    """torch.optim.AdamW on the kernels of include/lgm_optim.h. max_grad_norm: clip the gradients' global 2-norm
    (over all param groups) to it inside the step, as accelerator.clip_grad_norm_ before optimizer.step() does; the
    gradients themselves stay unscaled (CPU tensors: torch's clip_grad_norm_ runs, which scales them in place) and
    `grad_norm` holds the step's total norm as a 0-dim device tensor.
    Hyperparameters are read from param_groups on every step. amsgrad, maximize and capturable are not supported."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 max_grad_norm: Optional[float] = None, *, amsgrad: bool = False, maximize: bool = False,
                 capturable: bool = False):
        if isinstance(lr, torch.Tensor):
            raise ValueError("lgm_amd.optim.AdamW: lr must be a number (a tensor lr belongs to capturable)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid betas: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if max_grad_norm is not None and not max_grad_norm >= 0.0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm}")
        # torch.optim.AdamW's keys, all of them: a state_dict of this class loads there and steps
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=None, capturable=capturable, differentiable=False, fused=None,
                        decoupled_weight_decay=True)
        super().__init__(params, defaults)
        self.max_grad_norm = max_grad_norm
        self.grad_norm: Optional[torch.Tensor] = None
        self._lists = _Lists()
        self._checked = {}  # parameter -> the tensors _check_param validated with it
        self._check_groups()

    def __getstate__(self):
        return dict(super().__getstate__(), max_grad_norm=self.max_grad_norm)

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("max_grad_norm", None)
        self.grad_norm, self._lists, self._checked = None, _Lists(), {}

    def _check_groups(self):
        for group in self.param_groups:
            for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
                if group.get(flag):
                    raise ValueError(f"lgm_amd.optim.AdamW does not support {flag}=True")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_groups()
        # the parameters that have a gradient, per group, each validated (everything before anything is changed)
        work, devs = [], set()
        for group in self.param_groups:
            entries = []
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                state = self.state[p]
                c = self._checked.get(p)
                if (c is None or c[0]() is not g or c[1] is not state.get("exp_avg")
                        or c[2] is not state.get("exp_avg_sq") or c[4] != _meta(p, g)):
                    c = self._check_param(p, g, state)
                devs.add(p.device)
                entries.append((p, g, state, c[3]))
            work.append((group, entries))
        if not devs:
            self.grad_norm = None
            return loss
        if len(devs) > 1:
            raise RuntimeError(f"lgm_amd.optim.AdamW: parameters on more than one device ({', '.join(map(str, devs))})")
        dev = devs.pop()
        if dev.type != "cuda":
            self._step_torch(work)
            return loss
        rows, sets, keep, steps = self._table_rows(work)
        self._lists.update(rows, dev)  # (may still refuse the list: the steps are counted after it)
        torch._foreach_add_(steps, 1.0)
        out = None
        if self.max_grad_norm is not None:
            out = self._lists.grad_norm(self.max_grad_norm, dev)
            self.grad_norm = out[0]
        else:
            self.grad_norm = None
        for group, st, first, last in sets:
            beta1, beta2 = group["betas"]
            self._lists.adamw(first, last, out, dev, group["lr"], beta1, beta2, group["eps"], group["weight_decay"], st)
        del keep  # (the layout copies of gradients lived until the launches were enqueued)
        return loss

    def _check_param(self, p, g, state):
        """Validate one parameter with its gradient, make its state as torch.optim.Adam._init_group does, and remember
        the tensors that were looked at: (weak reference to g, exp_avg, exp_avg_sq, gradient usable as it is, _meta(p,
        g)). A later step with the very same tensor objects, unchanged in dtype, shape and strides (`p.data = ...` or
        an in-place restride keeps the object), skips all of this (their data pointers are still read every step);
        the gradient is not kept alive."""
        _check_f32(g, "gradient")
        _check_f32(p, "parameter")
        if g.device != p.device:
            raise RuntimeError(f"lgm_amd.optim.AdamW: a parameter on {p.device} with its gradient on {g.device}: "
                               "parameters and gradients on more than one device")
        if g.shape != p.shape:
            raise RuntimeError(f"lgm_amd.optim.AdamW: gradient {tuple(g.shape)} of a parameter {tuple(p.shape)}")
        if len(state) == 0:
            state["step"] = torch.tensor(0.0, dtype=torch.float32)
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        direct = True
        if p.is_cuda:
            if not _dense(p):
                raise RuntimeError(f"lgm_amd.optim.AdamW: a parameter of shape {tuple(p.shape)} and strides "
                                   f"{p.stride()} is not dense")
            st = state["step"]
            if st.device.type != "cpu":  # (a state_dict of a fused torch optimizer keeps its steps on the device)
                state["step"] = st.detach().to("cpu", torch.float32)
            for key in ("exp_avg", "exp_avg_sq"):
                t = state[key]
                if t.dtype != torch.float32 or t.device != p.device or t.shape != p.shape:
                    raise RuntimeError(f"lgm_amd.optim.AdamW: state {key} is {t.dtype} {tuple(t.shape)} on "
                                       f"{t.device}, its parameter float32 {tuple(p.shape)} on {p.device}")
                if not _same_layout(t, p):
                    state[key] = torch.empty_like(p, memory_format=torch.preserve_format).copy_(t)
            direct = _same_layout(g, p)  # (otherwise the gradient is copied into the parameter's layout every step)
        c = self._checked[p] = (weakref.ref(g), state["exp_avg"], state["exp_avg_sq"], direct, _meta(p, g))
        return c

    def _table_rows(self, work):
        """The table rows (p, g, m, v pointers, numel) in table order -- group by group, inside a group by step count
        (a late first gradient has its own bias correction) -- the sets that share one launch: (group, step, first
        row, past the last row), the gradients' layout copies, and the step tensors, which the caller increments:
        the counts used here are already those of this step."""
        steps = [state["step"] for _, es in work for _, _, state, _ in es]
        counts = (torch.stack(steps) + 1).tolist()
        rows, sets, keep, k = [], [], [], 0
        for group, entries in work:
            by_step = {}
            for p, g, state, direct in entries:
                if not direct:
                    g = torch.empty_like(p, memory_format=torch.preserve_format).copy_(g)
                    keep.append(g)
                row = (p.data_ptr(), g.data_ptr(), state["exp_avg"].data_ptr(), state["exp_avg_sq"].data_ptr(), p.numel())
                by_step.setdefault(counts[k], []).append(row)
                k += 1
            for t in sorted(by_step):
                sets.append((group, t, len(rows), len(rows) + len(by_step[t])))
                rows.extend(by_step[t])
        return rows, sets, keep, steps

    def _step_torch(self, work):
        """CPU tensors: torch's own clip and functional AdamW (which counts the steps itself)."""
        from torch.optim.adamw import adamw
        if self.max_grad_norm is not None:
            self.grad_norm = torch.nn.utils.clip_grad_norm_([p for _, es in work for p, *_ in es], self.max_grad_norm)
        else:
            self.grad_norm = None
        for group, entries in work:
            if not entries:
                continue
            beta1, beta2 = group["betas"]
            adamw([p for p, *_ in entries], [g for _, g, *_ in entries], [s["exp_avg"] for _, _, s, _ in entries],
                  [s["exp_avg_sq"] for _, _, s, _ in entries], [], [s["step"] for _, _, s, _ in entries], foreach=None,
                  capturable=False, differentiable=False, fused=None, amsgrad=False, beta1=beta1, beta2=beta2,
                  lr=group["lr"], weight_decay=group["weight_decay"], eps=group["eps"], maximize=False)


@torch.no_grad()
def clip_grad_norm_(parameters: Union[torch.Tensor, Iterable[torch.Tensor]], max_norm: float, norm_type: float = 2.0,
                    error_if_nonfinite: bool = False, foreach: Optional[bool] = None) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_ for float32 GPU gradients on k_optim_sqnorm, k_optim_reduce and k_optim_scale:
    returns the total norm as a 0-dim device tensor without a host sync (error_if_nonfinite=True reads it: one sync,
    as in torch). norm_type != 2 and CPU tensors go to torch's function. Every call builds and uploads its table anew
    (two small pinned copies and a partials buffer; nothing is kept between calls, unlike AdamW, which reuses its table
    while the pointers stay)."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    params = list(parameters)
    grads = [p.grad for p in params if p.grad is not None]
    if float(norm_type) != 2.0 or not grads or all(not g.is_cuda for g in grads):
        return torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type, error_if_nonfinite, foreach)
    dev = grads[0].device
    rows, back = [], []
    for g in grads:
        _check_f32(g, "gradient")
        if g.device != dev:
            raise RuntimeError(f"lgm_amd.optim.clip_grad_norm_: gradients on more than one device ({dev}, {g.device})")
        t = g
        if not _dense(g):  # (norm and scale do not care about the layout, only about gaps)
            t = g.contiguous()
            back.append((g, t))
        rows.append((0, t.data_ptr(), 0, 0, t.numel()))
    lists = _Lists()
    lists.update(rows, dev)
    out = lists.grad_norm(float(max_norm), dev)
    norm = out[0]
    if error_if_nonfinite and not bool(torch.isfinite(norm)):
        raise RuntimeError(f"The total norm of order {norm_type} for gradients from `parameters` is non-finite, so it "
                           "cannot be clipped. To disable this error and scale the gradients by the non-finite norm "
                           "anyway, set `error_if_nonfinite=False`")
    lists.scale(out, dev)
    for g, t in back:
        g.copy_(t)
    return norm
