"""Shared by tests/test_optim_cpu.py and tests/test_optim_gpu.py: the float64 evaluation of include/lgm_optim.h's
formulas (the truth of the optimizer tests), and one parameter list held in three arms: lgm_amd.optim (under test),
torch's own clip_grad_norm_ + torch.optim.AdamW in fp32 on the same device (measured next to it), and the truth."""
import math

import torch

from lgm_amd import optim as O
from lgm_amd import _native as nat

CHUNK = nat.OPTIM_CHUNK
FLOOR = 1e-6
HP = dict(lr=4e-4, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05)


def cat64(ts):
    """The logical values of a list of tensors as one float64 CPU vector (whatever their layouts)."""
    ts = [t.detach().cpu().double().reshape(-1) for t in ts]
    return torch.cat(ts) if ts else torch.zeros(0, dtype=torch.float64)


def rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def truth_step(tr, grads, groups, max_norm):
    """One step of include/lgm_optim.h in float64, exact hyperparameters. tr: one dict(p, m, v, t) per tensor (m, v
    None before the first gradient); grads: float64 tensors or None; groups: [(indices, lr, beta1, beta2, eps, wd)].
    Returns the total norm."""
    S = math.fsum(float((g * g).sum()) for g in grads if g is not None)
    norm = math.sqrt(S) if math.isfinite(S) else float("nan")
    coef = 1.0
    if max_norm is not None:
        coef = min(1.0, max_norm / (norm + 1e-6)) if math.isfinite(S) else float("nan")
    for idx, lr, b1, b2, eps, wd in groups:
        for i in idx:
            if grads[i] is None:
                continue
            s = tr[i]
            if s["m"] is None:
                s["m"], s["v"] = torch.zeros_like(s["p"]), torch.zeros_like(s["p"])
            s["t"] += 1
            t, g = s["t"], grads[i] * coef
            p = s["p"] * (1.0 - lr * wd)
            s["m"] = s["m"] + (g - s["m"]) * (1.0 - b1)
            s["v"] = b2 * s["v"] + (1.0 - b2) * (g * g)
            s["p"] = p - (lr / (1.0 - b1 ** t)) * (s["m"] / (s["v"].sqrt() / math.sqrt(1.0 - b2 ** t) + eps))
    return norm


class Slot:
    """How one parameter and its gradients are laid out in the arm under test. kind: 'plain'; 'cl' (channels_last
    parameter and gradient); 'cl_cg' (channels_last parameter, contiguous gradient); ('view', po, go): parameter and
    gradient are views at element offsets po and go of flat buffers (what a DDP bucket view looks like)."""

    def __init__(self, shape, kind="plain"):
        self.shape, self.kind = tuple(shape), kind

    def _place(self, value, dev, off):
        n = value.numel()
        flat = torch.zeros(n + 8, device=dev)
        flat[off:off + n].copy_(value.reshape(-1))
        return flat[off:off + n].view(self.shape)

    def param(self, value, dev, native):
        if self.kind in ("cl", "cl_cg"):
            return value.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_()
        if native and isinstance(self.kind, tuple):
            return self._place(value, dev, self.kind[1]).requires_grad_()
        return value.to(dev).clone().requires_grad_()

    def grad(self, value, dev, native):
        if self.kind == "cl":
            return value.to(dev).contiguous(memory_format=torch.channels_last)
        if native and isinstance(self.kind, tuple):
            return self._place(value, dev, self.kind[2])
        return value.to(dev).clone()


def edge_slots():
    """The shapes of the main test: the chunk edges, an empty tensor, channels_last weights, misaligned views, 300
    tensors of 1 .. 17 elements and one tensor of 0.85M."""
    s = [Slot((n,)) for n in (1, 3, 14, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5, 0)]
    s += [Slot((64, 64, 3, 3), "cl"), Slot((64, 64, 3, 3), "cl_cg")]
    s += [Slot((5000,), ("view", 1, 3)), Slot((37,), ("view", 3, 1)), Slot((CHUNK + 3,), ("view", 0, 2)),
          Slot((2, CHUNK), ("view", 2, 0))]
    s += [Slot((1 + i % 17,)) for i in range(300)]
    s += [Slot((920, 921))]  # (961k elements in all: 1e-3 randn gradients have a norm below 1)
    return s


class Arms:
    """One parameter list in the three arms. groups: lists of slot indices with their hyperparameters (None: one
    group of everything with HP)."""

    def __init__(self, slots, dev, seed=0, max_norm=1.0, groups=None, torch_arm=True):
        self.slots, self.dev, self.max_norm = slots, torch.device(dev), max_norm
        self.gen = torch.Generator().manual_seed(seed)
        vals = [torch.randn(s.shape, generator=self.gen) for s in slots]
        self.groups = groups or [(list(range(len(slots))), dict(HP))]
        self.p_nat = [s.param(v, dev, True) for s, v in zip(slots, vals)]
        self.p_tor = [s.param(v, dev, False) for s, v in zip(slots, vals)] if torch_arm else None
        self.truth = [dict(p=v.double(), m=None, v=None, t=0) for v in vals]
        self.opt = O.AdamW([dict(params=[self.p_nat[i] for i in idx], **hp) for idx, hp in self.groups],
                           max_grad_norm=max_norm)
        self.topt = None
        if torch_arm:
            self.topt = torch.optim.AdamW([dict(params=[self.p_tor[i] for i in idx], **hp) for idx, hp in self.groups])
        self.held = []  # earlier gradients, kept alive: the next ones cannot land on their addresses
        self.table = []

    def draw(self, scale, skip=()):
        """One gradient value (CPU fp32) per slot, None for the slots in `skip`."""
        return [None if i in skip else scale * torch.randn(s.shape, generator=self.gen)
                for i, s in enumerate(self.slots)]

    def set_grads(self, gvals, native=True, torch_arm=True):
        for i, (s, g) in enumerate(zip(self.slots, gvals)):
            if native:
                if self.p_nat[i].grad is not None:
                    self.held.append(self.p_nat[i].grad)
                self.p_nat[i].grad = None if g is None else s.grad(g, self.dev, True)
            if torch_arm and self.p_tor is not None:
                self.p_tor[i].grad = None if g is None else s.grad(g, self.dev, False)

    def step(self, gvals, label="", check=True):
        """Gradients into the three arms, one step of each, and the bar on p, exp_avg, exp_avg_sq, the update and
        the norm: error <= max(2 x torch's error, 1e-6) relative L2 against the truth; for the update the floor is
        2 x the error of the truth rounded once to fp32. check "norm": the bar on the norm alone (a long list checks
        the rest after its last step only)."""
        self.set_grads(gvals)
        before = None
        if check is True:
            before = (cat64(self.p_nat), cat64(self.p_tor), cat64([t["p"] for t in self.truth]))
        gbits = [None if p.grad is None else p.grad.detach().clone().view(torch.int32) for p in self.p_nat]
        self.opt.step()
        if self.dev.type == "cuda":  # the fused step reads the gradients and never writes them
            for p, b in zip(self.p_nat, gbits):
                assert b is None or torch.equal(p.grad.view(torch.int32), b), "a gradient was written"
        tnorm = None
        if self.max_norm is not None:
            tnorm = torch.nn.utils.clip_grad_norm_(self.p_tor, self.max_norm)
        self.topt.step()
        hyper = [(idx, g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"])
                 for (idx, _), g in zip(self.groups, self.topt.param_groups)]
        norm = truth_step(self.truth, [None if g is None else g.double() for g in gvals], hyper, self.max_norm)
        if check is True:
            self.check(label, before, norm, tnorm)
        elif check == "norm":
            self.check(label, None, norm, tnorm, norm_only=True)
        return norm

    def state_lists(self, key):
        have = [i for i, t in enumerate(self.truth) if t["m"] is not None]
        tk = {"exp_avg": "m", "exp_avg_sq": "v"}[key]
        return (cat64([self.opt.state[self.p_nat[i]][key] for i in have]),
                cat64([self.topt.state[self.p_tor[i]][key] for i in have]), cat64([self.truth[i][tk] for i in have]))

    def check(self, label, before=None, norm=None, tnorm=None, norm_only=False):
        rows = {}
        if not norm_only:
            want = cat64([t["p"] for t in self.truth])
            got, tor = cat64(self.p_nat), cat64(self.p_tor)
            rows["p"] = (rel(got, want), rel(tor, want), FLOOR)
            for key in ("exp_avg", "exp_avg_sq"):
                a, b, c = self.state_lists(key)
                rows[key] = (rel(a, c), rel(b, c), FLOOR)
        if before is not None:
            du = want - before[2]
            rounded = want.float().double() - before[2].float().double()
            rows["update"] = (rel(got - before[0], du), rel(tor - before[1], du), 2 * rel(rounded, du))
        if norm is not None and tnorm is not None:
            rows["norm"] = (abs(float(self.opt.grad_norm) - norm) / norm, abs(float(tnorm) - norm) / norm, FLOOR)
        for name, (ek, et, floor) in rows.items():
            print(f"  {label} {name}: kernel {ek:.2e} torch {et:.2e} floor {floor:.1e}")
        self.table.append((label, rows))
        for name, (ek, et, floor) in rows.items():
            assert ek <= max(2 * et, floor), (label, name, ek, et, floor)
