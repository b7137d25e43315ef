"""The optimizer-step kernels (include/lgm_optim.h, lgm_amd/csrc/optim.hip) and lgm_amd/optim.py on the GPU.

Truth is the float64 CPU evaluation of the header's formulas (tests/optim_ref.py truth_step); torch's own
clip_grad_norm_ + torch.optim.AdamW (fp32, same GPU, same inputs) is measured next to the kernels. Bar, for p, exp_avg,
exp_avg_sq and the norm: kernel error <= max(2 x torch's error, 1e-6) relative L2; for the update p_after - p_before
the floor is 2 x the error of the float64 result rounded once to fp32 (the storage rounding of p dominates it)."""
import pytest
import torch
from torch.optim.lr_scheduler import OneCycleLR

from lgm_amd import LGM, preset
from lgm_amd import _native as nat
from lgm_amd import optim as O
from tests.optim_ref import CHUNK, FLOOR, HP, Arms, Slot, cat64, edge_slots, rel

pytestmark = pytest.mark.gpu

BIG, SMALL = 10.0, 1e-3  # gradient scales: clip active (coef ~ 1e-4 on these lists) and inactive (coef exactly 1)


def small_slots():
    return [Slot((n,)) for n in (5, CHUNK + 1, 300)] + [Slot((8, 4, 3, 3), "cl"), Slot((777,), ("view", 1, 2))]


def scheduled(opt):
    return OneCycleLR(opt, max_lr=HP["lr"], total_steps=20, pct_start=0.3)


def bits(ts):
    return [t.detach().cpu().reshape(-1).view(torch.int32) for t in ts]


def same_bits(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(bits(a), bits(b)))


def states(arms, key):
    return [arms.opt.state[p][key] for p in arms.p_nat if p in arms.opt.state]


def test_six_scheduled_steps_on_the_edge_shapes(cuda):
    """The chunk edges, an empty tensor, channels_last weights, misaligned views, 300 tiny tensors and one of 0.85M
    elements, six steps under OneCycleLR with the clip active and inactive in turn: the bar after every step, and the
    lr and beta1 sequences of torch's arm."""
    a = Arms(edge_slots(), cuda, seed=0)
    for i, s in enumerate(a.slots):
        if isinstance(s.kind, tuple):
            assert (a.p_nat[i].data_ptr() % 16 != 0) == (s.kind[1] % 4 != 0)
    assert a.p_nat[8].is_contiguous(memory_format=torch.channels_last) and not a.p_nat[8].is_contiguous()
    sn, st = scheduled(a.opt), scheduled(a.topt)
    seq_n, seq_t = [], []
    for k in range(6):
        scale = BIG if k % 2 == 0 else SMALL
        seq_n.append((a.opt.param_groups[0]["lr"], a.opt.param_groups[0]["betas"][0]))
        seq_t.append((a.topt.param_groups[0]["lr"], a.topt.param_groups[0]["betas"][0]))
        norm = a.step(a.draw(scale), label=f"step {k + 1}")
        coef = float(min(1.0, 1.0 / (norm + 1e-6)))
        assert (coef < 2e-4) if scale == BIG else (coef == 1.0), (k, norm)
        for i, s in enumerate(a.slots):  # no copy replaced a gradient, in whatever layout it came
            if isinstance(s.kind, tuple):
                assert a.p_nat[i].grad.data_ptr() % 16 == 4 * (s.kind[2] % 4)
        sn.step()
        st.step()
    assert seq_n == seq_t
    assert len({b for _, b in seq_n}) == 6 and len({lr for lr, _ in seq_n}) == 6  # (the scheduler did move both)
    assert a.opt.grad_norm.dim() == 0 and a.opt.grad_norm.device.type == "cuda"
    for p in a.p_nat:
        st8 = a.opt.state[p]
        assert st8["step"].device.type == "cpu" and st8["step"].dtype == torch.float32 and float(st8["step"]) == 6
        assert st8["exp_avg"].stride() == p.stride() and st8["exp_avg_sq"].stride() == p.stride()


def run_native(dev, mode, steps=3, in_place=False):
    """Three steps of the arm under test alone on small_slots(). mode 'fused': AdamW(max_grad_norm=1); 'split': the
    native clip_grad_norm_, then AdamW(max_grad_norm=None). in_place: the gradients are written into the same
    buffers every step; otherwise they are new tensors at new addresses (the old ones stay alive)."""
    a = Arms(small_slots(), dev, seed=3, max_norm=1.0 if mode == "fused" else None, torch_arm=False)
    sched = scheduled(a.opt)
    norms, addresses = [], []
    for k in range(steps):
        gv = a.draw(BIG if k % 2 == 0 else SMALL)
        if in_place and k > 0:
            for p, s, g in zip(a.p_nat, a.slots, gv):
                p.grad.copy_(g.to(dev))
        else:
            a.set_grads(gv, torch_arm=False)
        addresses.append([p.grad.data_ptr() for p in a.p_nat])
        if mode == "split":
            norms.append(O.clip_grad_norm_(a.p_nat, 1.0))
        a.opt.step()
        if mode == "fused":
            norms.append(a.opt.grad_norm)
        sched.step()
    return a, norms, addresses


def test_fused_step_equals_clip_then_step_and_repeats_bitwise(cuda):
    fused, n1, _ = run_native(cuda, "fused")
    again, n2, _ = run_native(cuda, "fused")
    split, n3, _ = run_native(cuda, "split")
    for other, n in ((again, n2), (split, n3)):
        assert same_bits(fused.p_nat, other.p_nat)
        assert same_bits(states(fused, "exp_avg"), states(other, "exp_avg"))
        assert same_bits(states(fused, "exp_avg_sq"), states(other, "exp_avg_sq"))
        assert same_bits(n1, n)
    assert float(n1[0]) > 100 and float(n1[1]) < 1  # both kinds of step were there


def test_gradients_reallocated_between_steps(cuda):
    """zero_grad(set_to_none=True) frees the gradients and the next backward allocates new ones: the pointer table
    follows them. New tensors at new addresses every step (the old ones are held alive) give the bits of a run that
    writes every gradient into the same buffers."""
    moved, _, addr_m = run_native(cuda, "fused")
    fixed, _, addr_f = run_native(cuda, "fused", in_place=True)
    assert all(x != y and y != z and x != z for x, y, z in zip(*addr_m))
    assert addr_f[0] == addr_f[1] == addr_f[2]
    assert same_bits(moved.p_nat, fixed.p_nat)
    assert same_bits(states(moved, "exp_avg_sq"), states(fixed, "exp_avg_sq"))


def test_late_and_missing_gradients(cuda):
    """A parameter whose first gradient arrives at step 3 has its own step count and bias correction; one that never
    gets a gradient gets no state and does not move."""
    a = Arms(small_slots(), cuda, seed=5)
    start = a.p_nat[1].detach().clone()
    for k in range(4):
        skip = {1, 2} if k < 2 else {1}
        a.step(a.draw(BIG if k % 2 == 0 else SMALL, skip), label=f"late {k + 1}")
    assert a.p_nat[1] not in a.opt.state or len(a.opt.state[a.p_nat[1]]) == 0
    assert torch.equal(a.p_nat[1].detach(), start)
    assert float(a.opt.state[a.p_nat[2]]["step"]) == 2 and float(a.opt.state[a.p_nat[0]]["step"]) == 4
    assert float(a.topt.state[a.p_tor[2]]["step"]) == 2


def test_two_param_groups_one_global_norm(cuda):
    groups = [([0, 1, 3], dict(HP)), ([2, 4], dict(HP, lr=1e-3, weight_decay=0.0, betas=(0.8, 0.99)))]
    a = Arms(small_slots(), cuda, seed=7, groups=groups)
    for k in range(3):
        a.step(a.draw(BIG if k % 2 == 0 else SMALL), label=f"groups {k + 1}")


def test_nan_gradient_poisons_every_parameter(cuda):
    a = Arms(small_slots(), cuda, seed=9)
    gv = a.draw(1.0)
    gv[2][17] = float("nan")
    a.step(gv, check=False)
    assert torch.isnan(a.opt.grad_norm)
    for p, q in zip(a.p_nat, a.p_tor):
        assert bool(torch.isnan(q).all()), "torch's arm"
        assert bool(torch.isnan(p).all())
    with pytest.raises(RuntimeError, match="non-finite"):
        O.clip_grad_norm_(a.p_nat, 1.0, error_if_nonfinite=True)


def test_clip_grad_norm_against_torch(cuda):
    """The stand-alone clip: the norm by the bar; the scaled gradients within 1e-6 of torch's and of the truth."""
    slots = edge_slots()
    for scale in (BIG, SMALL):
        a = Arms(slots, cuda, seed=11, max_norm=None)
        gv = a.draw(scale)
        a.set_grads(gv)
        n_nat = O.clip_grad_norm_(a.p_nat, 1.0)
        n_tor = torch.nn.utils.clip_grad_norm_(a.p_tor, 1.0)
        g64 = cat64(gv)
        norm = float(g64.norm())
        coef = min(1.0, 1.0 / (norm + 1e-6))
        ek, et = abs(float(n_nat) - norm) / norm, abs(float(n_tor) - norm) / norm
        got, tor = cat64([p.grad for p in a.p_nat]), cat64([p.grad for p in a.p_tor])
        e_truth, e_torch, t_truth = rel(got, g64 * coef), rel(got, tor), rel(tor, g64 * coef)
        print(f"  clip scale {scale}: norm kernel {ek:.2e} torch {et:.2e}; scaled gradients kernel-truth {e_truth:.2e} "
              f"kernel-torch {e_torch:.2e} torch-truth {t_truth:.2e}")
        assert n_nat.dim() == 0 and n_nat.device.type == "cuda"
        assert ek <= max(2 * et, FLOOR)
        assert e_truth <= 1e-6 and e_torch <= 1e-6
        if scale == SMALL:  # coef exactly 1: nothing moves
            assert same_bits([p.grad for p in a.p_nat], [s.grad(g, cuda, True) for s, g in zip(slots, gv)])


def test_clip_grad_norm_other_cases(cuda):
    # a non-dense gradient (torch accepts any strides): scaled in place through a dense copy
    p = torch.zeros(50, 7, device=cuda, requires_grad=True)
    q = torch.zeros(50, 7, device=cuda, requires_grad=True)
    g = torch.randn(50, 14, device=cuda)
    p.grad, q.grad = g.clone()[:, ::2], g.clone()[:, ::2]
    assert not p.grad.is_contiguous()
    n1, n2 = O.clip_grad_norm_([p], 0.5), torch.nn.utils.clip_grad_norm_([q], 0.5)
    assert abs(float(n1) - float(n2)) <= 1e-6 * float(n2)
    assert rel(p.grad.cpu().double(), q.grad.cpu().double()) <= 1e-6
    # another norm type is torch's own function; a single tensor is a list of one; no gradients: norm 0
    p.grad, q.grad = g[:, :7].clone(), g[:, :7].clone()
    assert torch.equal(O.clip_grad_norm_(p, 0.5, norm_type=1.0), torch.nn.utils.clip_grad_norm_(q, 0.5, norm_type=1.0))
    assert torch.equal(p.grad, q.grad)
    p.grad = None
    assert float(O.clip_grad_norm_([p], 1.0)) == 0.0


def test_state_dict_round_trips(cuda):
    """native -> torch.optim.AdamW -> native: the state of each loads into the other, and one more step after each
    load meets the bar."""
    a = Arms(small_slots(), cuda, seed=13)
    for k in range(2):
        a.step(a.draw(BIG if k % 2 == 0 else SMALL), label=f"state {k + 1}")
    nat_sd, tor_sd = a.opt.state_dict(), a.topt.state_dict()
    assert set(nat_sd["param_groups"][0]) >= set(tor_sd["param_groups"][0])
    # native -> torch: a fresh torch optimizer on the native arm's parameters goes on from the native state
    t2 = torch.optim.AdamW(a.p_nat, **HP)
    t2.load_state_dict(nat_sd)
    native_opt, a.opt = a.opt, None
    gv = a.draw(BIG)
    a.set_grads(gv)
    before = (cat64(a.p_nat), cat64(a.p_tor), cat64([t["p"] for t in a.truth]))
    torch.nn.utils.clip_grad_norm_(a.p_nat, 1.0)
    t2.step()
    torch.nn.utils.clip_grad_norm_(a.p_tor, 1.0)
    a.topt.step()
    from tests.optim_ref import truth_step
    hyper = [(list(range(len(a.slots))), HP["lr"], *HP["betas"], HP["eps"], HP["weight_decay"])]
    truth_step(a.truth, [g.double() for g in gv], hyper, 1.0)
    a.opt = t2  # (the bar on torch's step from the native state)
    a.check("native->torch", before)
    # torch -> native: a fresh native optimizer goes on from that torch state
    n2 = O.AdamW(a.p_nat, max_grad_norm=1.0, **HP)
    n2.load_state_dict(t2.state_dict())
    a.opt = n2
    a.step(a.draw(SMALL), label="torch->native")
    assert float(n2.state[a.p_nat[0]]["step"]) == 4
    # and a fused torch optimizer's state (its steps live on the device)
    t3 = torch.optim.AdamW(a.p_nat, fused=True, **HP)
    for p in a.p_nat:
        p.grad = torch.zeros_like(p)
    t3.step()
    n3 = O.AdamW(a.p_nat, max_grad_norm=1.0, **HP)
    n3.load_state_dict(t3.state_dict())
    n3.step()
    assert float(n3.state[a.p_nat[0]]["step"]) == 2 and n3.state[a.p_nat[0]]["step"].device.type == "cpu"
    del native_opt


def test_profiler_sees_three_launches_and_none_on_errors(cuda):
    a = Arms(small_slots(), cuda, seed=15, torch_arm=False)
    a.set_grads(a.draw(BIG), torch_arm=False)
    a.opt.step()  # (state allocation and the table upload are behind us)
    a.set_grads(a.draw(BIG), torch_arm=False)
    prof = nat.KernelProfiler()
    with prof:
        a.opt.step()
    assert {k: n for k, (n, _) in prof.summary().items()} == {"k_optim_sqnorm": 1, "k_optim_reduce": 1,
                                                              "k_optim_adamw": 1}
    prof.reset()
    L = nat.lib()
    lists = a.opt._lists
    tab, cmap, part = nat.ptr(lists.table), nat.ptr(lists.chunk_tensor), nat.ptr(lists.partials)
    out = torch.zeros(2, device=cuda)
    n, nc, st = len(lists.rows), lists.nchunks, nat.stream_of(cuda)
    hp = (1e-3, 0.9, 0.95, 1e-8, 0.05, 1.0)
    with prof:
        d = nat.diag()
        bad = [L.lgm_optim_grad_norm(None, n, cmap, nc, 1.0, part, nc * 8, nat.ptr(out), st, d),  # null table
               L.lgm_optim_grad_norm(tab, -1, cmap, nc, 1.0, part, nc * 8, nat.ptr(out), st, d),  # negative counts
               L.lgm_optim_grad_norm(tab, n, cmap, -1, 1.0, part, nc * 8, nat.ptr(out), st, d),
               L.lgm_optim_grad_norm(tab, n, cmap, nc, 1.0, part, nc * 8 - 1, nat.ptr(out), st, d),  # short partials
               L.lgm_optim_grad_norm(tab, n, cmap, 2 ** 31, 1.0, part, 2 ** 34, nat.ptr(out), st, d),  # oversize grid
               L.lgm_optim_adamw(None, n, cmap, 0, nc, None, *hp, st, d),
               L.lgm_optim_adamw(tab, n, cmap, -1, nc, None, *hp, st, d),
               L.lgm_optim_adamw(tab, n, cmap, 2 ** 31 - 1, 1, None, *hp, st, d),
               L.lgm_optim_adamw(tab, n, cmap, 0, nc, None, 1e-3, 0.9, 0.95, 1e-8, 0.05, 0.0, st, d),  # step 0
               L.lgm_optim_scale(None, n, cmap, nc, nat.ptr(out), st, d),
               L.lgm_optim_scale(tab, n, cmap, nc, None, st, d),
               L.lgm_optim_scale(tab, n, cmap, 2 ** 31, nat.ptr(out), st, d)]
        assert all(rc < 0 for rc in bad), bad
        assert L.lgm_last_error()
        assert L.lgm_optim_grad_norm(None, 0, None, 0, 1.0, None, 0, None, st, d) == 0  # nothing to do
        assert L.lgm_optim_adamw(None, 0, None, 0, 0, None, *hp, st, d) == 0
        assert L.lgm_optim_scale(None, 0, None, 0, None, st, d) == 0
    assert prof.summary() == {}
    assert L.lgm_optim_workspace_size(nc) == nc * 8 and L.lgm_optim_workspace_size(0) == 0
    prof.close()


def test_lgm_tiny_parameter_list(cuda):
    """LGM(preset('tiny'))'s own parameter list (244 tensors, 59.7M elements) with random gradients, three steps:
    the norm is held to the bar after every step; p, exp_avg, exp_avg_sq (which carry all three steps) and the third
    step's update after the third (the fp64 comparison of 60M elements is what this test's time goes to)."""
    with torch.device("meta"):
        shapes = [tuple(p.shape) for p in LGM(preset("tiny")).parameters() if p.requires_grad]
    assert len(shapes) > 200 and any(torch.Size(s).numel() % 4 for s in shapes)
    a = Arms([Slot(s) for s in shapes], cuda, seed=17)
    sn, st = scheduled(a.opt), scheduled(a.topt)
    for k in range(3):  # (the norm after every step; p, the states and the update after the third)
        a.step(a.draw(BIG if k % 2 == 0 else SMALL), label=f"tiny {k + 1}", check=True if k == 2 else "norm")
        sn.step()
        st.step()
