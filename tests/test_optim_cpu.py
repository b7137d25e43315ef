"""lgm_amd/optim.py without a GPU: the exports, the CPU path (torch's own functional forms: bitwise torch.optim.AdamW),
state_dict interchange with torch.optim.AdamW, and the argument errors."""
import os

import pytest
import torch
from torch.optim.lr_scheduler import OneCycleLR

import lgm_amd
from lgm_amd import optim as O
from tests.optim_ref import CHUNK, HP, Arms, Slot


def slots():
    return [Slot((n,)) for n in (1, 14, 300, 0)] + [Slot((8, 4, 3, 3), "cl"), Slot((5, 7))]


def test_exports():
    assert lgm_amd.AdamW is O.AdamW and lgm_amd.clip_grad_norm_ is O.clip_grad_norm_
    assert "AdamW" in lgm_amd.__all__ and "clip_grad_norm_" in lgm_amd.__all__
    assert issubclass(O.AdamW, torch.optim.Optimizer)
    assert CHUNK == 4096
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lgm_optim.h")) as f:
        assert f"#define LGM_OPTIM_CHUNK {CHUNK}" in f.read()


def test_cpu_tensors_equal_torch_bitwise_over_six_scheduled_steps():
    a = Arms(slots(), "cpu", seed=1)
    sn = OneCycleLR(a.opt, max_lr=HP["lr"], total_steps=20, pct_start=0.3)
    st = OneCycleLR(a.topt, max_lr=HP["lr"], total_steps=20, pct_start=0.3)
    for k in range(6):
        assert a.opt.param_groups[0]["lr"] == a.topt.param_groups[0]["lr"]
        assert a.opt.param_groups[0]["betas"] == a.topt.param_groups[0]["betas"]
        a.set_grads(a.draw(10.0 if k % 2 == 0 else 1e-3))
        a.opt.step()
        tn = torch.nn.utils.clip_grad_norm_(a.p_tor, 1.0)
        a.topt.step()
        sn.step()
        st.step()
        assert torch.equal(a.opt.grad_norm, tn)
        for p, q in zip(a.p_nat, a.p_tor):
            assert torch.equal(p, q)
            for key in ("exp_avg", "exp_avg_sq", "step"):
                assert torch.equal(a.opt.state[p][key], a.topt.state[q][key])
            s = a.opt.state[p]
            assert s["step"].dtype == torch.float32 and s["step"].device.type == "cpu" and float(s["step"]) == k + 1
            assert s["exp_avg"].stride() == p.stride()
    # the stand-alone clip on CPU tensors is torch's
    gv = a.draw(10.0)
    a.set_grads(gv)
    assert torch.equal(O.clip_grad_norm_(a.p_nat, 1.0), torch.nn.utils.clip_grad_norm_(a.p_tor, 1.0))
    assert all(torch.equal(p.grad, q.grad) for p, q in zip(a.p_nat, a.p_tor))


def test_state_dict_interchange():
    a = Arms(slots(), "cpu", seed=2)
    for k in range(2):
        a.set_grads(a.draw(1.0))
        a.opt.step()
        torch.nn.utils.clip_grad_norm_(a.p_tor, 1.0)
        a.topt.step()
    sd_n, sd_t = a.opt.state_dict(), a.topt.state_dict()
    assert set(sd_n["param_groups"][0]) == set(sd_t["param_groups"][0])
    assert sd_n["state"].keys() == sd_t["state"].keys()
    assert set(sd_n["state"][0]) == set(sd_t["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    # each loads the other's and goes on identically
    a.opt.load_state_dict(sd_t)
    a.topt.load_state_dict(sd_n)
    assert a.opt.max_grad_norm == 1.0
    a.set_grads(a.draw(1.0))
    a.opt.step()
    torch.nn.utils.clip_grad_norm_(a.p_tor, 1.0)
    a.topt.step()
    for p, q in zip(a.p_nat, a.p_tor):
        assert torch.equal(p, q) and float(a.opt.state[p]["step"]) == 3 == float(a.topt.state[q]["step"])


def test_argument_errors():
    p = torch.zeros(4, requires_grad=True)
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            O.AdamW([p], **kw)
    for kw in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(weight_decay=-1.0),
               dict(max_grad_norm=-1.0)):
        with pytest.raises(ValueError):
            O.AdamW([p], **kw)
    # a flag that arrives through the param_groups (a loaded state_dict) is refused at the step
    opt = O.AdamW([p])
    opt.param_groups[0]["amsgrad"] = True
    p.grad = torch.ones(4)
    with pytest.raises(ValueError, match="amsgrad"):
        opt.step()
    # non-fp32 parameters or gradients
    h = torch.zeros(4, dtype=torch.float64, requires_grad=True)
    h.grad = torch.ones(4, dtype=torch.float64)
    with pytest.raises(TypeError, match="float32"):
        O.AdamW([h]).step()
    b = torch.zeros(4, dtype=torch.bfloat16, requires_grad=True)
    b.grad = torch.ones(4, dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="float32"):
        O.AdamW([b]).step()
    # sparse gradients
    e = torch.zeros(6, 3, requires_grad=True)
    e.grad = torch.sparse_coo_tensor(torch.tensor([[1, 4]]), torch.ones(2, 3), (6, 3))
    with pytest.raises(RuntimeError, match="sparse"):
        O.AdamW([e]).step()
    # parameters on more than one device
    m = torch.zeros(4, device="meta", requires_grad=True)
    m.grad = torch.zeros(4, device="meta")
    q = torch.zeros(4, requires_grad=True)
    q.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="more than one device"):
        O.AdamW([q, m]).step()
    # a parameter retyped behind the same objects (`p.data = ...`) is validated again
    w = torch.zeros(4, requires_grad=True)
    w.grad = torch.ones(4)
    wo = O.AdamW([w])
    wo.step()
    w.data = w.data.double()
    with pytest.raises(TypeError, match="float32"):
        wo.step()
    # no gradient anywhere: nothing happens, no state
    z = torch.ones(3, requires_grad=True)
    zo = O.AdamW([z], max_grad_norm=1.0)
    zo.step()
    assert len(zo.state) == 0 and zo.grad_norm is None and torch.equal(z.detach(), torch.ones(3))
