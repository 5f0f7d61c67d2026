"""Saving and restoring FusedAdamW / FusedSGD state (no GPU needed).

torch.optim.Optimizer.load_state_dict casts floating state to the
parameter's dtype; for bf16 parameters that would turn the fp32 master
weights and moments into bf16. The fused optimizers must hand back what
was saved: fp32, bit for bit, and a resumed run must continue exactly
like the uninterrupted one. The same protocol runs on the device in
test_optim_edges_gpu.py.
"""

import os

import pytest
import torch

from sparkdl.ops.optim import FusedAdamW, FusedSGD, _MultiTensorTable

from . import _optim as oh

CPU = "cpu"
SIZES = [(777,), (5, 3), (3,), (16385,)]


def _adamw(params):
    return FusedAdamW(params, lr=1e-2, weight_decay=0.05)


@pytest.mark.parametrize("kind", ["fp32", "bf16", "mixed"])
def test_adamw_resume_is_bit_exact(kind):
    opt_a, params_a, opt_b, params_b = oh.run_resume(
        _adamw, kind, SIZES, CPU)
    for p in params_b:
        st = opt_b.state[p]
        assert ("master" in st) == (p.dtype == torch.bfloat16)
        if "master" in st:
            assert torch.equal(p.detach(), st["master"].bfloat16())
    assert opt_b.param_groups[0]["step"] == 5


@pytest.mark.parametrize("nesterov", [False, True])
def test_sgd_resume_is_bit_exact(nesterov):
    def make(params):
        return FusedSGD(params, lr=0.1, momentum=0.9, weight_decay=1e-2,
                        nesterov=nesterov)
    opt_a, params_a, opt_b, params_b = oh.run_resume(
        make, "fp32", SIZES, CPU)
    assert all("momentum_buffer" in opt_b.state[p] for p in params_b)


def test_resume_keeps_the_memory_format_of_the_state():
    """A channels_last conv weight has a channels_last momentum buffer
    (zeros_like); the kernels pair the two by position in memory, so
    the restored buffer must keep those strides."""
    def weight():
        g = oh.case_generator("channels_last")
        w = torch.randn(8, 4, 3, 3, generator=g)
        return w.to(memory_format=torch.channels_last).requires_grad_(True)
    a, b = weight(), weight()
    opt_a = FusedSGD([a], lr=0.1, momentum=0.9)
    opt_b = FusedSGD([b], lr=0.1, momentum=0.9)
    for opt, p in ((opt_a, a), (opt_b, b)):
        p.grad = torch.ones_like(p)
        opt.step()
    assert opt_a.state[a]["momentum_buffer"].stride() == a.stride()
    opt_b.load_state_dict(oh.roundtrip(opt_a.state_dict()))
    buf = opt_b.state[b]["momentum_buffer"]
    assert buf.stride() == b.stride() and not buf.is_contiguous()
    assert torch.equal(buf, opt_a.state[a]["momentum_buffer"])


def test_load_does_not_alias_the_loaded_dict():
    """Stepping after a load must not write into the dict that was
    loaded (torch's .to() returns the same tensor when nothing has to
    be cast)."""
    params = oh.make_params("fp32", [(9,)], CPU, "alias")
    opt = _adamw(params)
    oh.set_grads(params, oh.make_grads(params, 1, "alias"))
    opt.step()
    saved = oh.roundtrip(opt.state_dict())
    before = saved["state"][0]["exp_avg"].clone()
    opt2 = _adamw(oh.clone_params(params))
    opt2.load_state_dict(saved)
    oh.set_grads(opt2.param_groups[0]["params"],
                 oh.make_grads(params, 2, "alias"))
    opt2.step()
    assert torch.equal(saved["state"][0]["exp_avg"], before)


def test_load_drops_tables_and_step_counter():
    """The chunk tables and the device step counter describe the state
    tensors that load_state_dict has just replaced."""
    params = oh.make_params("fp32", [(9,)], CPU, "drop")
    for opt in (_adamw(params), FusedSGD(params, lr=0.1, momentum=0.9)):
        oh.set_grads(params, oh.make_grads(params, 1, "drop"))
        opt.step()
        opt._tables[0] = object()
        if isinstance(opt, FusedAdamW):
            opt._step_state[0] = object()
        opt.load_state_dict(oh.roundtrip(opt.state_dict()))
        assert opt._tables == {}
        assert getattr(opt, "_step_state", {}) == {}


def test_load_refuses_state_that_is_not_fp32():
    """A dict whose fp32 state was already downcast is an error, not
    something to upcast quietly."""
    params = oh.make_params("bf16", [(9,)], CPU, "refuse")
    opt = _adamw(params)
    oh.set_grads(params, oh.make_grads(params, 1, "refuse"))
    opt.step()
    saved = oh.roundtrip(opt.state_dict())
    saved["state"][0]["master"] = saved["state"][0]["master"].bfloat16()
    with pytest.raises(TypeError, match="master"):
        _adamw(oh.clone_params(params)).load_state_dict(saved)


def test_checkpoint_roundtrip_with_optimizer(tmp_path):
    """save_checkpoint / load_checkpoint with a bf16 model trained by
    FusedAdamW: the path bench-style BERT training resumes through."""
    from sparkdl.utils import save_checkpoint, load_checkpoint
    torch.manual_seed(11)
    model = torch.nn.Linear(7, 5).bfloat16()
    opt = _adamw(model.parameters())
    x = torch.randn(4, 7).bfloat16()
    for _ in range(3):
        opt.zero_grad()
        model(x).float().square().sum().backward()
        opt.step()
    path = os.path.join(tmp_path, "ck.pt")
    save_checkpoint(path, model, opt, step=3)
    want = {k: {n: t.clone() for n, t in opt.state[p].items()}
            for k, p in enumerate(model.parameters())}

    model2 = torch.nn.Linear(7, 5).bfloat16()
    opt2 = _adamw(model2.parameters())
    step, _ = load_checkpoint(path, model2, opt2)
    assert step == 3
    for k, p in enumerate(model2.parameters()):
        for n in ("master", "exp_avg", "exp_avg_sq"):
            got = opt2.state[p][n]
            assert got.dtype == torch.float32, (k, n)
            assert torch.equal(got, want[k][n]), (k, n)
    for m, o in ((model, opt), (model2, opt2)):
        o.zero_grad()
        m(x).float().square().sum().backward()
        o.step()
    for p, q in zip(model.parameters(), model2.parameters()):
        assert torch.equal(p, q)
        assert torch.equal(opt.state[p]["master"], opt2.state[q]["master"])


# ---------------------------------------------------------------------------
# chunk table: host-side validation and key
# ---------------------------------------------------------------------------

def _entry(n=8, lowp=False):
    p = torch.zeros(n)
    g = torch.zeros(n, dtype=torch.bfloat16 if lowp else torch.float32)
    pl = torch.zeros(n, dtype=torch.bfloat16) if lowp else None
    return [p, g, torch.zeros(n), torch.zeros(n), pl]


def test_table_accepts_valid_entries_and_keys_every_pointer():
    e32, e16 = _entry(), _entry(lowp=True)
    sgd = [torch.zeros(3), torch.zeros(3), torch.zeros(3), None, None]
    tbl = _MultiTensorTable([tuple(e32), tuple(e16), tuple(sgd)], CPU)
    assert tbl.nblocks == 3
    assert tbl.key == (
        tuple(t.data_ptr() for t in e32[:4]) + (0,),
        tuple(t.data_ptr() for t in e16),
        tuple(t.data_ptr() for t in sgd[:3]) + (0, 0))
    # 16385 elements: two chunks
    assert _MultiTensorTable([tuple(_entry(16385))], CPU).nblocks == 2


@pytest.mark.parametrize("slot,lowp,bad", [
    (0, False, torch.bfloat16),    # p: a bf16 "master"
    (2, False, torch.bfloat16),    # m
    (3, True, torch.bfloat16),     # v, what load_state_dict used to leave
    (1, False, torch.bfloat16),    # g bf16 without pl
    (1, True, torch.float32),      # g fp32 with pl
    (4, True, torch.float32),      # pl fp32
    (2, False, torch.float64),
])
def test_table_refuses_wrong_dtypes(slot, lowp, bad):
    e = _entry(lowp=lowp)
    e[slot] = e[slot].to(bad)
    with pytest.raises(TypeError, match="kernel needs"):
        _MultiTensorTable([tuple(_entry()), tuple(e)], CPU)


def test_table_accepts_channels_last():
    """Conv weights of a channels_last model are dense but not
    contiguous in the default format; the kernels walk memory."""
    e = [torch.zeros(8, 4, 3, 3).to(memory_format=torch.channels_last)
         for _ in range(4)] + [None]
    assert not e[0].is_contiguous()
    assert _MultiTensorTable([tuple(e)], CPU).nblocks == 1


def test_table_refuses_wrong_layouts():
    e = _entry()
    e[2] = torch.zeros(16)[::2]
    with pytest.raises(ValueError, match="contiguous"):
        _MultiTensorTable([tuple(e)], CPU)
    e = _entry()
    e[3] = torch.zeros(9)
    with pytest.raises(ValueError, match="elements"):
        _MultiTensorTable([tuple(e)], CPU)
    e = _entry()
    e[1] = torch.zeros(8, device="meta")
    with pytest.raises(ValueError, match="expected"):
        _MultiTensorTable([tuple(e)], CPU)
