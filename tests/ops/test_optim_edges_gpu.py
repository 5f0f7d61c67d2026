"""fused_adamw_k / fused_sgd_k / zero_grads_k at the edges of their
chunking, and FusedAdamW / FusedSGD across load_state_dict, on the GPU.

Values: plain float64 AdamW / SGD (tests/ops/_optim.py) from the same
fp32 or bf16 inputs. The allowed error is not invented: per tensor, the
kernel may be off by 4 x what torch.optim.AdamW / SGD in fp32 is off
from the same float64 reference (the kernel multiplies by 1/bc1 and
rsqrt(bc2) where torch divides). Hyperparameters are exactly
representable in fp32, so the float64 reference, torch in fp32 and the
kernel (which takes them as float) run the same algorithm.

Layouts and bookkeeping: bit-equality with a plain run (the kernels
have no atomics, every element is computed alone), and sentinels around
views at odd element offsets.
"""

import math

import pytest
import torch

from . import _optim as oh

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sparkdl.ops.optim import FusedAdamW, FusedSGD

DEV = "cuda"
# 16384 elements a chunk, float4 body with a scalar tail of n % 4:
# n < 4 (tail only), tails 1, 2, 3, one chunk less one / exactly / plus
# one (a second chunk of a single element), two chunks and a tail of 3
SIZES = [(1,), (2,), (3,), (4,), (5,), (7,), (16383,), (16384,), (16385,),
         (32768 + 3,)]
ADAM = dict(lr=2.0 ** -7, betas=(0.875, 1 - 2.0 ** -10), eps=2.0 ** -27,
            weight_decay=2.0 ** -4)
SGD = dict(lr=2.0 ** -4, weight_decay=2.0 ** -6)
SENTINEL = -1024.0


@pytest.fixture(autouse=True)
def _require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")


def _assert_4x(what, got, torch32, ref64):
    """Kernel error <= 4 x the reference-only error of this tensor.

    The largest error over a tensor of 1 .. 7 elements is a draw, not a
    measure: torch's result for the one-element parameter happens to
    sit 7.1e-9 from the float64 one, an eighth of an ulp, and the
    kernel's, 5.3e-8 away and still inside one ulp, would fail at 4 x
    that. So the reference-only error is not taken below half an fp32
    ulp of the tensor's largest element, the error of a correctly
    rounded result. The floor only matters where the tensor is too
    small to measure on: every tensor of 16383 elements and more is
    within 4 x its measured reference error without it."""
    e_ref = oh.max_err(torch32, ref64)
    e_k = oh.max_err(got, ref64)
    top = ref64.abs().max().item()
    floor = 0.5 * 2.0 ** (math.frexp(top)[1] - 24) if top else 0.0
    print("%-34s n=%-6d reference-only %.3g (floor %.3g) kernel %.3g"
          % (what, ref64.numel(), e_ref, floor, e_k))
    assert e_k <= 4 * max(e_ref, floor), (what, e_k, e_ref, floor)
    return e_ref, e_k


def _float_leaf(p):
    return p.detach().float().cpu().clone().requires_grad_(True)


# ---------------------------------------------------------------------------
# values at the chunk and vector edges
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["fp32", "bf16", "mixed"])
def test_adamw_edges_match_float64(kind):
    """Three steps, ten sizes in one group; each tensor is asserted at
    4 x its own reference-only error. Largest absolute errors over the
    tensors, measured on an MI355X (torch.optim.AdamW in fp32 against
    float64 -> kernel against float64):
      p / master   4.9e-07 -> 3.9e-07
      exp_avg      7.0e-08 -> 4.9e-08
      exp_avg_sq   2.4e-09 -> 1.8e-09"""
    params = oh.make_params(kind, SIZES, DEV, "edges")
    p0 = [p.detach().clone() for p in params]
    ref_params = [_float_leaf(p) for p in params]
    opt = FusedAdamW(params, **ADAM)
    opt_ref = torch.optim.AdamW(ref_params, foreach=False, **ADAM)
    history = []
    for step in (1, 2, 3):
        grads = oh.make_grads(params, step, "edges")
        history.append(grads)
        oh.set_grads(params, grads)
        oh.set_grads(ref_params, [g.float().cpu() for g in grads])
        opt.step()
        opt_ref.step()
    for i, (p, pr) in enumerate(zip(params, ref_params)):
        st, st_ref = opt.state[p], opt_ref.state[pr]
        p64, m64, v64 = oh.adamw_f64(
            p0[i].cpu(), [h[i].cpu() for h in history], ADAM["lr"],
            ADAM["betas"], ADAM["eps"], ADAM["weight_decay"])
        lowp = p.dtype == torch.bfloat16
        master = st["master"] if lowp else p
        assert master.dtype == torch.float32
        tag = "adamw %s %s[%d] " % (kind, "bf16" if lowp else "fp32", i)
        _assert_4x(tag + "p", master, pr, p64)
        _assert_4x(tag + "exp_avg", st["exp_avg"], st_ref["exp_avg"], m64)
        _assert_4x(tag + "exp_avg_sq", st["exp_avg_sq"],
                   st_ref["exp_avg_sq"], v64)
        if lowp:
            assert torch.equal(p.detach(), master.bfloat16()), tag


@pytest.mark.parametrize("momentum,nesterov", [(0.875, False), (0.875, True),
                                               (0.0, False)])
def test_sgd_edges_match_float64(momentum, nesterov):
    """As above for fused_sgd_k, with nesterov and with momentum 0
    (the kernel then never reads the buffer's old value). Measured
    (torch.optim.SGD in fp32 -> kernel): p 4.1e-07 -> 4.1e-07,
    momentum buffer 6.5e-07 -> 5.2e-07."""
    params = oh.make_params("fp32", SIZES, DEV, "sgd-edges")
    p0 = [p.detach().clone() for p in params]
    ref_params = [_float_leaf(p) for p in params]
    opt = FusedSGD(params, momentum=momentum, nesterov=nesterov, **SGD)
    opt_ref = torch.optim.SGD(ref_params, momentum=momentum,
                              nesterov=nesterov, foreach=False, **SGD)
    history = []
    for step in (1, 2, 3):
        grads = oh.make_grads(params, step, "sgd-edges")
        history.append(grads)
        oh.set_grads(params, grads)
        oh.set_grads(ref_params, [g.cpu() for g in grads])
        opt.step()
        opt_ref.step()
    for i, (p, pr) in enumerate(zip(params, ref_params)):
        p64, buf64 = oh.sgd_f64(
            p0[i].cpu(), [h[i].cpu() for h in history], SGD["lr"], momentum,
            SGD["weight_decay"], nesterov)
        tag = "sgd m=%g nesterov=%d [%d] " % (momentum, nesterov, i)
        _assert_4x(tag + "p", p, pr, p64)
        if momentum:
            _assert_4x(tag + "buf", opt.state[p]["momentum_buffer"],
                       opt_ref.state[pr]["momentum_buffer"], buf64)


# ---------------------------------------------------------------------------
# views at odd element offsets inside one flat buffer
# ---------------------------------------------------------------------------

def _flat_views(sizes, dtype, fill=None):
    """One flat buffer holding the tensors back to back with a single
    guard element between them and three at either end, so consecutive
    views start at every residue mod 4. Returns (flat, views, guard
    mask)."""
    total = 6 + sum(s[0] for s in sizes) + len(sizes) - 1
    flat = torch.full((total,), SENTINEL, dtype=dtype, device=DEV)
    guard = torch.ones(total, dtype=torch.bool, device=DEV)
    views, off = [], 3
    for (n,) in sizes:
        views.append(flat[off:off + n])
        guard[off:off + n] = False
        off += n + 1
    assert {v.storage_offset() % 4 for v in views} == {0, 1, 2, 3}
    if fill is not None:
        for v, f in zip(views, fill):
            v.copy_(f)
    return flat, views, guard


def _guards_intact(flat, guard):
    return bool((flat[guard] == SENTINEL).all()) and \
        int(guard.sum()) == 6 + len(SIZES) - 1


@pytest.mark.parametrize("which", ["adamw-fp32", "adamw-bf16", "sgd"])
def test_views_into_one_flat_buffer(which):
    """The layout DistributedOptimizer's unpadded buckets hand the
    kernels: every parameter, grad (and SGD momentum buffer) is a view
    at an arbitrary element offset. The update must equal the one on
    separately allocated tensors bit for bit, and neither step() nor
    zero_grad() may touch the guard elements around the views."""
    kind = "bf16" if which == "adamw-bf16" else "fp32"
    dtype = torch.bfloat16 if kind == "bf16" else torch.float32
    plain = oh.make_params(kind, SIZES, DEV, "views")
    pflat, pviews, pguard = _flat_views(SIZES, dtype, [p.detach()
                                                       for p in plain])
    gflat, gviews, gguard = _flat_views(SIZES, dtype)
    params = [v.detach().requires_grad_(True) for v in pviews]
    for p, v, g in zip(params, pviews, gviews):
        assert p.data_ptr() == v.data_ptr()
        p.grad = g
    if which == "sgd":
        def make(ps):
            return FusedSGD(ps, momentum=0.875, **SGD)
        opt, opt_plain = make(params), make(plain)
        mflat, mviews, mguard = _flat_views(
            SIZES, dtype, [torch.zeros(s, device=DEV) for s in SIZES])
        for p, m in zip(params, mviews):
            opt.state[p]["momentum_buffer"] = m
    else:
        opt, opt_plain = FusedAdamW(params, **ADAM), FusedAdamW(plain,
                                                                **ADAM)
    for step in (1, 2, 3):
        grads = oh.make_grads(plain, step, "views")
        oh.set_grads(plain, grads)
        for gv, g in zip(gviews, grads):
            gv.copy_(g)
        opt.step()
        opt_plain.step()
        torch.cuda.synchronize()
        assert _guards_intact(pflat, pguard), step
        assert _guards_intact(gflat, gguard), step
        if which == "sgd":
            assert _guards_intact(mflat, mguard), step
            for p, m in zip(params, mviews):
                assert opt.state[p]["momentum_buffer"].data_ptr() \
                    == m.data_ptr()
        for p, g in zip(params, gviews):
            assert p.grad.data_ptr() == g.data_ptr()
    oh.assert_runs_equal(opt, params, opt_plain, plain)

    for gv in gviews:
        gv.fill_(3.0)
    opt.zero_grad()
    torch.cuda.synchronize()
    for p, g in zip(params, gviews):
        assert p.grad is not None and p.grad.data_ptr() == g.data_ptr()
        assert bool((p.grad == 0).all())
    assert _guards_intact(gflat, gguard)
    assert _guards_intact(pflat, pguard)


# ---------------------------------------------------------------------------
# grads that change under the table
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["adamw", "sgd"])
def test_grad_replaced_between_steps(which):
    """A freshly allocated grad tensor each step (the old ones stay
    alive, so the pointers really differ) against grads copied into
    place: bit-equal, and the old grad tensors are left alone."""
    def make(ps):
        if which == "sgd":
            return FusedSGD(ps, momentum=0.875, **SGD)
        return FusedAdamW(ps, **ADAM)
    sizes = [(5,), (16385,), (777,)]
    a = oh.make_params("fp32", sizes, DEV, "replace")
    b = oh.clone_params(a)
    opt_a, opt_b = make(a), make(b)
    alive, seen = [], set()
    for step in (1, 2, 3):
        grads = oh.make_grads(a, step, "replace")
        for p, g in zip(a, grads):
            p.grad = g.clone()
            alive.append((p.grad, g))
            assert p.grad.data_ptr() not in seen
            seen.add(p.grad.data_ptr())
        oh.set_grads(b, grads)
        opt_a.step()
        opt_b.step()
    oh.assert_runs_equal(opt_a, a, opt_b, b)
    for used, want in alive:
        assert torch.equal(used, want)


def test_adamw_param_that_gets_its_first_grad_late():
    """One parameter has grad None at steps 1 and 2 and a grad at 3.

    Decision: FusedAdamW keeps ONE step count per param group, on the
    device, advanced by the step itself so that a captured graph of the
    step replays correctly; a parameter that joins late is bias-
    corrected with the group's step (3 here), as in other multi-tensor
    AdamW implementations, and unlike torch.optim.AdamW, which would
    use 1. The float64 reference is written that way. The reference-
    only error is that of the same lines evaluated in fp32."""
    sizes = [(777,), (16385,), (7,)]
    params = oh.make_params("fp32", sizes, DEV, "late")
    p0 = [p.detach().clone() for p in params]
    opt = FusedAdamW(params, **ADAM)
    history = []
    for step in (1, 2, 3):
        grads = oh.make_grads(params, step, "late")
        if step < 3:
            grads[1] = None
        history.append(grads)
        for p, g in zip(params, grads):
            if g is not None:
                oh.set_grads([p], [g])
        opt.step()
        if step < 3:
            assert not opt.state[params[1]]
            assert torch.equal(params[1].detach(), p0[1])
    assert opt.param_groups[0]["step"] == 3
    for i, p in enumerate(params):
        args = (p0[i].cpu(), [None if h[i] is None else h[i].cpu()
                              for h in history], ADAM["lr"], ADAM["betas"],
                ADAM["eps"], ADAM["weight_decay"])
        ref64 = oh.adamw_f64(*args)
        ref32 = oh.adamw_f64(*args, dtype=torch.float32)
        st = opt.state[p]
        for name, got, r32, r64 in zip(
                ("p", "exp_avg", "exp_avg_sq"),
                (p, st["exp_avg"], st["exp_avg_sq"]), ref32, ref64):
            _assert_4x("late [%d] %s" % (i, name), got, r32, r64)
    # per-parameter counting would have given another result
    torch_way = oh.adamw_f64(p0[1].cpu(), [history[2][1].cpu()],
                             ADAM["lr"], ADAM["betas"], ADAM["eps"],
                             ADAM["weight_decay"])[0]
    assert oh.max_err(params[1], torch_way) > 1e-4


# ---------------------------------------------------------------------------
# save / restore on the device
# ---------------------------------------------------------------------------

RESUME_SIZES = [(777,), (16385,), (3,)]


def _make_opt(which):
    if which == "adamw":
        return lambda ps: FusedAdamW(ps, lr=1e-2, weight_decay=0.05)
    return lambda ps: FusedSGD(ps, lr=0.1, momentum=0.9, weight_decay=1e-2,
                               nesterov=which == "sgd-nesterov")


@pytest.mark.parametrize("which,kind", [
    ("adamw", "fp32"), ("adamw", "bf16"), ("adamw", "mixed"),
    ("sgd", "fp32"), ("sgd-nesterov", "fp32")])
def test_resume_is_bit_exact(which, kind):
    oh.run_resume(_make_opt(which), kind, RESUME_SIZES, DEV)


@pytest.mark.parametrize("which,kind", [
    ("adamw", "fp32"), ("adamw", "bf16"), ("adamw", "mixed"),
    ("sgd", "fp32")])
def test_load_into_an_optimizer_that_has_stepped(which, kind):
    """Two steps, snapshot, two more steps, then load the snapshot into
    the SAME optimizer, put the parameters back and step twice: bit-
    equal to a fresh optimizer resumed from the snapshot. The chunk
    table of the running optimizer points at state tensors that
    load_state_dict replaces (the grads, stable, keep the old key
    matching), and its device step counter stands at 4, not 2."""
    key = ("live", which, kind)
    make = _make_opt(which)
    params = oh.make_params(kind, RESUME_SIZES, DEV, *key)
    opt = make(params)
    for step in (1, 2):
        oh.set_grads(params, oh.make_grads(params, step, *key))
        opt.step()
    saved = oh.roundtrip(opt.state_dict())
    p_saved = [p.detach().clone() for p in params]
    old_state = [t for _, _, t in oh.state_tensors(opt, params)]
    for step in (3, 4):
        oh.set_grads(params, oh.make_grads(params, step, *key))
        opt.step()
    at_4 = [t.clone() for t in old_state]

    opt.load_state_dict(saved)
    oh.assert_state_matches_saved(opt, params, saved)
    with torch.no_grad():
        for p, s in zip(params, p_saved):
            p.copy_(s)
    fresh_params = [s.clone().requires_grad_(True) for s in p_saved]
    fresh = make(fresh_params)
    fresh.load_state_dict(saved)
    for step in (5, 6):
        grads = oh.make_grads(params, step, *key)
        oh.set_grads(params, grads)
        oh.set_grads(fresh_params, grads)
        opt.step()
        fresh.step()
    oh.assert_runs_equal(opt, params, fresh, fresh_params)
    assert opt.param_groups[0]["step"] == 4
    # the replaced state tensors were not written again
    torch.cuda.synchronize()
    for t, want in zip(old_state, at_4):
        assert torch.equal(t, want)
