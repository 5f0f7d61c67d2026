"""Shared pieces of the optimizer tests (test_optim_resume_cpu.py,
test_optim_edges_gpu.py): parameter sets, per-step grads, the
save / restore protocol and plain float64 AdamW / SGD references.

Everything is drawn on the CPU from a generator seeded by the case key
and then moved, so a CPU run and a GPU run see the same values.
"""

import io

import torch

from ._exact import case_generator

FP32_STATE = ("master", "exp_avg", "exp_avg_sq", "momentum_buffer")


def param_dtypes(kind, n):
    """'fp32', 'bf16' (fp32 masters in the optimizer) or 'mixed': the
    two interleaved inside one param group."""
    if kind == "mixed":
        return [torch.float32 if i % 2 == 0 else torch.bfloat16
                for i in range(n)]
    return [torch.float32 if kind == "fp32" else torch.bfloat16] * n


def make_params(kind, sizes, device, *key):
    g = case_generator("params", kind, tuple(sizes), *key)
    return [torch.randn(s, generator=g).to(dt).to(device).requires_grad_(True)
            for s, dt in zip(sizes, param_dtypes(kind, len(sizes)))]


def make_grads(params, step, *key):
    """Fresh grad tensors for ``step`` (1-based), in each parameter's
    dtype; a function of (key, step, index, shape) only."""
    out = []
    for i, p in enumerate(params):
        g = case_generator("grad", step, i, tuple(p.shape), *key)
        out.append(torch.randn(p.shape, generator=g).to(p.dtype)
                   .to(p.device))
    return out


def set_grads(params, grads):
    """Copy into an existing grad (stable pointers) or install it."""
    for p, g in zip(params, grads):
        if p.grad is None:
            p.grad = g.clone()
        else:
            p.grad.copy_(g)


def clone_params(params):
    return [p.detach().clone().requires_grad_(True) for p in params]


def roundtrip(state_dict):
    """state_dict -> torch.save -> bytes -> torch.load."""
    buf = io.BytesIO()
    torch.save(state_dict, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=False)


def state_tensors(opt, params):
    """[(param index, key, tensor)] of the fp32 optimizer state."""
    return [(i, k, opt.state[p][k]) for i, p in enumerate(params)
            for k in FP32_STATE if k in opt.state[p]]


def assert_state_matches_saved(opt, params, saved):
    """After load_state_dict: fp32, and bit-identical to ``saved`` (the
    dict that came out of torch.load)."""
    ids = [pid for g in saved["param_groups"] for pid in g["params"]]
    seen = 0
    for i, k, t in state_tensors(opt, params):
        src = saved["state"][ids[i]][k]
        assert src.dtype == torch.float32, (i, k, src.dtype)
        assert t.dtype == torch.float32, (i, k, t.dtype)
        assert t.shape == params[i].shape, (i, k, t.shape)
        assert t.device == params[i].device, (i, k, t.device)
        assert torch.equal(t.cpu(), src.cpu()), (i, k)
        seen += 1
    assert seen >= len(params)


def assert_runs_equal(opt_a, params_a, opt_b, params_b):
    for i, (a, b) in enumerate(zip(params_a, params_b)):
        assert a.dtype == b.dtype
        assert torch.equal(a.detach(), b.detach()), ("param", i)
    sa, sb = state_tensors(opt_a, params_a), state_tensors(opt_b, params_b)
    assert [(i, k) for i, k, _ in sa] == [(i, k) for i, k, _ in sb]
    for (i, k, ta), (_, _, tb) in zip(sa, sb):
        assert ta.dtype == tb.dtype == torch.float32, (i, k)
        assert torch.equal(ta, tb), (i, k)
    for ga, gb in zip(opt_a.param_groups, opt_b.param_groups):
        assert ga["step"] == gb["step"]


def run_resume(make_opt, kind, sizes, device, before=3, after=2):
    """The protocol of both resume tests: ``before`` steps, state_dict
    through torch.save / torch.load, a fresh optimizer over cloned
    parameters, then ``after`` more steps of both with identical grads.
    Returns nothing; asserts."""
    key = ("resume", kind)
    params_a = make_params(kind, sizes, device, *key)
    opt_a = make_opt(params_a)
    for step in range(1, before + 1):
        set_grads(params_a, make_grads(params_a, step, *key))
        opt_a.step()
    for _, k, t in state_tensors(opt_a, params_a):
        assert t.dtype == torch.float32, k      # what gets saved
    saved = roundtrip(opt_a.state_dict())

    params_b = clone_params(params_a)
    opt_b = make_opt(params_b)
    opt_b.load_state_dict(saved)
    assert_state_matches_saved(opt_b, params_b, saved)

    for step in range(before + 1, before + after + 1):
        grads = make_grads(params_a, step, *key)
        set_grads(params_a, grads)
        set_grads(params_b, grads)
        opt_a.step()
        opt_b.step()
    # loading must not have aliased the loaded dict either
    assert_runs_equal(opt_a, params_a, opt_b, params_b)
    return opt_a, params_a, opt_b, params_b


# ---------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------

def adamw_f64(p0, grads_per_step, lr, betas, eps, wd, first_step=1,
              dtype=torch.float64):
    """Plain float64 AdamW of one tensor. ``grads_per_step`` holds one
    grad (any dtype) or None per optimizer step; the bias correction of
    the k-th entry uses step number ``first_step + k`` whether or not
    earlier entries were None (one step count per group). Returns
    (p, m, v) in float64. ``dtype=torch.float32`` evaluates the same
    lines in fp32: the reference-only error where torch.optim.AdamW
    (one step count per parameter) does not apply."""
    b1, b2 = betas
    p = p0.detach().to(dtype).clone()
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    for k, g in enumerate(grads_per_step):
        if g is None:
            continue
        step = first_step + k
        g = g.to(dtype)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        bc1 = 1 - b1 ** step
        bc2 = 1 - b2 ** step
        p = p * (1 - lr * wd) - (lr / bc1) * m / ((v / bc2).sqrt() + eps)
    return p, m, v


def sgd_f64(p0, grads_per_step, lr, momentum, wd, nesterov):
    """Plain float64 SGD (torch.optim.SGD semantics, dampening 0).
    Returns (p, momentum buffer) in float64."""
    p = p0.detach().double().clone()
    buf = None
    for g in grads_per_step:
        d = g.double() + wd * p
        if momentum != 0.0:
            buf = d.clone() if buf is None else momentum * buf + d
            d = d + momentum * buf if nesterov else buf
        p = p - lr * d
    return p, buf


def max_err(got, ref64):
    return (got.detach().double().cpu() - ref64.cpu()).abs().max().item()
