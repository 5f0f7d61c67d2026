"""The fused vocabulary projection + cross-entropy kernels
(csrc/linear_xent.hip) against an fp64 reference.

Operands make z = h @ W^T + bias exact in fp32: h holds integers in
[-4, 4] over 4, W integers in [-4, 4] over 8, bias multiples of 1/32, so
every partial sum is a multiple of 1/32 far below 2^24 (checked). What
is left is the error of exp, log and the summations:

  per-row loss   (V + 64) 2^-24 + 2^-23 (|lse| + |z_label|): summing V
                 positive fp32 terms in any order, 64 units for exp and
                 log, one rounding each of lse and of the difference
  dZ             one bf16 ulp of the reference + that loss bound x |g|
  dbias          (M + V + 64) 2^-24 x the column's sum of |d_ref|
  sum / mean     the row bounds added up, plus M 2^-24 sum |loss| for
                 the summation in any order (and one rounding for mean)

Shapes (M, V, K): one row, one full tile, one K-step; a second band of
one row and a second tile of one column with a buffer swap; a partial
tile with V % 8 != 0 and an odd number of K-steps; three tiles with
V % 8 == 2 (as 30522) and the padded dZ stride.
"""

import functools

import pytest
import torch

from . import _exact as ex

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import sparkdl.ops as ops

DEV = "cuda"
IGNORE = -100
EPS = 2.0 ** -24
SHAPES = [(1, 256, 64), (257, 257, 128), (255, 250, 192), (300, 522, 128)]
VARIANTS = ["plain", "ignore", "nobias"]
cases = pytest.mark.parametrize("variant", VARIANTS)
shapes = pytest.mark.parametrize("shape", SHAPES, ids=str)


@pytest.fixture(autouse=True)
def _require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")


@functools.lru_cache(maxsize=None)
def _case(shape, variant):
    """Operands on the device and the fp64 reference, once per case."""
    M, V, K = shape
    g = ex.case_generator("lce", M, V, K)
    h = (torch.randint(-4, 5, (M, K), generator=g) / 4).bfloat16().to(DEV)
    W = (torch.randint(-4, 5, (V, K), generator=g) / 8).bfloat16().to(DEV)
    bias = (torch.randint(-32, 33, (V,), generator=g) / 32).to(DEV)
    ex.check_exact_bound(4, 4, K, 32)       # in units of 1/32
    labels = torch.randint(0, V, (M,), generator=g)
    forced = [c for c in (0, 255, 256) if c < V]
    labels[:len(forced)] = torch.tensor(forced)[:M]
    labels[M - 1] = V - 1
    if variant == "ignore":
        labels[0] = labels[M - 1] = IGNORE
    labels = labels.to(DEV)
    if variant == "nobias":
        bias = None
    z = ex.ref_exact(h, W, bias)
    valid = labels != IGNORE
    lse = torch.logsumexp(z, 1)
    zl = z.gather(1, labels.clamp_min(0)[:, None])[:, 0]
    loss = torch.where(valid, lse - zl, torch.zeros_like(lse))
    tol = (V + 64) * EPS + 2 * EPS * (lse.abs() + zl.abs())
    onehot = torch.nn.functional.one_hot(labels.clamp_min(0), V)
    dz_unit = (torch.softmax(z, 1) - onehot) * valid[:, None]
    return dict(h=h, W=W, bias=bias, labels=labels, valid=valid, loss=loss,
                tol=tol, dz_unit=dz_unit)


def _bf16_ulp(x):
    return torch.ldexp(torch.ones_like(x), torch.frexp(x)[1] - 8)


@shapes
@cases
def test_forward(shape, variant):
    c = _case(shape, variant)
    C = ops.ext()
    args = (c["h"], c["W"], c["bias"], c["labels"], IGNORE)
    loss, lse, count = C.lce_forward(*args)
    err = (loss.double() - c["loss"]).abs()
    print("loss: worst err/bound %.3f" % (err / c["tol"]).max().item())
    assert bool((err <= c["tol"]).all()), (err / c["tol"]).max().item()
    assert bool((loss[~c["valid"]] == 0).all())
    n = int(c["valid"].sum())
    assert count.item() == n
    again = C.lce_forward(*args)
    assert all(torch.equal(a, b) for a, b in zip((loss, lse, count), again))
    total = c["loss"].sum().item()
    tol = (c["tol"] * c["valid"]).sum().item() + shape[0] * EPS * total
    for reduction, div in (("sum", 1), ("mean", max(n, 1))):
        got = C.lce_forward(*args, reduction)[0]
        assert got.shape == ()
        err = abs(got.item() - total / div)
        bound = tol / div + EPS * total / div
        print("%s: err %.3g bound %.3g" % (reduction, err, bound))
        assert err <= bound, (reduction, err, bound)


@shapes
@cases
def test_backward(shape, variant):
    c = _case(shape, variant)
    C = ops.ext()
    M, V, _ = shape
    loss, lse, count = C.lce_forward(c["h"], c["W"], c["bias"], c["labels"],
                                     IGNORE)
    gout = torch.tensor([0.75], device=DEV)
    args = (c["h"], c["W"], c["bias"], c["labels"], lse, gout, count, IGNORE)
    dz, dbias = C.lce_backward(*args)
    g = 0.75 / max(int(c["valid"].sum()), 1)
    ref = c["dz_unit"] * g
    err = (dz.double() - ref).abs()
    tol = _bf16_ulp(ref) + c["tol"][:, None] * g
    print("dZ: worst err/bound %.3f" % (err / tol).max().item())
    assert dz.shape == (M, V) and bool((err <= tol).all())
    assert bool((dz[~c["valid"]] == 0).all())
    ldz = dz.stride(0)
    assert ldz % 64 == 0 and ldz >= V and dz.stride(1) == 1
    store = torch.as_strided(dz, (M, ldz), (ldz, 1))
    assert bool((store[:, V:] == 0).all()), "padding columns"
    err = (dbias.double() - ref.sum(0)).abs()
    tol = (M + V + 64) * EPS * ref.abs().sum(0)
    print("dbias: worst err/bound %.3f"
          % (err / tol.clamp_min(1e-300)).max().item())
    assert dbias.shape == (V,) and bool((err <= tol).all())
    again = C.lce_backward(*args)
    assert torch.equal(store, torch.as_strided(again[0], (M, ldz), (ldz, 1)))
    assert torch.equal(dbias, again[1])


@pytest.mark.parametrize("reduction", ["mean", "none"])
def test_autograd_dh_dw(reduction):
    """dh and dW (library GEMMs on the bf16 dZ) and dbias through
    ops.linear_cross_entropy; "none" backpropagates one weight per row."""
    c = _case((300, 522, 128), "ignore")
    h, W, bias = (t.detach().clone().requires_grad_(True)
                  for t in (c["h"], c["W"], c["bias"]))
    loss = ops.linear_cross_entropy(h, W, bias, c["labels"], IGNORE,
                                    reduction)
    if reduction == "mean":
        gr = torch.full((300, 1), 1.0 / int(c["valid"].sum()), device=DEV)
        loss.backward()
    else:
        gr = (torch.arange(300, device=DEV) % 7 - 3)[:, None] / 4
        loss.backward(gr[:, 0])
    dz = c["dz_unit"] * gr
    r = 2.0 ** -8
    h64, W64 = c["h"].double(), c["W"].double()
    for got, ref, mag in (
            (h.grad, dz @ W64, dz.abs() @ W64.abs()),
            (W.grad, dz.t() @ h64, dz.abs().t() @ h64.abs())):
        err = (got.double() - ref).abs()
        tol = r * mag + r * ref.abs()
        print("worst err/bound %.3f"
              % (err / tol.clamp_min(1e-300)).max().item())
        assert got.dtype == torch.bfloat16 and bool((err <= tol).all())
    err = (bias.grad.double() - dz.sum(0)).abs()
    assert bool((err <= (300 + 522 + 64) * EPS * dz.abs().sum(0)).all())


def test_graph_replays_match_eager():
    c = _case((257, 257, 128), "ignore")
    C = ops.ext()
    gout = torch.tensor([0.75], device=DEV)

    def run():
        loss, lse, count = C.lce_forward(c["h"], c["W"], c["bias"],
                                         c["labels"], IGNORE, "mean")
        dz, dbias = C.lce_backward(c["h"], c["W"], c["bias"], c["labels"],
                                   lse, gout, count, IGNORE)
        return loss, dz.contiguous(), dbias

    want = [t.clone() for t in run()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = run()
    for _ in range(3):
        for t in got:
            t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_ragged_k_takes_the_composed_ops():
    g = ex.case_generator("lce-fallback")
    h = torch.randn(5, 96, generator=g).bfloat16().to(DEV).requires_grad_()
    W = torch.randn(33, 96, generator=g).bfloat16().to(DEV).requires_grad_()
    bias = torch.randn(33, generator=g).to(DEV).requires_grad_()
    labels = torch.randint(0, 33, (5,), generator=g).to(DEV)
    assert not ops.linear_cross_entropy_ok(h, W, bias, labels)
    ops.linear_cross_entropy(h, W, bias, labels).backward()
    got = [h.grad, W.grad, bias.grad]
    h.grad = W.grad = bias.grad = None
    logits = torch.nn.functional.linear(h, W) + bias.to(torch.bfloat16)
    want = torch.nn.functional.cross_entropy(logits.float(), labels)
    want.backward()
    assert torch.equal(ops.linear_cross_entropy(h, W, bias, labels), want)
    assert all(torch.equal(a, b)
               for a, b in zip(got, [h.grad, W.grad, bias.grad]))
