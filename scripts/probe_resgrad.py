"""Stand-alone timing of a bottleneck's bn3 (BatchNorm + residual add +
ReLU) whose output has two consumers, forward + backward with two
incoming gradients, at the four residual sites of ResNet-50 at batch
512, bf16 channels_last: the two-gradient backward (bn_bwd2) against
the composed path (SPARKDL_FUSED_RESGRAD=0: autograd adds the two
gradients, then the one-gradient kernels run).

Device events, a warm-up, the cases alternated round by round in one
process; prints the median us per call for forward+backward and for the
forward alone, their difference as the backward's time, and the
backward's effective TB/s over the bytes it moves, counted from the
shapes:

  A = 2*N*C*H*W bytes, one bf16 tensor
  composed bwd:  add u, v in, dy out (3A); reduce x, dy, mask in
                 (2A + A/16); apply x, dy, mask in, dx, dres out
                 (4A + A/16)                          = 9A + 2A/16
  fused bwd:     reduce x, u, v, mask in, s out (4A + A/16); apply
                 x, s in, dx out (3A)                 = 7A + A/16

Usage: python scripts/probe_resgrad.py [--rounds R] [--calls K]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import sparkdl.ops as ops  # noqa: E402

SITES = [(512, 256, 56, 56), (512, 512, 28, 28), (512, 1024, 14, 14),
         (512, 2048, 7, 7)]
CASES = {"fused": "1", "composed": "0"}  # SPARKDL_FUSED_RESGRAD


def bwd_bytes(shape):
    N, C, H, W = shape
    A = 2 * N * C * H * W
    return {"fused": 7 * A + A // 16, "composed": 9 * A + 2 * A // 16}


def probe(shape, rounds, calls):
    C = shape[1]

    def act(requires_grad=False):
        return torch.randn(shape, device="cuda").bfloat16() \
            .to(memory_format=torch.channels_last) \
            .requires_grad_(requires_grad)

    x, r = act(True), act(True)
    ga, gb = act(), act()
    gamma = (torch.rand(C, device="cuda") + 0.5).requires_grad_(True)
    beta = torch.randn(C, device="cuda").requires_grad_(True)
    rm = torch.zeros(C, device="cuda")
    rv = torch.ones(C, device="cuda")

    def call(case, backward):
        os.environ["SPARKDL_FUSED_RESGRAD"] = CASES[case]
        y, y2 = ops.batch_norm_act(x, gamma, beta, rm, rv, relu=True,
                                   residual=r, fork=True)
        if backward:
            torch.autograd.backward([y, y2], [ga, gb])
            x.grad = r.grad = gamma.grad = beta.grad = None

    def timed(case, backward):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            call(case, backward)
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / calls  # us per call

    runs = [(c, b) for b in (False, True) for c in CASES]
    for c, b in runs:  # warm-up
        for _ in range(3):
            call(c, b)
    torch.cuda.synchronize()
    times = {run: [] for run in runs}
    for _ in range(rounds):
        for run in runs:
            times[run].append(timed(*run))

    nbytes = bwd_bytes(shape)
    print("shape %s, %d rounds x %d calls, median (min) us per call"
          % (shape, rounds, calls))
    for c in CASES:
        fwd = statistics.median(times[(c, False)])
        both = statistics.median(times[(c, True)])
        bwd = both - fwd
        print("%-9s fwd %8.1f (%8.1f)  fwd+bwd %8.1f (%8.1f)  "
              "bwd %8.1f us  %6.0f MB  %5.2f TB/s"
              % (c, fwd, min(times[(c, False)]), both,
                 min(times[(c, True)]), bwd, nbytes[c] / 1e6,
                 nbytes[c] / bwd / 1e6), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    torch.manual_seed(0)
    for shape in SITES:
        probe(shape, args.rounds, args.calls)
    print("max_memory_allocated %.0f MB"
          % (torch.cuda.max_memory_allocated() / 1e6))


if __name__ == "__main__":
    main()
