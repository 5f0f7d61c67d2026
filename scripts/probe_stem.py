"""Stand-alone timing of the ResNet stem epilogue, BatchNorm + ReLU +
MaxPool2d(3, 2, 1): the fused kernel chain (batch_norm_relu_maxpool)
against the composed path (batch_norm_act + torch max_pool2d,
SPARKDL_FUSED_STEM=0), forward and forward+backward, bf16 channels_last.

Device events, a warm-up, the cases alternated round by round in one
process; prints the median us per call and the effective TB/s over the
bytes each path moves, counted from the shapes:

  E = N*C*H*W elements, P = N*C*Ho*Wo pooled elements
  both, forward:  statistics read x (2E)
  fused fwd:      x in (2E), pooled (2P) + codes (P) out
  fused bwd:      reduce x, pooled grad, codes in (2E + 3P);
                  apply the same in, dx out (4E + 3P)
  composed fwd:   x in, y + mask out (4E + E/8); pool y in, pooled +
                  int64 indices out (2E + 10P)
  composed bwd:   pool grad + indices in, dy out (2E + 10P); reduce x,
                  dy, mask in (4E + E/8); apply the same in, dx out
                  (6E + E/8)

Usage: python scripts/probe_stem.py [N C H W] [--rounds R] [--calls K]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import sparkdl.ops as ops  # noqa: E402


def traffic(shape):
    N, C, H, W = shape
    E = N * C * H * W
    P = N * C * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1)
    fused_f = 2 * E + 2 * E + 3 * P
    fused_b = (2 * E + 3 * P) + (4 * E + 3 * P)
    comp_f = 2 * E + (4 * E + E // 8) + (2 * E + 10 * P)
    comp_b = (2 * E + 10 * P) + (4 * E + E // 8) + (6 * E + E // 8)
    return {"fused": (fused_f, fused_f + fused_b),
            "composed": (comp_f, comp_f + comp_b)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", type=int,
                    default=[512, 64, 112, 112])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    shape = tuple(args.shape)
    N, C, H, W = shape
    assert torch.cuda.is_available(), "needs the GPU"

    torch.manual_seed(0)
    x = torch.randn(shape, device="cuda").bfloat16() \
        .to(memory_format=torch.channels_last).requires_grad_(True)
    gamma = (torch.rand(C, device="cuda") + 0.5).requires_grad_(True)
    beta = torch.randn(C, device="cuda").requires_grad_(True)
    rm = torch.zeros(C, device="cuda")
    rv = torch.ones(C, device="cuda")
    pshape = (N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
    dy = torch.randn(pshape, device="cuda").bfloat16() \
        .to(memory_format=torch.channels_last)

    cases = {"fused": "1", "composed": "0"}  # SPARKDL_FUSED_STEM

    def call(case, backward):
        os.environ["SPARKDL_FUSED_STEM"] = cases[case]
        y = ops.batch_norm_relu_maxpool(x, gamma, beta, rm, rv)
        if backward:
            y.backward(dy)
            x.grad = gamma.grad = beta.grad = None

    def timed(case, backward):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.calls):
            call(case, backward)
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / args.calls  # us per call

    runs = [(c, b) for b in (False, True) for c in cases]
    for c, b in runs:  # warm-up
        for _ in range(3):
            call(c, b)
    torch.cuda.synchronize()
    times = {r: [] for r in runs}
    for _ in range(args.rounds):
        for r in runs:
            times[r].append(timed(*r))

    nbytes = traffic(shape)
    print("shape %s, %d rounds x %d calls, median (min) us per call"
          % (shape, args.rounds, args.calls))
    for (c, b), ts in times.items():
        by = nbytes[c][int(b)]
        med = statistics.median(ts)
        print("%-9s %-8s %9.1f (%9.1f) us  %6.0f MB  %5.2f TB/s"
              % (c, "fwd+bwd" if b else "fwd", med, min(ts), by / 1e6,
                 by / med / 1e6), flush=True)
    print("max_memory_allocated %.0f MB"
          % (torch.cuda.max_memory_allocated() / 1e6))


if __name__ == "__main__":
    main()
