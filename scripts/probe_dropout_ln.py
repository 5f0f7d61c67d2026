"""Stand-alone timing of the BERT sublayer tail ln(res + dropout(x)):
the fused kernels (ops.dropout_add_layer_norm) against the composed path
(torch dropout, torch add, ops.layer_norm: what BertLayer runs with
fused_dropout_ln off), forward and forward+backward, bf16, training
mode.

Device events, a warm-up, the cases alternated round by round in one
process; prints the median (min) us per call and the effective TB/s over
the bytes each path moves, counted from the shapes (gamma, beta, the
statistics and the dgamma / dbeta partials left out: a few rows):

  E = rows * cols elements
  composed fwd:  dropout x in, dropped + bool mask out (2E + 2E + E);
                 add two in, h out (6E); LayerNorm h in, y out (4E): 15E
  composed bwd:  LayerNorm backward h, dy in, dh out (6E); masked scale
                 dh, mask in, dx out (2E + E + 2E): 11E
  fused fwd:     x, res in, h, y out: 8E
  fused bwd:     h, dy in, d_res, d_sub out: 8E

Usage: python scripts/probe_dropout_ln.py [ROWS COLS] [--p P]
                                          [--rounds R] [--calls K]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import sparkdl.ops as ops  # noqa: E402


def traffic(shape):
    E = shape[0] * shape[1]
    return {"fused": (8 * E, 16 * E), "composed": (15 * E, 26 * E)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", type=int, default=[64 * 512, 768])
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    shape = tuple(args.shape)
    assert len(shape) == 2, "ROWS COLS"
    assert torch.cuda.is_available(), "needs the GPU"

    torch.manual_seed(0)
    x = torch.randn(shape, device="cuda").bfloat16().requires_grad_(True)
    res = torch.randn(shape, device="cuda").bfloat16().requires_grad_(True)
    gamma = (torch.rand(shape[1], device="cuda") + 0.5).requires_grad_(True)
    beta = torch.randn(shape[1], device="cuda").requires_grad_(True)
    dy = torch.randn(shape, device="cuda").bfloat16()
    leaves = (x, res, gamma, beta)

    def fused():
        return ops.dropout_add_layer_norm(x, res, gamma, beta, p=args.p,
                                          training=True)

    def composed():
        return ops.layer_norm(
            res + torch.nn.functional.dropout(x, args.p, True), gamma, beta)

    cases = {"fused": fused, "composed": composed}

    def call(case, backward):
        y = cases[case]()
        if backward:
            y.backward(dy)
            for t in leaves:
                t.grad = None

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
    print("shape %s p=%g, %d rounds x %d calls, median (min) us per call"
          % (shape, args.p, args.rounds, args.calls))
    med = {}
    for (c, b), ts in times.items():
        by = nbytes[c][int(b)]
        med[c, b] = statistics.median(ts)
        print("%-9s %-8s %9.1f (%9.1f) us  %6.0f MB  %5.2f TB/s"
              % (c, "fwd+bwd" if b else "fwd", med[c, b], min(ts),
                 by / 1e6, by / med[c, b] / 1e6), flush=True)
    for b in (False, True):
        print("%-8s composed / fused = %.2fx%s"
              % ("fwd+bwd" if b else "fwd",
                 med["composed", b] / med["fused", b],
                 "" if med["fused", b] <= med["composed", b]
                 else "  (the fused path is SLOWER)"))
    print("max_memory_allocated %.0f MB"
          % (torch.cuda.max_memory_allocated() / 1e6))


if __name__ == "__main__":
    main()
