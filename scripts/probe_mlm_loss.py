"""Stand-alone timing of the BERT MLM loss: the fused kernels
(ops.linear_cross_entropy) against the composed path (F.linear on the
library GEMM, bf16 bias add, cast to fp32, F.cross_entropy: what
bert_pretrain_step runs with fused_mlm_loss off), forward and
forward+backward, bf16 operands, at the benchmark's shape: batch 64 x
seq 512 with 15 % masked is about 4915 rows, V = 30522, K = 768.

Device events, a warm-up, the cases alternated round by round in one
process; prints the median (min) us per call, the two losses, and for
each case the peak of torch.cuda.max_memory_allocated over one
forward+backward above what was allocated before it.

Usage: python scripts/probe_mlm_loss.py [M V K] [--rounds R] [--calls K]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import sparkdl.ops as ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", type=int, default=[4915, 30522, 768])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    assert len(args.shape) == 3, "M V K"
    M, V, K = args.shape
    assert torch.cuda.is_available(), "needs the GPU"

    torch.manual_seed(0)
    h = torch.randn(M, K, device="cuda").bfloat16().requires_grad_(True)
    W = (torch.randn(V, K, device="cuda") * 0.02).bfloat16() \
        .requires_grad_(True)
    bias = (torch.randn(V, device="cuda") * 0.02).requires_grad_(True)
    labels = torch.randint(0, V, (M,), device="cuda")
    leaves = (h, W, bias)
    assert ops.linear_cross_entropy_ok(h, W, bias, labels)

    def fused():
        return ops.linear_cross_entropy(h, W, bias, labels)

    def composed():
        logits = F.linear(h, W) + bias.to(torch.bfloat16)
        return F.cross_entropy(logits.float(), labels)

    cases = {"fused": fused, "composed": composed}

    def call(case, backward):
        loss = cases[case]()
        if backward:
            loss.backward()
            for t in leaves:
                t.grad = None
        return loss

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

    print("h [%d, %d] x W [%d, %d], %d rounds x %d calls, median (min) us "
          "per call" % (M, K, V, K, args.rounds, args.calls))
    med = {}
    for (c, b), ts in times.items():
        med[c, b] = statistics.median(ts)
        print("%-9s %-8s %9.1f (%9.1f) us"
              % (c, "fwd+bwd" if b else "fwd", med[c, b], min(ts)),
              flush=True)
    for b in (False, True):
        print("%-8s composed / fused = %.2fx%s"
              % ("fwd+bwd" if b else "fwd",
                 med["composed", b] / med["fused", b],
                 "" if med["fused", b] <= med["composed", b]
                 else "  (the fused path is SLOWER)"))
    for c in cases:
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        loss = call(c, True).item()
        print("%-9s loss %.6f  peak above the operands %.0f MB"
              % (c, loss, (torch.cuda.max_memory_allocated() - base) / 1e6))


if __name__ == "__main__":
    main()
