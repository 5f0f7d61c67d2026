"""Stand-alone timing of a stride-1 1x1 convolution followed by a
training-mode BatchNorm forward at the ResNet-50 sites of batch 512,
bf16 channels_last: today's route (MIOpen convolution under the
committed tuning, then bn_stats_k -> bn_finalize_k -> bn_apply_k)
against the fused route (conv1x1_stats, which reads A once and writes
the BatchNorm partial sums, then bn_finalize_k -> bn_apply_k).

Two measurements per site and route: the convolution alone, and the
convolution with the whole BatchNorm(+ReLU) forward. bn_finalize_k and
bn_apply_k are the same kernels on the same data in both routes, so the
difference between the routes in the second measurement is the
difference up to the coefficients; it decides the routing
(CONV1X1_STATS_SITES in sparkdl/ops/functional.py).

Device events, a warm-up, the cases alternated round by round in one
process; prints the median (min) us per call and the effective TB/s over
the bytes the route has to move, counted from the shapes:

  conv:      A in, C out                       2*M*(K + N)
  conv + BN: today  A in, C out, C in (stats), C in, y out, mask out
             fused  A in, C out,               C in, y out, mask out

Usage: python scripts/probe_conv1x1_bn.py [--rounds R] [--calls K]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import sparkdl.ops as ops  # noqa: E402

# (count per step, N, H, W, Cin, Cout)
SITES = [
    (1, 512, 56, 56, 64, 64),
    (4, 512, 56, 56, 64, 256),
    (2, 512, 56, 56, 256, 64),
    (1, 512, 56, 56, 256, 128),
    (4, 512, 28, 28, 128, 512),
    (6, 512, 14, 14, 256, 1024),
]
ROUTES = ("miopen", "fused")


def probe(site, rounds, calls):
    count, n, h, w, cin, cout = site
    C = ops.ext()
    M = n * h * w
    x = torch.randn(n, cin, h, w, device="cuda").bfloat16() \
        .to(memory_format=torch.channels_last)
    wt = (torch.randn(cout, cin, device="cuda") * (2.0 / cout) ** 0.5) \
        .bfloat16()
    w4 = wt.view(cout, cin, 1, 1)
    x2d = x.permute(0, 2, 3, 1).reshape(M, cin)
    gamma = torch.rand(cout, device="cuda") + 0.5
    beta = torch.randn(cout, device="cuda")
    rm = torch.zeros(cout, device="cuda")
    rv = torch.ones(cout, device="cuda")

    def call(route, bn):
        if route == "miopen":
            y = torch.nn.functional.conv2d(x, w4)
            if bn:
                C.bn_fwd(y.permute(0, 2, 3, 1), None, gamma, beta, rm, rv,
                         0.1, 1e-5, True, True)
        else:
            y, slab = C.conv1x1_stats(x2d, wt)
            if bn:
                C.bn_fwd_slab(y, None, slab, gamma, beta, rm, rv, 0.1,
                              1e-5, True)

    def timed(route, bn):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            call(route, bn)
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / calls  # us per call

    runs = [(r, b) for b in (False, True) for r in ROUTES]
    with torch.no_grad():
        for run in runs:  # warm-up
            for _ in range(3):
                call(*run)
        torch.cuda.synchronize()
        times = {run: [] for run in runs}
        for _ in range(rounds):
            for run in runs:
                times[run].append(timed(*run))

    a, c = 2 * M * cin, 2 * M * cout
    nbytes = {("miopen", False): a + c, ("fused", False): a + c,
              ("miopen", True): a + 4 * c + c // 16,
              ("fused", True): a + 3 * c + c // 16}
    print("site M=%d K=%d N=%d (x%d per step), %d rounds x %d calls, "
          "median (min) us per call" % (M, cin, cout, count, rounds, calls))
    med = {}
    for run in runs:
        med[run] = statistics.median(times[run])
        print("  %-6s %-8s %8.1f (%8.1f) us  %6.0f MB  %5.2f TB/s"
              % (run[0], "conv+bn" if run[1] else "conv", med[run],
                 min(times[run]), nbytes[run] / 1e6,
                 nbytes[run] / med[run] / 1e6), flush=True)
    gain = med[("miopen", True)] - med[("fused", True)]
    print("  fused saves %7.1f us per call, %7.1f us per step"
          % (gain, gain * count), flush=True)
    return gain * count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    torch.backends.cudnn.benchmark = False
    bench._load_miopen_tuning(512)
    torch.manual_seed(0)
    total = 0.0
    for site in SITES:
        g = probe(site, args.rounds, args.calls)
        total += max(g, 0.0)
    print("sites where fused wins, together: %.1f us per step" % total)


if __name__ == "__main__":
    main()
