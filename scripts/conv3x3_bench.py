"""Per-site A/B of the hand-written 3x3 convolution (csrc/conv3x3.hip)
against MIOpen at the four stride-1 3x3 sites of ResNet-50, batch 512,
bf16 channels_last: forward, data gradient and weight gradient
(``--passes``), same tensors, same process. The two paths alternate
window by window; each window is ``--reps`` calls between two device events, after warm-up. Prints, per
site and pass, the median microseconds per call of both paths, the
TFLOP/s those give for the 2*N*H*W*9*Cin*Cout operations of the
convolution, and MIOpen's time over the kernel's (> 1: the kernel is
faster). Needs the GPU."""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # noqa
import argparse
import statistics

import torch

# (H = W, Cin = Cout)
SITES = [(56, 64), (28, 128), (14, 256), (7, 512)]


def window(fn, reps):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1000  # us per call


def ab(ours, theirs, reps, windows):
    for fn in (ours, theirs):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(windows):
        a.append(window(ours, reps))
        b.append(window(theirs, reps))
    return statistics.median(a), statistics.median(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--passes", default="fwd,dgrad,wgrad")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("conv3x3_bench: no GPU")
    import sparkdl.ops as ops
    C = ops.ext()
    # MIOpen as the training benchmark runs it: immediate mode over the
    # committed tuning databases
    import bench
    torch.backends.cudnn.benchmark = False
    bench._load_miopen_tuning(args.batch)
    cl = torch.channels_last
    n = args.batch
    conv_bwd = torch.ops.aten.convolution_backward
    print("batch %d, %d windows of %d calls, median; us per call"
          % (n, args.windows, args.reps))
    for hw, c in SITES:
        g = torch.Generator(device="cuda").manual_seed(hw)
        x = torch.randn(n, c, hw, hw, device="cuda", generator=g) \
            .bfloat16().to(memory_format=cl)
        dy = torch.randn(n, c, hw, hw, device="cuda", generator=g) \
            .bfloat16().to(memory_format=cl)
        w = (torch.randn(c, c, 3, 3, device="cuda", generator=g)
             * (2.0 / (9 * c)) ** 0.5).bfloat16().to(memory_format=cl)
        xp, dyp = x.permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1)
        wf = w.permute(0, 2, 3, 1).contiguous()
        wb = w.flip(2, 3).permute(1, 2, 3, 0).contiguous()

        def fwd_lib():
            return torch.nn.functional.conv2d(x, w, padding=1)

        def dgrad_lib():
            return conv_bwd(dy, x, w, None, [1, 1], [1, 1], [1, 1], False,
                            [0, 0], 1, [True, False, False])[0]

        def wgrad_lib():
            return conv_bwd(dy, x, w, None, [1, 1], [1, 1], [1, 1], False,
                            [0, 0], 1, [False, True, False])[1]

        passes = [p for p in (
            ("fwd", lambda: C.conv3x3(xp, wf), fwd_lib),
            ("dgrad", lambda: C.conv3x3(dyp, wb), dgrad_lib),
            ("wgrad", lambda: C.conv3x3_wgrad(xp, dyp), wgrad_lib))
            if p[0] in args.passes.split(",")]
        # same results first: fp32 accumulation on both sides, so the
        # difference is summation order and one bf16 rounding
        for name, ours, theirs in passes:
            got, ref = ours(), theirs().permute(0, 2, 3, 1)
            err = (got.float() - ref.float()).abs().max().item()
            scale = ref.float().abs().max().item()
            assert err <= 2.0 ** -6 * scale, (hw, c, name, err, scale)
        flop = 2.0 * n * hw * hw * 9 * c * c
        for name, ours, theirs in passes:
            t, m = ab(ours, theirs, args.reps, args.windows)
            print("%2dx%-2d C=%3d %-5s  conv3x3 %8.1f us %6.1f TF   "
                  "miopen %8.1f us %6.1f TF   miopen/conv3x3 %.2f"
                  % (hw, hw, c, name, t, flop / t / 1e6, m, flop / m / 1e6,
                     m / t), flush=True)


if __name__ == "__main__":
    main()
