"""Per-site A/B of the hand-written 3x3 convolution (csrc/conv3x3.hip)
against MIOpen at the four stride-1 3x3 sites of ResNet-50, batch 512,
bf16 channels_last: forward, data gradient and weight gradient
(``--passes``), same tensors, same process. ``--stride 2`` does the same
for csrc/conv3x3_s2.hip at the three stride-2 sites, forward and data
gradient. The two paths alternate
window by window; each window is ``--reps`` calls between two device events, after warm-up. Prints, per
site and pass, the median microseconds per call of both paths, the
TFLOP/s those give for the 2*N*Ho*Wo*9*Cin*Cout operations of the
convolution, and MIOpen's time over the kernel's (> 1: the kernel is
faster). Needs the GPU."""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # noqa
import argparse
import statistics

import torch

# (H = W, Cin = Cout)
SITES = [(56, 64), (28, 128), (14, 256), (7, 512)]
# the same for --stride 2 (csrc/conv3x3_s2.hip): H = W of the input; the
# three convolutions that open stages 2, 3 and 4. Forward and dgrad only.
SITES_S2 = [(56, 128), (28, 256), (14, 512)]


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
    ap.add_argument("--stride", type=int, default=1, choices=(1, 2))
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
    st = args.stride
    print("batch %d, stride %d, %d windows of %d calls, median; us per call"
          % (n, st, args.windows, args.reps))
    for hw, c in (SITES if st == 1 else SITES_S2):
        ho = (hw - 1) // st + 1
        g = torch.Generator(device="cuda").manual_seed(hw)
        x = torch.randn(n, c, hw, hw, device="cuda", generator=g) \
            .bfloat16().to(memory_format=cl)
        dy = torch.randn(n, c, ho, ho, device="cuda", generator=g) \
            .bfloat16().to(memory_format=cl)
        w = (torch.randn(c, c, 3, 3, device="cuda", generator=g)
             * (2.0 / (9 * c)) ** 0.5).bfloat16().to(memory_format=cl)
        xp, dyp = x.permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1)
        wf = w.permute(0, 2, 3, 1).contiguous()
        wb = w.flip(2, 3).permute(1, 2, 3, 0).contiguous()
        wd = w.permute(1, 2, 3, 0).contiguous()  # unflipped [Cin,3,3,Cout]

        def fwd_lib():
            return torch.nn.functional.conv2d(x, w, stride=st, padding=1)

        def dgrad_lib():
            return conv_bwd(dy, x, w, None, [st, st], [1, 1], [1, 1], False,
                            [0, 0], 1, [True, False, False])[0]

        def wgrad_lib():
            return conv_bwd(dy, x, w, None, [st, st], [1, 1], [1, 1], False,
                            [0, 0], 1, [False, True, False])[1]

        if st == 1:
            ours = (("fwd", lambda: C.conv3x3(xp, wf), fwd_lib),
                    ("dgrad", lambda: C.conv3x3(dyp, wb), dgrad_lib),
                    ("wgrad", lambda: C.conv3x3_wgrad(xp, dyp), wgrad_lib))
        else:
            ours = (("fwd", lambda: C.conv3x3_s2(xp, wf), fwd_lib),
                    ("dgrad", lambda: C.conv3x3_s2_dgrad(dyp, wd, hw, hw),
                     dgrad_lib))
        passes = [p for p in ours if p[0] in args.passes.split(",")]
        # same results first: fp32 accumulation on both sides, so the
        # difference is summation order and one bf16 rounding
        for name, ours, theirs in passes:
            got, ref = ours(), theirs().permute(0, 2, 3, 1)
            err = (got.float() - ref.float()).abs().max().item()
            scale = ref.float().abs().max().item()
            assert err <= 2.0 ** -6 * scale, (hw, c, name, err, scale)
        flop = 2.0 * n * ho * ho * 9 * c * c
        for name, ours, theirs in passes:
            t, m = ab(ours, theirs, args.reps, args.windows)
            print("%2dx%-2d C=%3d %-5s  conv3x3 %8.1f us %6.1f TF   "
                  "miopen %8.1f us %6.1f TF   miopen/conv3x3 %.2f"
                  % (hw, hw, c, name, t, flop / t / 1e6, m, flop / m / 1e6,
                     m / t), flush=True)


if __name__ == "__main__":
    main()
