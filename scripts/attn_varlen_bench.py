"""Flash attention with variable-length (right-padded) batches: time
flash_attention_packed forward and forward+backward at the BERT shape
(B=64, H=12, S=512, bf16) with device events.

Cases (alternated round by round inside one process, after a warm-up):
  none   seq_lens=None (the fixed-length kernels; uses only the API
         that predates seq_lens, so `--cases none` also runs on older
         checkouts for an A/B of the default path)
  full   every length = S      (VARLEN kernels, nothing to skip)
  half   every length = S/2    (about a quarter of the math)
  mixed  seeded uniform lengths over [64, S]

A case may be listed more than once (`--cases none,none`): the repeats
are timed as separate entries, which shows the run-to-run spread.
"""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # noqa
import argparse
import json

import torch
from sparkdl.ops import functional as F_


def make_lens(case, B, S, device):
    if case == "none":
        return None
    if case == "full":
        vals = torch.full((B,), S)
    elif case == "half":
        vals = torch.full((B,), S // 2)
    elif case == "mixed":
        g = torch.Generator().manual_seed(11)
        vals = torch.randint(64, S + 1, (B,), generator=g)
    else:
        raise SystemExit("unknown case %r" % case)
    return vals.to(device=device, dtype=torch.int32)


def timed(fn, iters):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1000  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="none,full,half,mixed")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: timings on a CPU mean nothing")

    B, H, S = args.batch, args.heads, args.seq
    torch.manual_seed(0)
    qkv = torch.randn(B, S, 3, H, 64, device="cuda").bfloat16() \
        .requires_grad_(True)
    do = torch.randn(B, S, H * 64, device="cuda").bfloat16()

    cases = []
    for i, name in enumerate(args.cases.split(",")):
        lens = make_lens(name, B, S, "cuda")
        # `none` calls the op exactly as code without seq_lens does
        call = (lambda: F_.flash_attention_packed(qkv, 0.0)) \
            if lens is None else \
            (lambda lens=lens: F_.flash_attention_packed(
                qkv, 0.0, seq_lens=lens))

        def fwd(call=call):
            with torch.no_grad():
                call()

        def fwd_bwd(call=call):
            qkv.grad = None
            call().backward(do)

        frac = 1.0 if lens is None else \
            float((lens.float() ** 2).mean()) / S ** 2
        cases.append(dict(name="%s#%d" % (name, i), fwd=fwd,
                          fwd_bwd=fwd_bwd, frac=frac, t_fwd=[], t_fb=[]))

    for c in cases:  # warm up every case
        for _ in range(5):
            c["fwd"]()
            c["fwd_bwd"]()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for c in cases:
            c["t_fwd"].append(timed(c["fwd"], args.iters))
            c["t_fb"].append(timed(c["fwd_bwd"], args.iters))

    def stats(ts):
        ts = sorted(ts)
        return ts[len(ts) // 2], ts[0], ts[-1]

    print("attn_varlen_bench %s B=%d H=%d S=%d bf16, %d rounds x %d iters,"
          " us per call: median [min..max]"
          % (args.label, B, H, S, args.rounds, args.iters))
    out = {}
    for c in cases:
        f, fb = stats(c["t_fwd"]), stats(c["t_fb"])
        print("  %-8s len^2/S^2=%.3f  fwd %8.1f [%8.1f..%8.1f]   "
              "fwd+bwd %8.1f [%8.1f..%8.1f]"
              % ((c["name"], c["frac"]) + f + fb), flush=True)
        out[c["name"]] = dict(fwd_us=round(f[0], 1),
                              fwd_bwd_us=round(fb[0], 1))
    print(json.dumps(dict(label=args.label, shape=[B, H, S], us=out)))


if __name__ == "__main__":
    main()
