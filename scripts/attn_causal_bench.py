"""Causal flash attention: time flash_attention_packed forward and
forward+backward at the BERT shape (B=64, H=12, S=512, bf16) with device
events, at dropout 0 and 0.1.

Cases (alternated round by round inside one process, after a warm-up):
  dense   causal=False (uses only the API that predates `causal`, so
          `--cases dense` also runs on older checkouts for an A/B of the
          untouched instantiations)
  causal  causal=True: the triangular tile schedule, 36 of the 64 tile
          pairs at S=512
  sdpa    torch scaled_dot_product_attention(is_causal=True) on the same
          packed buffer, including the permute/contiguous copies into
          [B,H,S,64] and back to [B,S,H*64] that a caller needs today

A case may be listed more than once (`--cases dense,dense`): the repeats
are timed as separate entries, which shows the run-to-run spread.
"""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # noqa
import argparse
import json

import torch
from sparkdl.ops import functional as F_


def timed(fn, iters):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1000  # us per call


def make_call(case, qkv, p):
    if case == "dense":
        return lambda: F_.flash_attention_packed(qkv, p)
    if case == "causal":
        return lambda: F_.flash_attention_packed(qkv, p, causal=True)
    if case == "sdpa":
        B, S, _, H, _ = qkv.shape

        def sdpa():
            q, k, v = (t.contiguous()
                       for t in qkv.permute(2, 0, 3, 1, 4).unbind(0))
            o = torch.nn.functional.scaled_dot_product_attention(
                q, k, v, dropout_p=p, is_causal=True)
            return o.transpose(1, 2).reshape(B, S, H * 64)
        return sdpa
    raise SystemExit("unknown case %r" % case)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="dense,causal,sdpa")
    ap.add_argument("--dropouts", default="0,0.1")
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
    for p in (float(x) for x in args.dropouts.split(",")):
        for i, name in enumerate(args.cases.split(",")):
            call = make_call(name, qkv, p)

            def fwd(call=call):
                with torch.no_grad():
                    call()

            def fwd_bwd(call=call):
                qkv.grad = None
                call().backward(do)

            cases.append(dict(name="%s#%d p=%g" % (name, i, p), fwd=fwd,
                              fwd_bwd=fwd_bwd, t_fwd=[], t_fb=[]))

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

    print("attn_causal_bench %s B=%d H=%d S=%d bf16, %d rounds x %d iters,"
          " us per call: median [min..max]"
          % (args.label, B, H, S, args.rounds, args.iters))
    out = {}
    for c in cases:
        f, fb = stats(c["t_fwd"]), stats(c["t_fb"])
        print("  %-16s fwd %8.1f [%8.1f..%8.1f]   "
              "fwd+bwd %8.1f [%8.1f..%8.1f]" % ((c["name"],) + f + fb),
              flush=True)
        out[c["name"]] = dict(fwd_us=round(f[0], 1),
                              fwd_bwd_us=round(fb[0], 1))
    print(json.dumps(dict(label=args.label, shape=[B, H, S], us=out)))


if __name__ == "__main__":
    main()
