"""Flash attention for 128-wide heads: time forward and forward+backward
at B=8, H=32, S=2048, D=128 (bf16) with device events, at dropout 0 and
0.1, and report the peak memory of one forward+backward call.

Cases (alternated round by round inside one process, after a warm-up):
  d128         flash_attention_packed on [B,S,3,H,128], dense
  d128c        the same, causal=True
  sdpa, sdpac  torch scaled_dot_product_attention (dense, is_causal) on
               the same packed buffer, including the permute/contiguous
               copies into [B,H,S,128] and back to [B,S,H*128] that a
               caller needs
  d64, d64c    the D=64 kernels at 2*H heads on the same bytes viewed as
               [B,S,3,2H,64]: the same FLOPs and the same bytes, a
               yardstick inside the project

A case may be listed more than once (the default repeats d128): the
repeats are timed as separate entries, which shows the run-to-run spread.
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
    """(leaf tensor that receives the gradient, call)"""
    B, S, _, H, D = qkv.shape
    causal = case.endswith("c")
    if case in ("d128", "d128c"):
        return qkv, lambda: F_.flash_attention_packed(qkv, p, causal=causal)
    if case in ("d64", "d64c"):
        q64 = qkv.detach().view(B, S, 3, 2 * H, 64).requires_grad_(True)
        return q64, lambda: F_.flash_attention_packed(q64, p, causal=causal)
    if case in ("sdpa", "sdpac"):
        def sdpa():
            q, k, v = (t.contiguous()
                       for t in qkv.permute(2, 0, 3, 1, 4).unbind(0))
            o = torch.nn.functional.scaled_dot_product_attention(
                q, k, v, dropout_p=p, is_causal=causal)
            return o.transpose(1, 2).reshape(B, S, H * D)
        return qkv, sdpa
    raise SystemExit("unknown case %r" % case)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="d128,d128c,sdpa,sdpac,d64,d64c,d128")
    ap.add_argument("--dropouts", default="0,0.1")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--seq", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: timings on a CPU mean nothing")

    B, H, S = args.batch, args.heads, args.seq
    torch.manual_seed(0)
    qkv = torch.randn(B, S, 3, H, 128, device="cuda").bfloat16() \
        .requires_grad_(True)
    do = torch.randn(B, S, H * 128, device="cuda").bfloat16()

    cases = []
    for p in (float(x) for x in args.dropouts.split(",")):
        for i, name in enumerate(args.cases.split(",")):
            leaf, call = make_call(name, qkv, p)

            def fwd(call=call):
                with torch.no_grad():
                    call()

            def fwd_bwd(call=call, leaf=leaf):
                leaf.grad = None
                call().backward(do)

            cases.append(dict(name="%s#%d p=%g" % (name, i, p), fwd=fwd,
                              fwd_bwd=fwd_bwd, leaf=leaf, t_fwd=[],
                              t_fb=[]))

    for c in cases:  # warm up every case
        for _ in range(3):
            c["fwd"]()
            c["fwd_bwd"]()
        c["leaf"].grad = None
    torch.cuda.synchronize()
    for c in cases:  # peak memory of one forward+backward call
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        c["fwd_bwd"]()
        torch.cuda.synchronize()
        c["peak_mib"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        c["leaf"].grad = None
    for _ in range(args.rounds):
        for c in cases:
            c["t_fwd"].append(timed(c["fwd"], args.iters))
            c["t_fb"].append(timed(c["fwd_bwd"], args.iters))
            c["leaf"].grad = None

    def stats(ts):
        ts = sorted(ts)
        return ts[len(ts) // 2], ts[0], ts[-1]

    print("attn_d128_bench %s B=%d H=%d S=%d D=128 bf16, %d rounds x %d "
          "iters, us per call: median [min..max]; peak MiB above the "
          "resident inputs in one fwd+bwd"
          % (args.label, B, H, S, args.rounds, args.iters))
    out = {}
    for c in cases:
        f, fb = stats(c["t_fwd"]), stats(c["t_fb"])
        print("  %-16s fwd %8.1f [%8.1f..%8.1f]   "
              "fwd+bwd %8.1f [%8.1f..%8.1f]   peak %7.1f MiB"
              % ((c["name"],) + f + fb + (c["peak_mib"],)), flush=True)
        out[c["name"]] = dict(fwd_us=round(f[0], 1),
                              fwd_bwd_us=round(fb[0], 1),
                              peak_mib=round(c["peak_mib"], 1))
    print(json.dumps(dict(label=args.label, shape=[B, H, S, 128], us=out)))


if __name__ == "__main__":
    main()
