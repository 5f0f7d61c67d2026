"""Grouped-query flash attention: time forward and forward+backward at
B=8, Hq=32, S=2048, D=128 (bf16) for Hkv in {32, 8, 1}, dense and causal,
with device events, and report the peak memory of one forward+backward
call. The input is the packed [B,S,Hq+2Hkv,128] output of one fused
projection; its gradient is the result.

Paths (alternated round by round inside one process, after every case
of every shape has been warmed up):
  gqa    flash_attention_gqa_packed: K/V heads read in place, dK/dV
         summed per group in the kernel
  d128   what a caller had before: repeat_interleave K and V to Hq heads
         into [B,S,3,Hq,128], flash_attention_packed on that, autograd
         summing the per-head bf16 dK/dV back to Hkv heads
  sdpa   the same expansion in front of torch
         scaled_dot_product_attention, with the permute/contiguous
         copies into [B,Hq,S,128] and back that it needs

The expansion and the group sum are timed as part of d128 and sdpa. The
[min..max] over the rounds is the run-to-run spread.

Cases marked "+lens" pass seq_lens (fixed lengths, uniform over
[S/4, S]) to gqa and d128, which then run their VARLEN kernels; sdpa
takes no lengths and is left out of them.
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


def make_call(path, qkv, hq, hkv, causal, lens=None):
    B, S = qkv.shape[:2]
    if path == "gqa":
        return lambda: F_.flash_attention_gqa_packed(
            qkv, hkv, 0.0, seq_lens=lens, causal=causal)

    def expanded():  # q, k, v as [B,S,Hq,128]
        q, k, v = qkv.split([hq, hkv, hkv], dim=2)
        return (q, k.repeat_interleave(hq // hkv, 2),
                v.repeat_interleave(hq // hkv, 2))

    if path == "d128":
        return lambda: F_.flash_attention_packed(
            torch.stack(expanded(), 2), 0.0, seq_lens=lens, causal=causal)
    if path == "sdpa":
        def sdpa():
            q, k, v = (t.transpose(1, 2).contiguous() for t in expanded())
            o = torch.nn.functional.scaled_dot_product_attention(
                q, k, v, is_causal=causal)
            return o.transpose(1, 2).reshape(B, S, hq * 128)
        return sdpa
    raise SystemExit("unknown path %r" % path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", default="gqa,d128,sdpa")
    ap.add_argument("--kv-heads", default="32,8,1")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--seq", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: timings on a CPU mean nothing")

    B, Hq, S = args.batch, args.heads, args.seq
    torch.manual_seed(0)
    do = torch.randn(B, S, Hq * 128, device="cuda").bfloat16()
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(S // 4, S + 1, (B,), generator=g) \
        .to("cuda", torch.int32)
    cases = []
    for hkv in (int(x) for x in args.kv_heads.split(",")):
        qkv = torch.randn(B, S, Hq + 2 * hkv, 128, device="cuda") \
            .bfloat16().requires_grad_(True)
        for causal, lt in ((False, None), (True, None), (False, lens),
                           (True, lens)):
            for path in args.paths.split(","):
                if lt is not None and path == "sdpa":
                    continue
                call = make_call(path, qkv, Hq, hkv, causal, lt)

                def fwd(call=call):
                    with torch.no_grad():
                        call()

                def fwd_bwd(call=call, leaf=qkv):
                    leaf.grad = None
                    call().backward(do)

                cases.append(dict(
                    name="Hkv=%-2d %-11s %s" % (
                        hkv, ("causal" if causal else "dense")
                        + ("+lens" if lt is not None else ""), path),
                    fwd=fwd, fwd_bwd=fwd_bwd, leaf=qkv, t_fwd=[], t_fb=[]))

    for c in cases:  # warm up every case of every shape
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

    print("attn_gqa_bench %s B=%d Hq=%d S=%d D=128 bf16, %d rounds x %d "
          "iters, us per call: median [min..max]; peak MiB above the "
          "resident inputs in one fwd+bwd"
          % (args.label, B, Hq, S, args.rounds, args.iters))
    print("lengths of the +lens cases:", lens.tolist())
    out = {}
    for c in cases:
        f, fb = stats(c["t_fwd"]), stats(c["t_fb"])
        print("  %-27s fwd %8.1f [%8.1f..%8.1f]   "
              "fwd+bwd %8.1f [%8.1f..%8.1f]   peak %7.1f MiB"
              % ((c["name"],) + f + fb + (c["peak_mib"],)), flush=True)
        out[" ".join(c["name"].split())] = dict(
            fwd_us=round(f[0], 1), fwd_bwd_us=round(fb[0], 1),
            peak_mib=round(c["peak_mib"], 1))
    print(json.dumps(dict(label=args.label, shape=[B, Hq, S, 128], us=out)))


if __name__ == "__main__":
    main()
