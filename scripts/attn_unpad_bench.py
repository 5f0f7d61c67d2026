"""Unpadded (cu_seqlens) flash attention against the padded kernels on the
same sequences, and the BERT-base pretrain step packed against padded,
timed with device events.

  --what attn  forward and forward+backward of
               flash_attention_unpadded ([T,3,H,D], --impl unpadded) or
               flash_attention_packed(..., seq_lens=...) ([B,S,3,H,D],
               --impl padded), dense and causal, with and without
               dropout, at three length sets: `full` (all S), `half`
               (all S/2) and `mixed` (seeded uniform over [S/8, S]; at
               S=512 the sets of attn_varlen_bench.py).
  --what bert  the eager BERT-base pretrain step (batch 64, S=512, the
               step builder bench.py uses) on the `mixed` lengths, with
               unpad=True (--impl unpadded) or unpad=False (padded).

`--impl padded` uses only the interface that predates the unpadded
path, so this file also runs on an older checkout: that is how the
padded side of a comparison is taken on the parent commit. Alternate the
two in separate processes and compare medians.
"""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # noqa
import argparse
import json

import torch
from sparkdl.ops import functional as F_


def make_lens(case, B, S):
    if case == "full":
        return torch.full((B,), S)
    if case == "half":
        return torch.full((B,), S // 2)
    g = torch.Generator().manual_seed(11)
    return torch.randint(S // 8, S + 1, (B,), generator=g)


def timed(fn, iters):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1000  # us per call


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def attn_cases(args):
    B, H, D, S = args.batch, args.heads, args.width, args.seq
    torch.manual_seed(0)
    full = torch.randn(B, S, 3, H, D, device="cuda").bfloat16()
    full_do = torch.randn(B, S, H * D, device="cuda").bfloat16()
    cases = []
    for name in ("full", "half", "mixed"):
        lens = make_lens(name, B, S).to("cuda", torch.int32)
        if args.impl == "unpadded":
            qkv, cu, index, _ = F_.unpad_batch(full, lens)
            do = full_do.view(B * S, -1)[index].contiguous()
        else:
            qkv, do = full.clone(), full_do
        qkv.requires_grad_(True)
        for causal in (False, True):
            for p in (0.0, 0.1):
                if args.impl == "unpadded":
                    call = lambda qkv=qkv, cu=cu, causal=causal, p=p: \
                        F_.flash_attention_unpadded(qkv, cu, S, p, causal)
                else:
                    call = lambda qkv=qkv, lens=lens, causal=causal, p=p: \
                        F_.flash_attention_packed(qkv, p, seq_lens=lens,
                                                  causal=causal)

                def fwd(call=call):
                    with torch.no_grad():
                        call()

                def fwd_bwd(call=call, qkv=qkv, do=do):
                    qkv.grad = None
                    call().backward(do)

                cases.append(dict(
                    name="%s %s p=%.1f" % (
                        name, "causal" if causal else "dense ", p),
                    tokens=int(lens.sum()), run=(fwd, fwd_bwd), t=([], [])))
    return cases


def bert_cases(args):
    from sparkdl.models.bert import BertBase, bert_pretrain_step
    import sparkdl.ops as ops
    torch.manual_seed(1234)
    model = BertBase().cuda()
    ops.convert_bf16_training(model)
    opt = ops.FusedAdamW(model.parameters(), lr=1e-4, weight_decay=0.01)
    lens = make_lens("mixed", 64, 512)
    kw = dict(unpad=True) if args.impl == "unpadded" else {}
    step = bert_pretrain_step(model, opt, 64, 512, "cuda", True,
                              seq_lens=lens, **kw)
    return [dict(name="bert-base step", tokens=int(lens.sum()),
                 run=(step,), t=([],))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="attn", choices=["attn", "bert"])
    ap.add_argument("--impl", default="unpadded",
                    choices=["unpadded", "padded"])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: timings on a CPU mean nothing")

    cases = attn_cases(args) if args.what == "attn" else bert_cases(args)
    for c in cases:
        for _ in range(args.warmup):
            for fn in c["run"]:
                fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for c in cases:
            for fn, ts in zip(c["run"], c["t"]):
                ts.append(timed(fn, args.iters))

    shape = [args.batch, args.heads, args.width, args.seq] \
        if args.what == "attn" else [64, 12, 64, 512]
    print("attn_unpad_bench %s %s %s B,H,D,S=%s bf16, %d rounds x %d iters,"
          " us per call: median [min..max]"
          % (args.label, args.what, args.impl, shape, args.rounds,
             args.iters))
    out = {}
    for c in cases:
        st = [stats(ts) for ts in c["t"]]
        print("  %-22s tokens=%6d  " % (c["name"], c["tokens"]) + "   ".join(
            "%s %9.1f [%9.1f..%9.1f]" % ((k,) + s)
            for k, s in zip(("fwd", "fwd+bwd") if len(st) == 2
                            else ("step",), st)), flush=True)
        out[c["name"]] = [round(s[0], 1) for s in st]
    print(json.dumps(dict(label=args.label, what=args.what, impl=args.impl,
                          shape=shape, us=out)))


if __name__ == "__main__":
    main()
