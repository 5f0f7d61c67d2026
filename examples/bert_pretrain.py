"""BERT-base bf16 MLM pretraining on MI355X via HorovodRunner
(BASELINE.json config 4).

    python examples/bert_pretrain.py --np 8
    python examples/bert_pretrain.py --np 8 --varlen

--varlen trains on right-padded variable-length batches: per-sequence
lengths (seeded uniform over [64, seq]) go to the model as `seq_lens`,
the flash attention kernels skip the padded tiles, and MLM positions
are drawn among valid tokens only. With real data, pass the
tokenizer's `attention_mask` (or, sync-free, the lengths) to
`BertBase.forward_mlm`.
"""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # noqa
import argparse


def main(steps=50, batch=64, seq=512, varlen=False):
    import torch
    import sparkdl.torch as hvd
    import sparkdl.ops as ops
    from sparkdl.models.bert import BertBase, bert_pretrain_step
    from sparkdl.utils import StepTimer

    hvd.init()
    torch.manual_seed(1234)
    model = BertBase().cuda()
    ops.convert_bf16_training(model)   # bf16 weights, fp32 masters
    opt = hvd.DistributedOptimizer(
        ops.FusedAdamW(model.parameters(), lr=1e-4, weight_decay=0.01))
    hvd.broadcast_parameters(model, root_rank=0)

    seq_lens = None
    if varlen:
        g = torch.Generator().manual_seed(11 + hvd.rank())
        seq_lens = torch.randint(64, seq + 1, (batch,), generator=g)
    step = bert_pretrain_step(model, opt, batch, seq, "cuda", True,
                              seq_lens=seq_lens)
    timer = StepTimer()
    for _ in range(steps):
        with timer:
            step()
    if hvd.rank() == 0:
        s = timer.summary()
        print("p50 %.1f ms/step -> %.0f sequences/sec (whole job)"
              % (s["p50_ms"], batch * hvd.size() / (s["p50_ms"] / 1000)))
    return timer.summary()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--np", type=int, default=8)
    ap.add_argument("--varlen", action="store_true",
                    help="right-padded variable-length batches")
    args = ap.parse_args()
    from sparkdl import HorovodRunner
    print(HorovodRunner(np=args.np).run(main, varlen=args.varlen))
