"""BERT-base for the seq-512 bf16 pretrain benchmark (BASELINE.json
config 4), written from scratch.

MI355X mapping (round 2): every Linear — QKV, attention out, both FFN
halves, the MLM dense — runs on the hand-written 256x256 16-wave MFMA
GEMM with fused bias(+GELU) epilogues and in-house dgrad; attention is
the hand-written flash forward+backward (packed-qkv zero-copy I/O,
in-kernel dropout) — no Triton/aotriton and no library GEMM on the
fwd/dgrad path (wgrad remains hipBLASLt, see NOTES-round2.md);
LayerNorm and the optimizer (fused multi-tensor AdamW) are hand-written
CDNA4 kernels.

The two sublayer tails of every layer, ``ln(x + drop(sublayer(x)))``,
are eager dropout and add in front of the LayerNorm kernel by default.
``BertConfig(fused_dropout_ln=True)`` (or SPARKDL_FUSED_DROPOUT_LN=1)
runs each as one kernel forward and one backward
(``ops.dropout_add_layer_norm``) with no stored mask. It is opt-in
because its dropout mask is the kernels' counter hash, not torch's
Philox draw: the same seed then gives another training trajectory.
"""

import math
import os

import torch
import torch.nn as nn

from sparkdl.ops import LayerNorm, Linear, LinearGelu


class BertConfig:
    def __init__(self, vocab_size=30522, hidden=768, layers=12, heads=12,
                 ffn=3072, max_seq=512, type_vocab=2, dropout=0.1,
                 fused_dropout_ln=None):
        self.vocab_size = vocab_size
        self.hidden = hidden
        self.layers = layers
        self.heads = heads
        self.ffn = ffn
        self.max_seq = max_seq
        self.type_vocab = type_vocab
        self.dropout = dropout
        # None: SPARKDL_FUSED_DROPOUT_LN ("1" = on); off by default
        if fused_dropout_ln is None:
            fused_dropout_ln = os.environ.get(
                "SPARKDL_FUSED_DROPOUT_LN", "0") == "1"
        self.fused_dropout_ln = bool(fused_dropout_ln)


class BertEmbeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.word = nn.Embedding(cfg.vocab_size, cfg.hidden)
        self.position = nn.Embedding(cfg.max_seq, cfg.hidden)
        self.token_type = nn.Embedding(cfg.type_vocab, cfg.hidden)
        self.ln = LayerNorm(cfg.hidden, eps=1e-12)
        self.drop = nn.Dropout(cfg.dropout)

    def forward(self, ids, token_type=None):
        B, S = ids.shape
        pos = torch.arange(S, device=ids.device).unsqueeze(0)
        h = self.word(ids) + self.position(pos)
        if token_type is not None:
            h = h + self.token_type(token_type)
        return self.drop(self.ln(h))


class BertSelfAttention(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.heads = cfg.heads
        self.head_dim = cfg.hidden // cfg.heads
        self.qkv = Linear(cfg.hidden, 3 * cfg.hidden)
        self.out = Linear(cfg.hidden, cfg.hidden)
        self.drop_p = cfg.dropout

    def forward(self, x, seq_lens=None):
        """seq_lens: optional int32 [B] on x's device — valid length of
        each right-padded row. Padded keys are never attended to and
        the attention output at padded positions is exactly zero, on
        the flash path and on the fallback path alike."""
        from sparkdl.ops import functional as F_
        B, S, H = x.shape
        qkv = self.qkv(x).view(B, S, 3, self.heads, self.head_dim)
        p = self.drop_p if self.training else 0.0
        if (qkv.is_cuda and qkv.dtype == torch.bfloat16
                and self.head_dim == 64 and S % 64 == 0):
            # hand-written CDNA4 flash kernels (fwd+bwd, in-kernel
            # dropout), reading the packed qkv buffer with strided rows
            # and writing O as [B,S,H] directly — no Triton and no
            # permute/contiguous copies on the hot path; lengths are
            # read in-kernel (padded tiles skipped, no host sync)
            o = F_.flash_attention_packed(qkv, dropout_p=p,
                                          seq_lens=seq_lens)
        else:
            q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)  # [B,h,S,d]
            if seq_lens is None:
                o = nn.functional.scaled_dot_product_attention(
                    q, k, v, dropout_p=p)
            else:
                # same semantics as the kernels (zero padded rows)
                o = F_.masked_attention_ref(q, k, v, seq_lens,
                                            dropout_p=p)
            o = o.transpose(1, 2).reshape(B, S, H)
        return self.out(o)


class BertLayer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.attn = BertSelfAttention(cfg)
        self.ln1 = LayerNorm(cfg.hidden, eps=1e-12)
        self.ffn_in = LinearGelu(cfg.hidden, cfg.ffn)
        self.ffn_out = Linear(cfg.ffn, cfg.hidden)
        self.ln2 = LayerNorm(cfg.hidden, eps=1e-12)
        self.drop = nn.Dropout(cfg.dropout)
        self.fused_dropout_ln = getattr(cfg, "fused_dropout_ln", False)

    def _tail(self, ln, sub, x):
        """ln(x + drop(sub)) as one op, on ln's parameters."""
        from sparkdl.ops import functional as F_
        return F_.dropout_add_layer_norm(sub, x, ln.weight, ln.bias,
                                         self.drop.p, self.training, ln.eps)

    def forward(self, x, seq_lens=None):
        if self.fused_dropout_ln:
            x = self._tail(self.ln1, self.attn(x, seq_lens), x)
            return self._tail(self.ln2, self.ffn_out(self.ffn_in(x)), x)
        x = self.ln1(x + self.drop(self.attn(x, seq_lens)))
        x = self.ln2(x + self.drop(self.ffn_out(self.ffn_in(x))))
        return x


class BertBase(nn.Module):
    def __init__(self, cfg=None):
        super().__init__()
        self.cfg = cfg = cfg or BertConfig()
        self.embeddings = BertEmbeddings(cfg)
        self.encoder = nn.ModuleList(
            [BertLayer(cfg) for _ in range(cfg.layers)])
        # MLM head with tied decoder weights.
        self.mlm_dense = Linear(cfg.hidden, cfg.hidden)
        self.mlm_ln = LayerNorm(cfg.hidden, eps=1e-12)
        self.mlm_bias = nn.Parameter(torch.zeros(cfg.vocab_size))
        self.apply(self._init)

    def _init(self, m):
        if isinstance(m, (nn.Linear, Linear, LinearGelu)):
            nn.init.normal_(m.weight, std=0.02)
            if getattr(m, "bias", None) is not None:
                nn.init.zeros_(m.bias)
        elif isinstance(m, nn.Embedding):
            nn.init.normal_(m.weight, std=0.02)

    @staticmethod
    def _seq_lens(ids, attention_mask, seq_lens):
        """Resolve the padding arguments to int32 [B] lengths on ids'
        device (or None), once per forward."""
        if attention_mask is not None and seq_lens is not None:
            raise ValueError(
                "pass either attention_mask or seq_lens, not both")
        if attention_mask is not None:
            from sparkdl.ops.functional import seqlens_from_mask
            if attention_mask.shape != ids.shape:
                raise ValueError("attention_mask must match ids' [B, S]")
            seq_lens = seqlens_from_mask(attention_mask.to(ids.device))
        if seq_lens is None:
            return None
        return torch.as_tensor(seq_lens).to(
            device=ids.device, dtype=torch.int32).contiguous()

    def encode(self, ids, token_type=None, *, attention_mask=None,
               seq_lens=None):
        """Hidden states [B, S, hidden].

        Variable-length batches are right-padded: pass either
        ``attention_mask`` ([B,S], 1 = token, each row a prefix of
        ones; validated, which syncs once outside graph capture) or
        ``seq_lens`` (int [B]; the sync-free path). Padded keys are
        then never attended to, so hidden states at valid positions do
        not depend on the padding. Hidden states AT padded positions
        are unspecified but finite."""
        seq_lens = self._seq_lens(ids, attention_mask, seq_lens)
        h = self.embeddings(ids, token_type)
        # Keep the residual stream in the autocast compute dtype (bf16) so
        # every LayerNorm / bias+GELU hits the CDNA4 kernels; embeddings
        # and type-promoted residual adds would otherwise pin it to fp32.
        if h.is_cuda and torch.is_autocast_enabled():
            h = h.to(torch.get_autocast_dtype("cuda"))
        for layer in self.encoder:
            h = layer(h, seq_lens)
        return h

    def _mlm_logits(self, h):
        h = self.mlm_ln(torch.nn.functional.gelu(self.mlm_dense(h)))
        logits = torch.nn.functional.linear(
            h, self.embeddings.word.weight.to(h.dtype), None)
        return logits + self.mlm_bias.to(logits.dtype)

    def forward(self, ids, token_type=None, *, attention_mask=None,
                seq_lens=None):
        """MLM logits [B, S, vocab]; padding arguments as in encode()
        (logits at padded positions are unspecified but finite)."""
        return self._mlm_logits(self.encode(
            ids, token_type, attention_mask=attention_mask,
            seq_lens=seq_lens))

    def forward_mlm(self, ids, positions, token_type=None, *,
                    attention_mask=None, seq_lens=None):
        """MLM logits only at the masked positions (flat indices into the
        [B*S] token stream) — the vocab projection runs on ~15% of tokens
        instead of all of them, the standard pretrain-head optimization.
        Padding arguments as in encode()."""
        h = self.encode(ids, token_type, attention_mask=attention_mask,
                        seq_lens=seq_lens)
        h = h.reshape(-1, self.cfg.hidden).index_select(0, positions)
        return self._mlm_logits(h)


def bert_pretrain_step(model, opt, batch, seq, device, use_cuda,
                       mask_frac=0.15, seq_lens=None):
    """Build a closure running one synthetic MLM pretrain step.

    The vocab projection + loss run only on the masked positions
    (mask_frac of tokens), as in real MLM pretraining.

    seq_lens (optional, int [batch]): treat the batch as right-padded
    to ``seq`` with these valid lengths — MLM positions are drawn only
    among valid tokens and the lengths go to the model (device-side,
    no per-step host sync).
    """
    cfg = model.cfg
    g = torch.Generator(device="cpu").manual_seed(7)
    ids = torch.randint(0, cfg.vocab_size, (batch, seq), generator=g) \
        .to(device)
    mask = torch.rand(batch, seq, generator=g) < mask_frac
    lens_dev = None
    if seq_lens is not None:
        lens = torch.as_tensor(seq_lens).to("cpu", torch.int64) \
            .clamp(0, seq)
        if lens.shape != (batch,):
            raise ValueError("seq_lens must hold one length per row")
        mask &= torch.arange(seq).unsqueeze(0) < lens.unsqueeze(1)
        lens_dev = lens.to(device=device, dtype=torch.int32)
    positions = mask.flatten().nonzero(as_tuple=False).flatten().to(device)
    labels = ids.flatten().index_select(0, positions)
    autocast_dev = "cuda" if use_cuda else "cpu"
    # Pure-bf16 weights (convert_bf16_training) need no autocast: every
    # GEMM already sees bf16 operands and grads flow in bf16.
    pure_bf16 = model.embeddings.word.weight.dtype == torch.bfloat16

    def step():
        opt.zero_grad()
        if pure_bf16:
            logits = model.forward_mlm(ids, positions,
                                       seq_lens=lens_dev)
            loss = torch.nn.functional.cross_entropy(
                logits.float(), labels)
        else:
            with torch.autocast(autocast_dev, dtype=torch.bfloat16):
                logits = model.forward_mlm(ids, positions,
                                           seq_lens=lens_dev)
                loss = torch.nn.functional.cross_entropy(
                    logits.float(), labels)
        loss.backward()
        opt.step()
        return loss

    return step
