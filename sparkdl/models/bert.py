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

The MLM loss is ``F.linear`` on the tied embedding, an eager bias add,
a cast to fp32 and ``F.cross_entropy`` by default.
``BertConfig(fused_mlm_loss=True)`` (or SPARKDL_FUSED_MLM_LOSS=1) makes
``bert_pretrain_step`` call ``BertBase.mlm_loss``, which runs
``ops.linear_cross_entropy``: the logits never reach memory. It is
opt-in because the fused loss is computed from fp32 logits where the
default path rounds them to bf16 first, so the same seed gives a
slightly different trajectory.

``BertConfig(causal=True)`` makes every self-attention causal (position
q attends to positions <= q; the flash kernels' triangular schedule on
the GPU). ``forward_mlm(ids, positions)`` with ``positions`` = every
token but the last of each row, and the ids shifted by one as labels,
is then a next-token language model on the same loss code.

Heads of width 64 and 128 (``hidden // heads``) have flash kernels. At
width 128 a call without ``seq_lens`` takes them when
SPARKDL_FLASH_D128 is "1" (see ``_FLASH_D128_DEFAULT`` and
profiles/README.md, "Flash attention, 128-wide heads"); a call with
``seq_lens`` always does: its only alternative is the composed
reference, which materialises the [B,h,S,S] fp32 scores.

``BertConfig(kv_heads=k)`` with k < heads is grouped-query attention:
the ``heads`` query heads share k key/value heads in groups of
``heads // k`` and ``qkv`` projects to ``hidden + 2*k*head_dim``
features, laid out [Q heads | K heads | V heads]. On the padded path,
at width 128 in bf16 on the GPU with ``S % 64 == 0``, attention is
``ops.flash_attention_gqa_packed`` (K/V heads read in place, dK/dV
summed per group in the kernel): always with ``seq_lens``, and without
them when SPARKDL_FLASH_GQA is "1" (see ``_FLASH_GQA_DEFAULT``).
Everywhere else, the unpadded path included, K and V are expanded to
``heads`` heads in front of what the multi-head model calls.
``kv_heads=None`` or ``== heads`` is the multi-head model, unchanged.

Unpadded batches: ``encode``, ``forward``, ``forward_mlm`` and
``mlm_loss`` take ``cu_seqlens`` (int32 ``[B+1]``, with ``max_seqlen``
defaulting to ``cfg.max_seq``). ``ids`` and ``token_type`` are then
one-dimensional ``[T]``, the sequences back to back, the hidden states
are ``[T, hidden]`` and ``positions`` index that flat axis: every GEMM,
LayerNorm and bias+GELU runs on the real tokens only, and attention is
``ops.flash_attention_unpadded`` (bf16 on the GPU, heads of width 64 or
128; elsewhere the composed ``ops.unpadded_attention_ref``).
``bert_pretrain_step(..., seq_lens=..., unpad=True)`` packs its batch
once and trains this way.
"""

import math
import os

import torch
import torch.nn as nn

from sparkdl.ops import LayerNorm, Linear, LinearGelu


class BertConfig:
    def __init__(self, vocab_size=30522, hidden=768, layers=12, heads=12,
                 ffn=3072, max_seq=512, type_vocab=2, dropout=0.1,
                 fused_dropout_ln=None, fused_mlm_loss=None, causal=False,
                 kv_heads=None):
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
        # None: SPARKDL_FUSED_MLM_LOSS ("1" = on); off by default
        if fused_mlm_loss is None:
            fused_mlm_loss = os.environ.get(
                "SPARKDL_FUSED_MLM_LOSS", "0") == "1"
        self.fused_mlm_loss = bool(fused_mlm_loss)
        # left-to-right (decoder-style) self-attention
        self.causal = bool(causal)
        # grouped-query attention: `heads` query heads share `kv_heads`
        # key/value heads (None or == heads: plain multi-head attention)
        if kv_heads is None:
            kv_heads = heads
        if kv_heads < 1 or heads % kv_heads:
            raise ValueError("kv_heads=%r must divide heads=%r"
                             % (kv_heads, heads))
        self.kv_heads = int(kv_heads)


class BertEmbeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.word = nn.Embedding(cfg.vocab_size, cfg.hidden)
        self.position = nn.Embedding(cfg.max_seq, cfg.hidden)
        self.token_type = nn.Embedding(cfg.type_vocab, cfg.hidden)
        self.ln = LayerNorm(cfg.hidden, eps=1e-12)
        self.drop = nn.Dropout(cfg.dropout)

    def forward(self, ids, token_type=None, cu_seqlens=None):
        if cu_seqlens is not None:
            # ids [T]: a token's position is its offset inside its
            # sequence, found on the device (no sync). Spare tokens
            # count on from cu[B]; clamped into the table.
            tok = torch.arange(ids.shape[0], device=ids.device)
            cu = cu_seqlens.long()
            seq = torch.searchsorted(cu[1:].contiguous(), tok, right=True)
            pos = (tok - cu[seq]).clamp(0, self.position.num_embeddings - 1)
        else:
            B, S = ids.shape
            pos = torch.arange(S, device=ids.device).unsqueeze(0)
        h = self.word(ids) + self.position(pos)
        if token_type is not None:
            h = h + self.token_type(token_type)
        return self.drop(self.ln(h))


# Value of SPARKDL_FLASH_D128 when it is unset: whether 128-wide heads
# take the flash kernels without seq_lens (decided by the measurement in
# profiles/attn_d128.log against scaled_dot_product_attention).
_FLASH_D128_DEFAULT = "0"

# Value of SPARKDL_FLASH_GQA when it is unset: whether a kv_heads model
# takes the grouped-query kernels without seq_lens (decided by the
# measurement in profiles/attn_gqa.log against K/V expanded to every
# query head in front of the 128-wide kernels and of
# scaled_dot_product_attention). With seq_lens it always does.
_FLASH_GQA_DEFAULT = "0"


class BertSelfAttention(nn.Module):
    # False sends every call through the library / composed branch
    use_flash = True

    def __init__(self, cfg):
        super().__init__()
        self.heads = cfg.heads
        self.head_dim = cfg.hidden // cfg.heads
        self.kv_heads = getattr(cfg, "kv_heads", cfg.heads)
        if self.kv_heads == self.heads:
            self.qkv = Linear(cfg.hidden, 3 * cfg.hidden)
        else:  # one projection to [Q heads | K heads | V heads]
            self.qkv = Linear(cfg.hidden, cfg.hidden
                              + 2 * self.kv_heads * self.head_dim)
        self.out = Linear(cfg.hidden, cfg.hidden)
        self.drop_p = cfg.dropout
        self.causal = getattr(cfg, "causal", False)

    def _expanded(self, qkv):
        """Grouped-query projection output [..., heads + 2*kv_heads, d]
        -> q, k, v [..., heads, d], K/V heads repeated over their group
        (what every composed branch and the unpadded kernels take)."""
        h, hkv = self.heads, self.kv_heads
        q, k, v = qkv.split([h, hkv, hkv], dim=-2)
        return (q, k.repeat_interleave(h // hkv, dim=-2),
                v.repeat_interleave(h // hkv, dim=-2))

    def _forward_gqa(self, x, seq_lens):
        """The padded path with kv_heads < heads."""
        from sparkdl.ops import functional as F_
        B, S, H = x.shape
        qkv = self.qkv(x).view(B, S, self.heads + 2 * self.kv_heads,
                               self.head_dim)
        p = self.drop_p if self.training else 0.0
        take = seq_lens is not None or os.environ.get(
            "SPARKDL_FLASH_GQA", _FLASH_GQA_DEFAULT) == "1"
        if self.use_flash and take and F_.flash_attention_gqa_ok(qkv):
            # K/V heads read in place, dK/dV summed per group in-kernel
            o = F_.flash_attention_gqa_packed(
                qkv, self.kv_heads, dropout_p=p, seq_lens=seq_lens,
                causal=self.causal)
        else:
            q, k, v = (t.transpose(1, 2) for t in self._expanded(qkv))
            if seq_lens is None:
                o = nn.functional.scaled_dot_product_attention(
                    q, k, v, dropout_p=p, is_causal=self.causal)
            else:
                o = F_.masked_attention_ref(q, k, v, seq_lens, dropout_p=p,
                                            causal=self.causal)
            o = o.transpose(1, 2).reshape(B, S, H)
        return self.out(o)

    def _forward_unpadded(self, x, cu_seqlens, max_seqlen):
        """x [T, hidden], the sequences back to back (cu_seqlens int32
        [B+1]); the attention output at spare tokens is exactly zero."""
        from sparkdl.ops import functional as F_
        if self.kv_heads != self.heads:
            # no grouped-query variant of the unpadded kernels: expand
            qkv = torch.stack(self._expanded(self.qkv(x).view(
                x.shape[0], -1, self.head_dim)), dim=1)
        else:
            qkv = self.qkv(x).view(x.shape[0], 3, self.heads,
                                   self.head_dim)
        p = self.drop_p if self.training else 0.0
        if self.use_flash and F_.flash_attention_unpadded_ok(qkv):
            # no S % 64 condition and no opt-in at width 128: the only
            # alternative is the composed reference
            o = F_.flash_attention_unpadded(qkv, cu_seqlens, max_seqlen,
                                            dropout_p=p, causal=self.causal)
        else:
            o = F_.unpadded_attention_ref(qkv, cu_seqlens, dropout_p=p,
                                          causal=self.causal)
        return self.out(o)

    def forward(self, x, seq_lens=None, cu_seqlens=None, max_seqlen=None):
        """seq_lens: optional int32 [B] on x's device — valid length of
        each right-padded row. Padded keys are never attended to and
        the attention output at padded positions is exactly zero, on
        the flash path and on the fallback path alike."""
        from sparkdl.ops import functional as F_
        if cu_seqlens is not None:
            return self._forward_unpadded(x, cu_seqlens, max_seqlen)
        if self.kv_heads != self.heads:
            return self._forward_gqa(x, seq_lens)
        B, S, H = x.shape
        qkv = self.qkv(x).view(B, S, 3, self.heads, self.head_dim)
        p = self.drop_p if self.training else 0.0
        wide_ok = seq_lens is not None or os.environ.get(
            "SPARKDL_FLASH_D128", _FLASH_D128_DEFAULT) == "1"
        if (self.use_flash and qkv.is_cuda and qkv.dtype == torch.bfloat16
                and (self.head_dim == 64
                     or (self.head_dim == 128 and wide_ok))
                and S % 64 == 0):
            # hand-written CDNA4 flash kernels (fwd+bwd, in-kernel
            # dropout), reading the packed qkv buffer with strided rows
            # and writing O as [B,S,H] directly — no Triton and no
            # permute/contiguous copies on the hot path; lengths are
            # read in-kernel (padded tiles skipped, no host sync)
            o = F_.flash_attention_packed(qkv, dropout_p=p,
                                          seq_lens=seq_lens,
                                          causal=self.causal)
        else:
            q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)  # [B,h,S,d]
            if seq_lens is None:
                o = nn.functional.scaled_dot_product_attention(
                    q, k, v, dropout_p=p, is_causal=self.causal)
            else:
                # same semantics as the kernels (zero padded rows)
                o = F_.masked_attention_ref(q, k, v, seq_lens,
                                            dropout_p=p,
                                            causal=self.causal)
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

    def forward(self, x, seq_lens=None, cu_seqlens=None, max_seqlen=None):
        if cu_seqlens is not None:  # x [T, hidden]
            a = self.attn(x, cu_seqlens=cu_seqlens, max_seqlen=max_seqlen)
        else:
            a = self.attn(x, seq_lens)
        if self.fused_dropout_ln:
            x = self._tail(self.ln1, a, x)
            return self._tail(self.ln2, self.ffn_out(self.ffn_in(x)), x)
        x = self.ln1(x + self.drop(a))
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

    def _cu_seqlens(self, ids, attention_mask, seq_lens, cu_seqlens,
                    max_seqlen):
        """Check the unpadded arguments; -> (int32 cu_seqlens on ids'
        device, max_seqlen)."""
        if attention_mask is not None or seq_lens is not None:
            raise ValueError("cu_seqlens describes an unpadded batch: pass "
                             "no attention_mask or seq_lens with it")
        if ids.dim() != 1:
            raise ValueError("with cu_seqlens, ids is one-dimensional [T]")
        cu = torch.as_tensor(cu_seqlens).to(
            device=ids.device, dtype=torch.int32).contiguous()
        return cu, int(self.cfg.max_seq if max_seqlen is None
                       else max_seqlen)

    def encode(self, ids, token_type=None, *, attention_mask=None,
               seq_lens=None, cu_seqlens=None, max_seqlen=None):
        """Hidden states [B, S, hidden].

        Unpadded batches: ``ids`` (and ``token_type``) ``[T]`` with the
        sequences back to back and ``cu_seqlens`` int ``[B+1]`` give
        hidden states ``[T, hidden]``; tokens from ``cu[B]`` on are
        spare capacity with unspecified but finite hidden states.

        Variable-length batches are right-padded: pass either
        ``attention_mask`` ([B,S], 1 = token, each row a prefix of
        ones; validated, which syncs once outside graph capture) or
        ``seq_lens`` (int [B]; the sync-free path). Padded keys are
        then never attended to, so hidden states at valid positions do
        not depend on the padding. Hidden states AT padded positions
        are unspecified but finite."""
        if cu_seqlens is not None:
            cu_seqlens, max_seqlen = self._cu_seqlens(
                ids, attention_mask, seq_lens, cu_seqlens, max_seqlen)
            seq_lens = None
        else:
            seq_lens = self._seq_lens(ids, attention_mask, seq_lens)
        h = self.embeddings(ids, token_type, cu_seqlens)
        # Keep the residual stream in the autocast compute dtype (bf16) so
        # every LayerNorm / bias+GELU hits the CDNA4 kernels; embeddings
        # and type-promoted residual adds would otherwise pin it to fp32.
        if h.is_cuda and torch.is_autocast_enabled():
            h = h.to(torch.get_autocast_dtype("cuda"))
        for layer in self.encoder:
            h = layer(h, seq_lens, cu_seqlens, max_seqlen)
        return h

    def _mlm_logits(self, h):
        h = self.mlm_ln(torch.nn.functional.gelu(self.mlm_dense(h)))
        logits = torch.nn.functional.linear(
            h, self.embeddings.word.weight.to(h.dtype), None)
        return logits + self.mlm_bias.to(logits.dtype)

    def forward(self, ids, token_type=None, *, attention_mask=None,
                seq_lens=None, cu_seqlens=None, max_seqlen=None):
        """MLM logits [B, S, vocab] ([T, vocab] with cu_seqlens); padding
        arguments as in encode() (logits at padded positions are
        unspecified but finite)."""
        return self._mlm_logits(self.encode(
            ids, token_type, attention_mask=attention_mask,
            seq_lens=seq_lens, cu_seqlens=cu_seqlens,
            max_seqlen=max_seqlen))

    def forward_mlm(self, ids, positions, token_type=None, *,
                    attention_mask=None, seq_lens=None, cu_seqlens=None,
                    max_seqlen=None):
        """MLM logits only at the masked positions (flat indices into the
        [B*S] token stream) — the vocab projection runs on ~15% of tokens
        instead of all of them, the standard pretrain-head optimization.
        Padding arguments as in encode(); with cu_seqlens the positions
        index the flat [T] axis."""
        h = self.encode(ids, token_type, attention_mask=attention_mask,
                        seq_lens=seq_lens, cu_seqlens=cu_seqlens,
                        max_seqlen=max_seqlen)
        h = h.reshape(-1, self.cfg.hidden).index_select(0, positions)
        return self._mlm_logits(h)

    def mlm_loss(self, ids, positions, labels, token_type=None, *,
                 attention_mask=None, seq_lens=None, cu_seqlens=None,
                 max_seqlen=None, ignore_index=-100, reduction="mean"):
        """The MLM loss at the masked positions (as forward_mlm; labels
        int64 [len(positions)]) through ops.linear_cross_entropy on the
        tied embedding weight and mlm_bias: on bf16 GPU tensors the
        vocabulary projection and the cross-entropy are one kernel chain
        and no logits are stored; elsewhere exactly
        ``cross_entropy(forward_mlm(...).float(), labels)``."""
        from sparkdl.ops import functional as F_
        h = self.encode(ids, token_type, attention_mask=attention_mask,
                        seq_lens=seq_lens, cu_seqlens=cu_seqlens,
                        max_seqlen=max_seqlen)
        h = h.reshape(-1, self.cfg.hidden).index_select(0, positions)
        h = self.mlm_ln(torch.nn.functional.gelu(self.mlm_dense(h)))
        return F_.linear_cross_entropy(
            h, self.embeddings.word.weight.to(h.dtype), self.mlm_bias,
            labels, ignore_index=ignore_index, reduction=reduction)


def bert_pretrain_step(model, opt, batch, seq, device, use_cuda,
                       mask_frac=0.15, seq_lens=None, unpad=False):
    """Build a closure running one synthetic MLM pretrain step.

    The vocab projection + loss run only on the masked positions
    (mask_frac of tokens), as in real MLM pretraining.

    seq_lens (optional, int [batch]): treat the batch as right-padded
    to ``seq`` with these valid lengths — MLM positions are drawn only
    among valid tokens and the lengths go to the model (device-side,
    no per-step host sync).

    unpad=True (with seq_lens): pack ids, MLM positions and labels once
    here, at set-up, and run the model on the unpadded ``[T]`` token
    stream with ``cu_seqlens`` and no spare capacity: the same tokens,
    positions and labels as unpad=False, without the padding's work.
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
    kw = {"seq_lens": lens_dev}
    if unpad:
        if seq_lens is None:
            raise ValueError("unpad=True needs seq_lens")
        from sparkdl.ops.functional import unpad_batch
        ids, cu, index, _ = unpad_batch(ids, lens_dev)
        # flat [B*S] position -> its place in the packed stream
        where = torch.zeros(batch * seq, dtype=torch.long, device=device)
        where[index] = torch.arange(index.numel(), device=device)
        positions = where.index_select(0, positions)
        kw = {"cu_seqlens": cu, "max_seqlen": seq}
    autocast_dev = "cuda" if use_cuda else "cpu"
    # Pure-bf16 weights (convert_bf16_training) need no autocast: every
    # GEMM already sees bf16 operands and grads flow in bf16.
    pure_bf16 = model.embeddings.word.weight.dtype == torch.bfloat16

    fused_mlm_loss = getattr(cfg, "fused_mlm_loss", False)

    def step():
        opt.zero_grad()
        if fused_mlm_loss:
            with torch.autocast(autocast_dev, dtype=torch.bfloat16,
                                enabled=not pure_bf16):
                loss = model.mlm_loss(ids, positions, labels, **kw)
        elif pure_bf16:
            logits = model.forward_mlm(ids, positions, **kw)
            loss = torch.nn.functional.cross_entropy(
                logits.float(), labels)
        else:
            with torch.autocast(autocast_dev, dtype=torch.bfloat16):
                logits = model.forward_mlm(ids, positions, **kw)
                loss = torch.nn.functional.cross_entropy(
                    logits.float(), labels)
        loss.backward()
        opt.step()
        return loss

    return step
