"""Autograd functions over the sparkdl._C HIP kernels, plus the plain
PyTorch fp32 reference implementations the GPU numerics tests compare
against ("HIP-kernel unit tests vs PyTorch-ROCm reference
outputs")."""

import os

import torch

import sparkdl.ops as _ops


# ---------------------------------------------------------------------------
# Reference implementations (fp32, plain PyTorch) — used on CPU and as the
# numerics oracle for the HIP kernels.
# ---------------------------------------------------------------------------

def layer_norm_ref(x, gamma, beta, eps=1e-5):
    xf = x.float()
    out = torch.nn.functional.layer_norm(
        xf, (x.shape[-1],), gamma.float(), beta.float(), eps)
    return out.to(x.dtype)


def bias_gelu_ref(x, bias):
    return torch.nn.functional.gelu(
        x.float() + bias.float(), approximate="none").to(x.dtype)


def masked_attention_ref(q, k, v, seq_lens, dropout_p=0.0):
    """Attention over a right-padded batch: row ``n`` of the leading
    dim holds ``seq_lens[n]`` valid tokens at positions ``[0, len)``.

    q/k/v: ``[N, ..., S, d]`` (``[BH,S,d]`` or ``[B,h,S,d]``); seq_lens:
    integer ``[N]`` (clamped into ``[0, S]``). For ``q < len``:
    ``O[q] = softmax_{k < len}(q.k / sqrt(d)) @ V[:len]``. Query rows
    ``>= len`` give exactly zero and act as constants for autograd: no
    dQ, no contribution to dK/dV, and dK/dV rows ``>= len`` are zero.
    ``len == 0`` gives all-zero output and gradients without NaN.

    Scores are masked with the finite fp32 minimum, not ``-inf``: an
    all-``-inf`` row (length 0) would make the softmax NaN, and that
    NaN survives into the backward even when the forward is zeroed. P
    is then zeroed by selection wherever the key or the query is
    padding."""
    S, d = q.shape[-2], q.shape[-1]
    qf, kf, vf = q.float(), k.float(), v.float()
    lens = torch.as_tensor(seq_lens, device=q.device).clamp(0, S)
    lens = lens.reshape((-1,) + (1,) * (q.dim() - 2))
    valid = torch.arange(S, device=q.device) < lens    # [N, ..., S]
    kmask = valid.unsqueeze(-2)
    qmask = valid.unsqueeze(-1)
    # fp32 throughout, also when called under autocast (the fill value
    # does not fit a 16-bit score matrix)
    with torch.autocast(q.device.type, enabled=False):
        s = qf @ kf.transpose(-1, -2) / d ** 0.5
        s = s.masked_fill(~kmask, torch.finfo(torch.float32).min)
        p = torch.softmax(s, dim=-1)
        p = torch.where(kmask & qmask, p, p.new_zeros(()))
        if dropout_p > 0:
            p = torch.nn.functional.dropout(p, dropout_p)
        o = p @ vf
    return o.to(q.dtype)


def seqlens_from_mask(attention_mask, validate=None):
    """``[B, S]`` bool/integer key-padding mask (nonzero = token) ->
    int32 ``[B]`` lengths on the mask's device, by a device-side sum.

    The attention kernels take right-padded batches only, so with
    ``validate=True`` every row must be a prefix of ones (no holes, no
    left padding), else ``ValueError``. That check reads one flag back
    to the host. The default validates except while the current stream
    is being captured into a graph, where a host sync is illegal.
    Passing ``seq_lens`` directly to the attention / model entry points
    is the path with no sync at all."""
    m = attention_mask
    if m.dim() != 2:
        raise ValueError("attention_mask must be [B, S], got %s"
                         % (tuple(m.shape),))
    mb = m != 0
    lens = mb.sum(-1, dtype=torch.int32)
    if validate is None:
        validate = not (m.is_cuda
                        and torch.cuda.is_current_stream_capturing())
    if validate:
        prefix = torch.arange(m.shape[1], device=m.device) \
            < lens.unsqueeze(-1)
        if not bool((mb == prefix).all()):
            raise ValueError(
                "attention_mask must be right-padded: every row a run "
                "of ones followed by zeros (no holes, no left padding)")
    return lens


# ---------------------------------------------------------------------------
# Autograd bindings
# ---------------------------------------------------------------------------

class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        C = _ops.ext()
        x = x.contiguous()
        y, mean, rstd = C.layernorm_fwd(x, gamma, beta, eps)
        ctx.save_for_backward(x, gamma, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        C = _ops.ext()
        x, gamma, mean, rstd = ctx.saved_tensors
        dx, dgamma, dbeta = C.layernorm_bwd(
            x, dy.contiguous(), gamma, mean, rstd)
        return dx, dgamma, dbeta, None


class _BiasGeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias):
        C = _ops.ext()
        x = x.contiguous()
        ctx.save_for_backward(x, bias)
        return C.bias_gelu_fwd(x, bias)

    @staticmethod
    def backward(ctx, dy):
        C = _ops.ext()
        x, bias = ctx.saved_tensors
        dx, dbias = C.bias_gelu_bwd(x, bias, dy.contiguous())
        return dx, dbias


def _to_nhwc(t):
    """[N,C,H,W] channels_last tensor -> [N,H,W,C] contiguous view."""
    return t.permute(0, 2, 3, 1).contiguous(memory_format=torch.contiguous_format)


def _from_nhwc(t):
    """[N,H,W,C] contiguous -> [N,C,H,W] tensor in channels_last layout."""
    return t.permute(0, 3, 1, 2)


def _alias(t):
    """A tensor over t's memory, shape and strides that is no view of
    t to autograd."""
    return torch.empty(0, dtype=t.dtype, device=t.device).set_(
        t.untyped_storage(), t.storage_offset(), t.size(), t.stride())


class _BNReLUFn(torch.autograd.Function):
    """With ``fork`` the node has two outputs, one tensor under two
    handles for two consumers, and so receives their gradients apart:
    the two-gradient kernels add them inside the reduction instead of
    autograd adding them in a pass of its own, and the masked sum they
    write is also the residual's gradient.

    ``slab`` (training only): the partial sums of x that its producer
    already wrote (``_Conv1x1StatsFn``); the statistics pass over x is
    then skipped. It gets no gradient."""

    @staticmethod
    def forward(ctx, x, residual, gamma, beta, running_mean, running_var,
                momentum, eps, training, relu, fork=False, slab=None):
        C = _ops.ext()
        xp = _to_nhwc(x)
        rp = _to_nhwc(residual) if residual is not None else None
        if slab is not None and training:
            y, mean, rstd, mask = C.bn_fwd_slab(
                xp, rp, slab, gamma, beta, running_mean, running_var,
                momentum, eps, relu)
        else:
            y, mean, rstd, mask = C.bn_fwd(
                xp, rp, gamma, beta, running_mean, running_var, momentum,
                eps, training, relu)
        # mask (1 bit/elem) replaces y in backward — y itself need not
        # be kept alive by autograd
        ctx.save_for_backward(xp, mask, gamma, mean, rstd)
        ctx.bn_flags = (training, relu, residual is not None)
        out = _from_nhwc(y)
        if not fork:
            return out
        # an output a consumer leaves unused arrives as None
        ctx.set_materialize_grads(False)
        # two handles on y's memory, each a tensor of its own: an
        # autograd view of one output would hand its gradient to that
        # output instead of to this node
        return _alias(out), _alias(out)

    @staticmethod
    def backward(ctx, dy, dy2=None):
        C = _ops.ext()
        xp, mask, gamma, mean, rstd = ctx.saved_tensors
        training, relu, has_res = ctx.bn_flags
        needs_dres = has_res and ctx.needs_input_grad[1]
        if dy is None:
            dy, dy2 = dy2, None
        if dy is None:
            return (None,) * 12
        if dy2 is not None:
            outs = C.bn_bwd2(xp, mask, _to_nhwc(dy), _to_nhwc(dy2), gamma,
                             mean, rstd, training, relu)
        else:
            outs = C.bn_bwd(xp, mask, _to_nhwc(dy), gamma, mean, rstd,
                            training, relu, needs_dres)
        dx = _from_nhwc(outs[0])
        dres = _from_nhwc(outs[3]) if needs_dres else None
        return (dx, dres, outs[1], outs[2], None, None, None, None, None,
                None, None, None)


def batch_norm_act(x, gamma, beta, running_mean, running_var,
                   momentum=0.1, eps=1e-5, training=True, relu=False,
                   residual=None, fork=False, slab=None):
    """Fused BatchNorm(+residual add)(+ReLU).

    bf16 channels_last GPU tensors hit the CDNA4 kernels; everything else
    runs the reference torch path (same math, also the numerics oracle).

    ``fork=True`` is for an output with two consumers (a bottleneck's
    output feeds the next block's first convolution and its residual
    branch) and returns a pair, one member for each. On the kernel path
    the two are one tensor under two handles, so the backward gets the
    consumers' gradients separately and sums them inside its reduction
    kernel (bn_bwd2) instead of autograd adding them first; results are
    bitwise the same. A consumer that leaves its member unused costs
    nothing: one gradient runs the one-gradient kernels. On the
    reference path, and with SPARKDL_FUSED_RESGRAD=0 on the kernel path
    too, the pair is ``(y, y)`` and autograd adds as usual.

    ``slab`` is for ``conv1x1_bn_act``: x's partial sums from the
    kernel that wrote x (kernel path and training mode only)."""
    # The NHWC kernels stage per-channel folds in LDS sized for
    # C <= 2048 (csrc/batchnorm.hip `lds[kFoldFloats]`) and read bf16 in
    # 8-wide packs; larger or ragged channel counts take the reference
    # path rather than corrupting LDS.
    C = x.shape[1]
    if (x.is_cuda and x.dtype == torch.bfloat16
            and C <= 2048 and C % 8 == 0):
        if fork and os.environ.get("SPARKDL_FUSED_RESGRAD", "1") != "0":
            return _BNReLUFn.apply(x, residual, gamma, beta, running_mean,
                                   running_var, momentum, eps, training,
                                   relu, True, slab)
        y = _BNReLUFn.apply(x, residual, gamma, beta, running_mean,
                            running_var, momentum, eps, training, relu,
                            False, slab)
        return (y, y) if fork else y
    assert slab is None, "a statistics slab needs the kernel path"
    # reference path: fp32 compute (stats/affine are fp32), cast back
    y = torch.nn.functional.batch_norm(
        x.float(), running_mean, running_var, gamma, beta,
        training, momentum, eps).to(x.dtype)
    if residual is not None:
        y = y + residual
    y = torch.relu(y) if relu else y
    return (y, y) if fork else y


class _BNReLUPoolFn(torch.autograd.Function):
    """maxpool3x3s2p1(relu(bn(x))) in one kernel chain. Besides x and
    the statistics, backward keeps one byte per pooled element (the
    winning tap, or "no gradient"): no full-resolution y, ReLU mask,
    int64 pool indices or full-resolution dy exist."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum,
                eps, training):
        C = _ops.ext()
        xp = _to_nhwc(x)
        pooled, mean, rstd, code = C.bn_pool_fwd(
            xp, gamma, beta, running_mean, running_var, momentum, eps,
            training)
        ctx.save_for_backward(xp, code, gamma, mean, rstd)
        ctx.bn_training = training
        return _from_nhwc(pooled)

    @staticmethod
    def backward(ctx, dy):
        C = _ops.ext()
        xp, code, gamma, mean, rstd = ctx.saved_tensors
        dx, dgamma, dbeta = C.bn_pool_bwd(
            xp, code, _to_nhwc(dy), gamma, mean, rstd, ctx.bn_training)
        return _from_nhwc(dx), dgamma, dbeta, None, None, None, None, None


def batch_norm_relu_maxpool(x, gamma, beta, running_mean, running_var,
                            momentum=0.1, eps=1e-5, training=True):
    """``max_pool2d(relu(batch_norm(x)), 3, stride=2, padding=1)``, the
    ResNet stem epilogue.

    bf16 GPU tensors with C % 8 == 0 and C <= 2048 run the fused CDNA4
    kernels, whose outputs, running statistics and gradients are bitwise
    those of the composed path; everything else (CPU included) composes
    batch_norm_act(relu=True) with torch's max_pool2d.
    SPARKDL_FUSED_STEM=0 forces the composed path."""
    C = x.shape[1]
    if (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4
            and C <= 2048 and C % 8 == 0
            and 0 < x.numel() // C < 2 ** 31
            and os.environ.get("SPARKDL_FUSED_STEM", "1") != "0"):
        return _BNReLUPoolFn.apply(x, gamma, beta, running_mean,
                                   running_var, momentum, eps, training)
    y = batch_norm_act(x, gamma, beta, running_mean, running_var,
                       momentum=momentum, eps=eps, training=training,
                       relu=True)
    return torch.nn.functional.max_pool2d(y, 3, stride=2, padding=1)


def layer_norm(x, gamma, beta, eps=1e-5):
    """LayerNorm over the last dim. HIP kernel for bf16-on-GPU, reference
    path otherwise (CPU tests)."""
    if x.is_cuda and x.dtype == torch.bfloat16:
        return _LayerNormFn.apply(x, gamma, beta, eps)
    return torch.nn.functional.layer_norm(
        x, (x.shape[-1],), gamma.to(x.dtype), beta.to(x.dtype), eps)


def _mul32(x, c):
    """x * c mod 2^32 on int64 tensors holding 32-bit values, without
    leaving the int64 range."""
    lo = x * (c & 0xffff)
    hi = (x * (c >> 16)) & 0xffff
    return (lo + (hi << 16)) & 0xffffffff


def dropout_keep_mask(seed, rows, cols, p, device="cpu"):
    """The keep mask of the dropout_add_layer_norm kernels as a bool
    ``[rows, cols]`` tensor, in integer torch ops. This is the kernels'
    specification: forward and backward regenerate exactly this mask
    from the seed and store none.

    ``seed`` (an int or a one-element integer tensor) is truncated to
    its low 32 bits, and the element index ``i = row * cols + col`` is
    a 32-bit unsigned number (``rows * cols < 2^31``)::

        x = seed ^ (i * 2654435761)        all mod 2^32
        x ^= x >> 16;  x *= 0x7feb352d
        x ^= x >> 15;  x *= 0x846ca68b
        x ^= x >> 16
        keep = (x & 0xffffff) >= p24,  p24 = int(float32(p) * 2^24)

    so ``p24 == 0`` keeps everything and an element is kept with
    probability ``1 - p24 / 2^24``. It is the counter hash (drop_hash
    in csrc/common.hip.h) that the attention kernels use for
    attention-probability dropout."""
    if not 0 <= rows * cols < 2 ** 31:
        raise ValueError("rows * cols must be below 2^31")
    if not 0.0 <= p < 1.0:
        raise ValueError("p must be in [0, 1), got %r" % (p,))
    seed = int(seed) & 0xffffffff
    p24 = int(torch.tensor(p, dtype=torch.float32).item() * 16777216.0)
    i = torch.arange(rows * cols, dtype=torch.int64, device=device)
    x = _mul32(i, 2654435761) ^ seed
    x = _mul32(x ^ (x >> 16), 0x7feb352d)
    x = _mul32(x ^ (x >> 15), 0x846ca68b)
    x = x ^ (x >> 16)
    return ((x & 0xffffff) >= p24).view(rows, cols)


class _DropoutAddLayerNormFn(torch.autograd.Function):
    """y = ln(h), h = residual + dropout(x), through dropout_add_ln_fwd
    / _bwd. Saves h and the statistics; the mask is regenerated from
    the step's seed."""

    @staticmethod
    def forward(ctx, x, residual, gamma, beta, p, eps):
        C = _ops.ext()
        seed = None
        if p > 0:
            # the attention kernels' counter: advanced on the device, so
            # a captured graph advances it on replay, and cloned so that
            # backward replays this step's mask
            seed = _attn_seed_tensor(x.device)
            seed.add_(1)
            seed = seed.clone()
        y, h, mean, rstd = C.dropout_add_ln_fwd(
            x.contiguous(), residual.contiguous(), gamma, beta, eps,
            float(p), seed)
        ctx.save_for_backward(h, gamma, mean, rstd,
                              seed if seed is not None else
                              torch.empty(0))
        ctx.dropout_p = float(p)
        return y

    @staticmethod
    def backward(ctx, dy):
        C = _ops.ext()
        h, gamma, mean, rstd, seed = ctx.saved_tensors
        if seed.numel() == 0:
            seed = None
        d_sub, d_res, dgamma, dbeta = C.dropout_add_ln_bwd(
            h, dy.contiguous(), gamma, mean, rstd, ctx.dropout_p, seed)
        return d_sub, d_res, dgamma, dbeta, None, None


def dropout_add_layer_norm(x, residual, gamma, beta, p=0.0, training=True,
                           eps=1e-5):
    """``layer_norm(residual + dropout(x, p, training))``, the tail of a
    post-norm transformer sublayer.

    bf16 GPU tensors of one shape with ``p < 1``, at most 8192 columns
    and fewer than 2^31 elements run one HIP kernel forward and one
    backward (csrc/layernorm.hip): no dropped tensor, no sum and no mask
    travel through memory in between, and no mask is kept for backward.
    The mask is ``dropout_keep_mask`` under the per-device seed counter
    that attention dropout uses (it advances by one per training call
    with ``p > 0``); given that mask, outputs and gradients are bitwise
    those of bf16 dropout, bf16 add and ``layer_norm`` composed. The
    mask is not torch's: the same ``torch.manual_seed`` gives another
    draw than the composed path.

    Everything else (CPU, fp32, ``p == 1``, wider rows) runs the
    composed path on torch's dropout."""
    cols = x.shape[-1] if x.dim() else 0
    if (x.is_cuda and x.dtype == torch.bfloat16
            and residual.is_cuda and residual.dtype == torch.bfloat16
            and residual.shape == x.shape and p < 1
            and cols <= 8192 and 0 < x.numel() < 2 ** 31):
        return _DropoutAddLayerNormFn.apply(
            x, residual, gamma, beta, p if training else 0.0, eps)
    return layer_norm(
        residual + torch.nn.functional.dropout(x, p, training),
        gamma, beta, eps)


def bias_gelu(x, bias):
    """Fused bias+GELU (erf). HIP kernel for bf16-on-GPU, reference path
    otherwise."""
    if x.is_cuda and x.dtype == torch.bfloat16:
        return _BiasGeluFn.apply(x, bias)
    return torch.nn.functional.gelu(x + bias.to(x.dtype), approximate="none")


# ---------------------------------------------------------------------------
# Fused MFMA GEMM + bias + GELU
# ---------------------------------------------------------------------------

_zero_bias_cache = {}


def _zero_bias(n, device):
    key = (n, device)
    if key not in _zero_bias_cache:
        _zero_bias_cache[key] = torch.zeros(
            n, dtype=torch.float32, device=device)
    return _zero_bias_cache[key]


class _LinearGeluFusedFn(torch.autograd.Function):
    """y = gelu(x @ W^T + b) with the GEMM + epilogue in one hand-written
    MFMA kernel; backward reuses the bias_gelu_bwd kernel on the saved
    pre-activation and rocBLAS for dgrad/wgrad."""

    @staticmethod
    def forward(ctx, x2d, weight, bias):
        C = _ops.ext()
        y, z = C.gemm_bias_act(x2d, weight, bias, 1, True)
        ctx.save_for_backward(x2d, weight, z)
        return y

    @staticmethod
    def backward(ctx, dy):
        C = _ops.ext()
        x2d, weight, z = ctx.saved_tensors
        dy = dy.contiguous()
        # dz = dy * gelu'(z); dbias = column-sum(dz)
        dz, dbias = C.bias_gelu_bwd(z, _zero_bias(z.shape[-1], z.device),
                                    dy)
        # dgrad through the same MFMA kernel: dX[M,K] = dZ[M,N] @ W[N,K]
        # == gemm(A=dZ, B=W^T[K,N]) — W^T is weight-sized, transposed on
        # the fly by a tiled bf16 kernel.
        if (weight.shape[0] % 64 == 0
                and os.environ.get("SPARKDL_FUSED_DGRAD", "1") != "0"):
            # dgrad contracts over N
            wt = C.transpose_bf16(weight)
            dx = C.gemm_bias_act(dz, wt, None, 0, False)[0]
        else:
            dx = dz @ weight        # [M,N] @ [N,K]
        dw = _wgrad(dz, x2d)
        return dx, dw, dbias


def linear_gelu_fused(x, weight, bias):
    """Apply the fused MFMA GEMM+bias+GELU path; caller guarantees bf16
    CUDA tensors with K % 64 == 0 (M/N edges are handled in-kernel)."""
    shape = x.shape
    x2d = x.reshape(-1, shape[-1]).contiguous()
    y = _LinearGeluFusedFn.apply(x2d, weight.contiguous(), bias)
    return y.reshape(*shape[:-1], weight.shape[0])


def linear_gelu_fused_ok(x, weight):
    # the 256x256 kernel clamps/predicates M and N edges; only the
    # K-loop step (64) is a hard requirement
    return (x.is_cuda and x.dtype == torch.bfloat16
            and weight.dtype == torch.bfloat16
            and x.shape[-1] % 64 == 0)


# ---------------------------------------------------------------------------
# Flash attention (SURVEY.md N6 attention GEMMs) — hand-written fwd+bwd,
# D=64 heads, replaces torch SDPA (aotriton) on the BERT hot path.
# ---------------------------------------------------------------------------

_attn_seed = {}


def _attn_seed_tensor(device):
    """Per-device persistent dropout seed, advanced by a DEVICE op each
    forward so the pattern changes per step even under hipGraph capture
    (the increment is captured and replayed). Offset by the launcher's
    RANK: data-parallel ranks seed torch identically for weight init,
    which must not make their dropout masks identical too."""
    if device not in _attn_seed:
        rank = int(os.environ.get("RANK", "0"))
        _attn_seed[device] = torch.randint(
            0, 2 ** 31, (1,), dtype=torch.int64,
            device=device) + rank * 2654435761 % (2 ** 31)
    return _attn_seed[device]


class _FlashAttnFn(torch.autograd.Function):
    """O = softmax(Q K^T / sqrt(64)) V with optional attention-prob
    dropout. q/k/v: [BH, S, 64] bf16 contiguous, S % 64 == 0.
    seq_lens (optional): int32 [BH] on the same device — right-padded
    rows, masked_attention_ref semantics; it gets no gradient."""

    @staticmethod
    def forward(ctx, q, k, v, dropout_p, seq_lens=None):
        C = _ops.ext()
        seed = None
        if dropout_p > 0:
            seed = _attn_seed_tensor(q.device)
            seed.add_(1)
            # the backward must replay this step's seed even if later
            # steps advanced the counter
            seed = seed.clone()
        o, lse = C.attn_fwd(q, k, v, float(dropout_p), seed, seq_lens)
        ctx.save_for_backward(q, k, v, o, lse,
                              seed if seed is not None else
                              torch.empty(0), seq_lens)
        ctx.dropout_p = float(dropout_p)
        return o

    @staticmethod
    def backward(ctx, do):
        C = _ops.ext()
        q, k, v, o, lse, seed, seq_lens = ctx.saved_tensors
        if seed.numel() == 0:
            seed = None
        do = do.contiguous()
        # D_i = rowsum(dO o O), fp32 (flash backward precompute)
        drow = (do.float() * o.float()).sum(-1)
        dq, dk, dv = C.attn_bwd(q, k, v, do, lse, drow, ctx.dropout_p,
                                seed, seq_lens)
        return dq, dk, dv, None, None


def flash_attention(q, k, v, dropout_p=0.0, seq_lens=None):
    """[B, h, S, d] attention through the hand-written kernels; the
    caller checks flash_attention_ok first.

    seq_lens (optional): int32 [B] on q's device, the valid length of
    each right-padded batch row (masked_attention_ref semantics: padded
    query rows come back exactly zero). The lengths are only ever read
    on the device, so the call stays sync-free and graph-capturable."""
    B, h, S, d = q.shape
    q3 = q.reshape(B * h, S, d).contiguous()
    k3 = k.reshape(B * h, S, d).contiguous()
    v3 = v.reshape(B * h, S, d).contiguous()
    if seq_lens is not None:
        # the [BH,S,64] kernels index lengths per bh
        seq_lens = seq_lens.view(B, 1).expand(B, h).reshape(B * h)
    o = _FlashAttnFn.apply(q3, k3, v3, dropout_p, seq_lens)
    return o.view(B, h, S, d)


def flash_attention_ok(q):
    return (q.is_cuda and q.dtype == torch.bfloat16 and q.dim() == 4
            and q.shape[-1] == 64 and q.shape[-2] % 64 == 0)


class _FlashAttnPackedFn(torch.autograd.Function):
    """Zero-copy BERT attention: reads the packed qkv buffer
    [B,S,3,H,64] (the qkv Linear's output, viewed) with strided kernel
    rows, writes O directly as [B,S,H*64], and the backward emits the
    packed dqkv the qkv Linear's backward consumes — no permute/
    contiguous copies anywhere around the attention."""

    @staticmethod
    def forward(ctx, qkv, dropout_p, seq_lens=None):
        C = _ops.ext()
        seed = None
        if dropout_p > 0:
            seed = _attn_seed_tensor(qkv.device)
            seed.add_(1)
            seed = seed.clone()
        o, lse = C.attn_fwd_packed(qkv, float(dropout_p), seed, seq_lens)
        ctx.save_for_backward(qkv, o, lse,
                              seed if seed is not None else
                              torch.empty(0), seq_lens)
        ctx.dropout_p = float(dropout_p)
        return o

    @staticmethod
    def backward(ctx, do):
        C = _ops.ext()
        qkv, o, lse, seed, seq_lens = ctx.saved_tensors
        if seed.numel() == 0:
            seed = None
        do = do.contiguous()
        B, S, HD = o.shape
        H = HD // 64
        # D_i = rowsum(dO o O) per (b,h,s): [B,S,H] -> [B*H, S]
        drow = (do.float() * o.float()).view(B, S, H, 64).sum(-1) \
            .transpose(1, 2).reshape(B * H, S).contiguous()
        dqkv = C.attn_bwd_packed(qkv, do, lse, drow, ctx.dropout_p, seed,
                                 seq_lens)
        return dqkv, None, None


def flash_attention_packed(qkv, dropout_p=0.0, seq_lens=None):
    """qkv: [B, S, 3, H, 64] bf16 contiguous -> O [B, S, H*64].

    seq_lens (optional): int32 [B] on qkv's device, the valid length of
    each right-padded batch row. Row b attends over keys [0, len_b);
    O rows >= len_b and the matching dqkv rows are exactly zero, and
    the kernels skip whole 64-wide tiles beyond len_b, so a padded
    batch costs about len^2, not S^2. Lengths are read on the device
    only: no host sync, graph-capturable, and the tensor may be
    refilled in place between graph replays. seqlens_from_mask turns an
    attention_mask into lengths (its validation syncs; passing seq_lens
    is the sync-free path)."""
    return _FlashAttnPackedFn.apply(qkv.contiguous(), dropout_p, seq_lens)


def _conv_gemm(a2d, w):
    """Best-kernel cascade for bias-free GEMMs (1x1 conv fwd/dgrad):
    streaming tall-skinny kernel when the shape fits, else the 256x256
    tile kernel, else the library GEMM."""
    C = _ops.ext()
    M, K = a2d.shape
    N = w.shape[0]
    if (K in (64, 128, 256)) and N % 64 == 0:
        return C.gemm_stream(a2d, w)
    if K % 64 == 0:
        return C.gemm_bias_act(a2d, w, None, 0, False)[0]
    return a2d @ w.t()


def _wgrad(dz, x2d):
    """Weight gradient dW = dZ^T @ X. Default: library GEMM (Tensile's
    split-K TN kernels measure ~650 TF on the BERT shapes vs the
    in-house tr_b16 kernel's 506-534 — probe ladder in
    profiles/wgrad_*.log). SPARKDL_FUSED_WGRAD=1 opts into the
    in-house kernel where its shape constraints hold."""
    if (os.environ.get("SPARKDL_FUSED_WGRAD", "0") == "1"
            and dz.shape[1] % 256 == 0 and x2d.shape[1] % 128 == 0
            and dz.shape[0] % 64 == 0):
        C = _ops.ext()
        return C.wgrad_splitk(dz, x2d).to(dz.dtype)
    return dz.t() @ x2d


def _wgrad_splitk(dy, x2d, chunk_rows=32768):
    """dW[N,K] = dy^T @ x for tall-skinny operands. A single TN GEMM
    with a tiny N x K output gives Tensile a near-empty grid (measured
    ~2 ms for the ResNet L1 wgrad); splitting the huge contraction into
    row chunks via a batched GEMM fills the chip, then the partials
    reduce in fp32."""
    M = dy.shape[0]
    if M <= 2 * chunk_rows:
        return dy.t() @ x2d
    # smallest divisor split keeping chunks near the target (avoids
    # padded copies of the big operands; NHW row counts are highly
    # composite)
    S = 0
    for s in range((M + chunk_rows - 1) // chunk_rows, 257):
        if M % s == 0:
            S = s
            break
    if S == 0:
        return dy.t() @ x2d
    cr = M // S
    dyb = dy.view(S, cr, -1).transpose(1, 2)
    xb = x2d.view(S, cr, -1)
    return torch.bmm(dyb, xb).sum(0, dtype=torch.float32).to(dy.dtype)


class _Conv1x1Fn(torch.autograd.Function):
    """y = x @ W^T over NHWC rows (1x1 conv). Forward and dgrad run on
    the in-house kernels (streaming kernel at the ResNet shapes);
    wgrad on the library GEMM."""

    @staticmethod
    def forward(ctx, x2d, weight):
        ctx.save_for_backward(x2d, weight)
        return _conv_gemm(x2d, weight)

    @staticmethod
    def backward(ctx, dy):
        C = _ops.ext()
        x2d, weight = ctx.saved_tensors
        dy = dy.contiguous()
        wt = C.transpose_bf16(weight)
        dx = _conv_gemm(dy, wt)
        dw = _wgrad_splitk(dy, x2d)
        return dx, dw


def conv1x1_gemm(x_nhwc, weight):
    """x_nhwc: [..., Cin] bf16; weight [Cout, Cin] bf16."""
    shape = x_nhwc.shape
    x2d = x_nhwc.reshape(-1, shape[-1]).contiguous()
    y = _Conv1x1Fn.apply(x2d, weight.contiguous())
    return y.reshape(*shape[:-1], weight.shape[0])


# ---------------------------------------------------------------------------
# 1x1 convolution forward that also writes the BatchNorm partial sums
# ---------------------------------------------------------------------------

# (Cin, Cout) of the stride-1 1x1 sites that take the fused forward by
# default: those where scripts/probe_conv1x1_bn.py measured
# conv1x1_stats + finalize faster than MIOpen + bn_stats_k + finalize
# at batch 512 (profiles/probe_conv1x1_bn.log): all six stride-1 shapes
# with Cin <= 256 of ResNet-50, by 16 to 123 us per call.
CONV1X1_STATS_SITES = frozenset({
    (64, 64), (64, 256), (256, 64), (256, 128), (128, 512), (256, 1024),
})


def conv1x1_stats_supported(cin, cout):
    """Shapes the conv1x1_stats kernel takes at all."""
    return cin in (64, 128, 256) and cout >= 64 and cout % 64 == 0


def conv1x1_stats_route(cin, cout, stride=1, mode=None):
    """Whether a 1x1 convolution followed by a training-mode BatchNorm
    runs the fused forward. ``mode`` defaults to SPARKDL_CONV1X1_STATS:
    "0" never, "all" wherever the kernel supports the shape, anything
    else (the default) at CONV1X1_STATS_SITES; never under
    SPARKDL_CONV1X1=all. The row count plays no
    part: the kernel is exact at any M >= 1."""
    if mode is None:
        mode = os.environ.get("SPARKDL_CONV1X1_STATS", "1")
    if mode == "0" or stride != 1 or not conv1x1_stats_supported(cin, cout):
        return False
    # SPARKDL_CONV1X1=all keeps its meaning: every 1x1 on gemm_stream
    if os.environ.get("SPARKDL_CONV1X1", "0") == "all":
        return False
    return mode == "all" or (cin, cout) in CONV1X1_STATS_SITES


class _Conv1x1StatsFn(torch.autograd.Function):
    """y = conv1x1(x, w) on channels_last bf16 tensors through
    conv1x1_stats: returns (y, slab), the slab (partial sums of y for
    the BatchNorm that follows) non-differentiable. No copies:
    channels_last [N,C,H,W] is [N*H*W, C] as a view, and so is y.
    Backward is ATen's convolution_backward on the channels_last
    tensors, i.e. the MIOpen dgrad and wgrad of the unfused path."""

    @staticmethod
    def forward(ctx, x, weight):
        C = _ops.ext()
        n, cin, h, w = x.shape
        x2d = x.permute(0, 2, 3, 1).reshape(n * h * w, cin)
        y2d, slab = C.conv1x1_stats(x2d, weight, 0)
        ctx.save_for_backward(x, weight)
        ctx.mark_non_differentiable(slab)
        # no zero tensor for the slab's absent gradient
        ctx.set_materialize_grads(False)
        y = y2d.view(n, h, w, weight.shape[0]).permute(0, 3, 1, 2)
        return y, slab

    @staticmethod
    def backward(ctx, dy, _dslab):
        if dy is None:
            return None, None
        x, weight = ctx.saved_tensors
        w4 = weight.view(weight.shape[0], weight.shape[1], 1, 1)
        dx, dw, _ = torch.ops.aten.convolution_backward(
            dy, x, w4, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
            [ctx.needs_input_grad[0], ctx.needs_input_grad[1], False])
        if dw is not None:
            dw = dw.view_as(weight)
        return dx, dw


def conv1x1_bn_act(x, conv, bn, residual=None, fork=False):
    """``bn(conv(x), residual, fork)`` for a ``Conv1x1`` and a
    ``BatchNormAct2d``, which stay the owners of the parameters and
    buffers. Where ``conv1x1_stats_route`` says so (training mode, bf16
    channels_last on the GPU) the convolution forward is the read-once
    kernel that also writes the BatchNorm partial sums, and the
    BatchNorm skips its statistics pass; otherwise, eval mode included,
    this is exactly the two module calls."""
    if (bn.training and x.is_cuda and x.dtype == torch.bfloat16
            and x.dim() == 4
            and x.is_contiguous(memory_format=torch.channels_last)
            and bn.num_features == conv.cout
            and conv1x1_stats_route(conv.cin, conv.cout, conv.stride)):
        y, slab = _Conv1x1StatsFn.apply(x, conv.weight.to(x.dtype))
        return batch_norm_act(
            y, bn.weight, bn.bias, bn.running_mean, bn.running_var,
            momentum=bn.momentum, eps=bn.eps, training=True, relu=bn.relu,
            residual=residual, fork=fork, slab=slab)
    return bn(conv(x), residual=residual, fork=fork)


class _LinearFusedFn(torch.autograd.Function):
    """y = x @ W^T + b with the bias fused into the MFMA GEMM epilogue
    (act=0). dgrad runs on the same kernel via W^T; wgrad/dbias on
    library GEMM / torch reductions."""

    @staticmethod
    def forward(ctx, x2d, weight, bias):
        C = _ops.ext()
        y = C.gemm_bias_act(x2d, weight, bias, 0, False)[0]
        ctx.save_for_backward(x2d, weight)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        C = _ops.ext()
        x2d, weight = ctx.saved_tensors
        dy = dy.contiguous()
        if (weight.shape[0] % 64 == 0
                and os.environ.get("SPARKDL_FUSED_DGRAD", "1") != "0"):
            wt = C.transpose_bf16(weight)
            dx = C.gemm_bias_act(dy, wt, None, 0, False)[0]
        else:
            dx = dy @ weight
        dw = _wgrad(dy, x2d)
        # dtype-arg sum fuses the bf16->fp32 conversion into the
        # reduction (no intermediate fp32 copy of dy)
        dbias = dy.sum(0, dtype=torch.float32) if ctx.has_bias else None
        return dx, dw, dbias


def linear_fused(x, weight, bias):
    """Fused-bias MFMA linear (act=0); same eligibility rule as
    linear_gelu_fused_ok."""
    shape = x.shape
    x2d = x.reshape(-1, shape[-1]).contiguous()
    y = _LinearFusedFn.apply(x2d, weight.contiguous(), bias)
    return y.reshape(*shape[:-1], weight.shape[0])
