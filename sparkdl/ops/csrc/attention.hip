// Flash attention (forward + backward), D=64 heads, bf16: the operand
// pre-transpose pass, the dense (CAUSAL=false) instantiations of the
// kernels of attention_kernels.hip.h — the design notes are at the top
// of that header — and the launchers behind kernels.h. The causal
// instantiations live in attention_causal.hip.

#include "attention_kernels.hip.h"

namespace {

// ------------------------------------------------ pre-transpose pass
// T[bh][d][s] = X(bh, s, d) where X rows are `rs` elements apart.
// One workgroup per (bh, 64-row s-block); LDS 64x64 transpose with
// padded rows.

__global__ __launch_bounds__(ATHREADS) void attn_pretranspose_k(
    const short* __restrict__ X, short* __restrict__ T, int S, int H,
    int rs) {
  __shared__ short tile[64][64 + 8];
  const int bh = blockIdx.x;
  const int sb = blockIdx.y;
  const long long base =
      ((long long)(bh / H) * S + (long long)sb * 64) * rs +
      (long long)(bh % H) * 64;
  // load 64 rows x 64 cols: 256 threads x 16 B, 2 sweeps
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const int r = w * 32 + threadIdx.x / 8;
    const int c = (threadIdx.x % 8) * 8;
    const bf16x8 v = *(const bf16x8*)(X + base + (long long)r * rs + c);
    *(bf16x8*)&tile[r][c] = v;
  }
  __syncthreads();
  short* out = T + ((long long)bh * 64) * S + sb * 64;
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const int d = w * 32 + threadIdx.x / 8;   // output row (= input col)
    const int s0 = (threadIdx.x % 8) * 8;     // output col (= input row)
    bf16x8 v;
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = tile[s0 + u][d];
    *(bf16x8*)&out[(long long)d * S + s0] = v;
  }
}

}  // namespace

void launch_attn_pretranspose(const short* X, short* T, int BH, int S,
                              int H, int rs, hipStream_t stream) {
  hipLaunchKernelGGL(attn_pretranspose_k, dim3(BH, S / 64),
                     dim3(ATHREADS), 0, stream, X, T, S, H, rs);
}

// The dispatch is the 2x2 of (seqlens, causal): the causal half is
// launch_attn_*_causal.
void launch_attn_fwd(const short* Q, const short* K, const short* VT,
                     short* O, float* LSE, const long long* seed, int BH,
                     int S, int H, int rs, int ors, float dropout_p,
                     const int* seqlens, bool causal, hipStream_t stream) {
  if (causal)
    return launch_attn_fwd_causal(Q, K, VT, O, LSE, seed, BH, S, H, rs,
                                  ors, dropout_p, seqlens, stream);
  const unsigned p24 = (unsigned)(dropout_p * 16777216.0f);
  const float inv1mp = dropout_p > 0.f ? 1.f / (1.f - dropout_p) : 1.f;
  // no lengths: the fixed-length instantiation, untouched by VARLEN
  auto* fwd = seqlens ? attn_fwd_k<true, false> : attn_fwd_k<false, false>;
  hipLaunchKernelGGL(fwd, dim3(BH, S / BQ), dim3(ATHREADS), 0, stream, Q,
                     K, VT, O, LSE, seed, S, H, rs, ors, p24, inv1mp,
                     seqlens);
}

void launch_attn_bwd(const short* Q, const short* K, const short* V,
                     const short* dO, const short* QT, const short* DOT,
                     const short* KT, const float* LSE, const float* Drow,
                     short* dQ, short* dK, short* dV,
                     const long long* seed, int BH, int S, int H, int rs,
                     int ors, int grs, float dropout_p,
                     const int* seqlens, bool causal, hipStream_t stream) {
  if (causal)
    return launch_attn_bwd_causal(Q, K, V, dO, QT, DOT, KT, LSE, Drow, dQ,
                                  dK, dV, seed, BH, S, H, rs, ors, grs,
                                  dropout_p, seqlens, stream);
  const unsigned p24 = (unsigned)(dropout_p * 16777216.0f);
  const float inv1mp = dropout_p > 0.f ? 1.f / (1.f - dropout_p) : 1.f;
  auto* dkdv = seqlens ? attn_bwd_dkdv_k<true, false>
                       : attn_bwd_dkdv_k<false, false>;
  auto* dq = seqlens ? attn_bwd_dq_k<true, false>
                     : attn_bwd_dq_k<false, false>;
  hipLaunchKernelGGL(dkdv, dim3(BH, S / BKV), dim3(ATHREADS), 0, stream,
                     Q, K, V, dO, QT, DOT, LSE, Drow, dK, dV, seed, S, H,
                     rs, ors, grs, p24, inv1mp, seqlens);
  hipLaunchKernelGGL(dq, dim3(BH, S / BQ), dim3(ATHREADS), 0, stream, Q,
                     K, V, dO, KT, LSE, Drow, dQ, seed, S, H, rs, ors,
                     grs, p24, inv1mp, seqlens);
}
