// Causal flash attention: the CAUSAL=true instantiations of the kernels
// of attention_kernels.hip.h (triangular tile schedule; the design notes
// are at the top of that header) and their launchers. A translation unit
// of its own so that the dense kernels of attention.hip are compiled
// exactly as before, while this new code is generated without packed
// fp32 instructions, like the other recent kernels here.

// device code of this file is generated without packed fp32 instructions
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

#include "attention_kernels.hip.h"

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// Same grid as the dense launch: one workgroup per (bh, 64-row tile);
// the kernels reverse blockIdx.y where that issues the longest first.
void launch_attn_fwd_causal(const short* Q, const short* K,
                            const short* VT, short* O, float* LSE,
                            const long long* seed, int BH, int S, int H,
                            int rs, int ors, float dropout_p,
                            const int* seqlens, hipStream_t stream) {
  const unsigned p24 = (unsigned)(dropout_p * 16777216.0f);
  const float inv1mp = dropout_p > 0.f ? 1.f / (1.f - dropout_p) : 1.f;
  auto* fwd = seqlens ? attn_fwd_k<true, true> : attn_fwd_k<false, true>;
  hipLaunchKernelGGL(fwd, dim3(BH, S / BQ), dim3(ATHREADS), 0, stream, Q,
                     K, VT, O, LSE, seed, S, H, rs, ors, p24, inv1mp,
                     seqlens);
}

void launch_attn_bwd_causal(const short* Q, const short* K, const short* V,
                            const short* dO, const short* QT,
                            const short* DOT, const short* KT,
                            const float* LSE, const float* Drow, short* dQ,
                            short* dK, short* dV, const long long* seed,
                            int BH, int S, int H, int rs, int ors, int grs,
                            float dropout_p, const int* seqlens,
                            hipStream_t stream) {
  const unsigned p24 = (unsigned)(dropout_p * 16777216.0f);
  const float inv1mp = dropout_p > 0.f ? 1.f / (1.f - dropout_p) : 1.f;
  auto* dkdv = seqlens ? attn_bwd_dkdv_k<true, true>
                       : attn_bwd_dkdv_k<false, true>;
  auto* dq = seqlens ? attn_bwd_dq_k<true, true>
                     : attn_bwd_dq_k<false, true>;
  hipLaunchKernelGGL(dkdv, dim3(BH, S / BKV), dim3(ATHREADS), 0, stream,
                     Q, K, V, dO, QT, DOT, LSE, Drow, dK, dV, seed, S, H,
                     rs, ors, grs, p24, inv1mp, seqlens);
  hipLaunchKernelGGL(dq, dim3(BH, S / BQ), dim3(ATHREADS), 0, stream, Q,
                     K, V, dO, KT, LSE, Drow, dQ, seed, S, H, rs, ors,
                     grs, p24, inv1mp, seqlens);
}
