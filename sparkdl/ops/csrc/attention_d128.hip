// Flash attention (forward + backward) for 128-wide heads, bf16, fp32
// accumulation:
//
//   O = softmax(Q K^T / sqrt(128)) V     S % 64 == 0, head dim 128
//
// Same contract as the D=64 family of attention_kernels.hip.h (strided
// rows for the packed [B,S,3,H,128] buffer, right-padded `seqlens` read
// on the device, the causal triangle, LSE, the (seed, bh, q*S+k) dropout
// hash; template <VARLEN, CAUSAL>), but a design of its own, because the
// D=64 one does not scale to 128:
//
//   * No pre-transposed operands and no [BH,128,S] scratch. The products
//     that need a transposed operand (V for P.V; dO and Q for dV and dK;
//     K for dQ) read it as an MFMA fragment from the SAME row-major tile
//     the QK-type product reads, with ds_read_b64_tr_b16: a 16-lane group
//     reads 4 rows x 16 columns, lane l naming row l/4, columns
//     4*(l%4)..+4 and receiving column l%16 of the 4 rows (semantics:
//     experimental/tr_b16_probe.hip). Two reads, rows 8g..8g+3 and
//     8g+4..8g+7 for group g, make one B-operand fragment. Each lane
//     supplies its own address, so the st_16x32 swizzle is absorbed
//     there: an 8-byte piece never leaves its 16-byte chunk.
//   * A [64][128] operand tile is two [64][64] half-tiles, one per half
//     of the head dimension, so stage_tile64 / lds_frag / the swizzle of
//     mfma_tile.hip.h apply unchanged. QK-type products take 4 K-steps
//     of 32; the output accumulators are 8 fragments of 16x16 per wave.
//   * The softmax scale 2^-3.5 is applied in fp32 to the scores (the
//     D=64 kernels round it into the bf16 Q operand, exact only for a
//     power of two). All three kernels compute s = acc * scale the same
//     way, so exp(s - LSE) in the backward reproduces the forward's P.
//
// LDS per workgroup: 72 KiB in each kernel (two workgroups per CU):
//   fwd:   K, V   2 buffers x 2 operands x 16 KiB, + P  8 KiB
//   dK/dV: Q, dO  64 KiB                            + PmT/dST 8 KiB
//   dQ:    K, V   64 KiB                            + dS 8 KiB
// Double-buffered staging with one wait and one barrier per tile; the
// all-padding early exit is block-uniform and taken before any barrier;
// masked p / dS are zero by selection; no atomics, no memset, no host
// sync: graph-capturable, and the same bits on every run.
//
// Bank conflicts of the transposing reads: a 16-lane group reads 4 rows
// x 32 B. Rows are 128 B; the swizzle XORs the 16 B chunk index with
// row & 7, so rows r and r+2 (same 128 B half of a 256 B bank period)
// land on different 32 B pairs: conflict-free inside a group. Groups g
// and g+1 read rows 8 apart, i.e. the same chunks of rows with the same
// parity: if the hardware serves two groups per pass that is 2-way. Not
// measured with counters (profiles/README.md).

// device code of this file is generated without packed fp32 instructions
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

#include "attention_d128_tile.hip.h"  // TrLane, stage_tile128, launch_d128

namespace {

// ------------------------------------------------------------- fwd

template <bool VARLEN, bool CAUSAL>
__global__ __launch_bounds__(ATHREADS) void attn_d128_fwd_k(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ V, short* __restrict__ O,
    float* __restrict__ LSE, const long long* __restrict__ seed_p, int S,
    int H, int rs, int ors, unsigned p24, float inv1mp,
    const int* __restrict__ seqlens) {
  extern __shared__ __attribute__((aligned(16))) short lds[];
  short* lK = lds;                      // [2][key][128], double-buffered
  short* lV = lds + 2 * kOperandElems;  // [2][key][128]
  short* lP = lds + 4 * kOperandElems;  // [q][key]

  const int bh = blockIdx.x;
  // CAUSAL: tile qt runs qt+1 trips, the longest are issued first
  const int qt = CAUSAL ? gridDim.y - 1 - blockIdx.y : blockIdx.y;
  const long long base =
      ((long long)(bh / H) * S) * rs + (long long)(bh % H) * D128;
  const long long obase =
      ((long long)(bh / H) * S) * ors + (long long)(bh % H) * D128;
  int len = S;
  if constexpr (VARLEN) {
    len = clamped_len(seqlens, bh / H, S);
    if (qt * BQ >= len) {  // block-uniform: the whole Q tile is padding
      zero_tile128(O + obase + (long long)qt * BQ * ors, ors, threadIdx.x);
      if (LSE && threadIdx.x < BQ)
        LSE[(long long)bh * S + qt * BQ + threadIdx.x] = 0.f;
      return;
    }
  }
  const unsigned seed = seed_p ? (unsigned)(*seed_p) : 0u;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;

  const FragLane fl(lane);
  const TrLane tr(lane);
  const unsigned lV_addr = lds_addr(lV);
  const float qscale = rsqrtf((float)D128);

  bf16x8 qf[4];
  {
    const int qrow = qt * BQ + wave * 16 + fl.frag_row;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      qf[ks] = *(const bf16x8*)(Q + base + (long long)qrow * rs + ks * 32 +
                                fl.frag_k);
  }

  float m_run[4], l_run[4];
  f32x4 o_acc[8];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m_run[r] = -1e30f;
    l_run[r] = 0.f;
  }
#pragma unroll
  for (int df = 0; df < 8; ++df) o_acc[df] = {0.f, 0.f, 0.f, 0.f};

  auto stage_kv = [&](int buf, int t) {
    stage_tile128(lK + buf * kOperandElems,
                  K + base + (long long)t * BKV * rs, rs, tid);
    stage_tile128(lV + buf * kOperandElems,
                  V + base + (long long)t * BKV * rs, rs, tid);
  };

  // VARLEN: only the tiles that hold a valid key (each holds >= 1).
  // CAUSAL: tiles 0..qt (under VARLEN qt*64 < len here, so each of
  // them holds a valid key as well)
  const int ntiles =
      CAUSAL ? qt + 1 : VARLEN ? (len + BKV - 1) / BKV : S / BKV;
  stage_kv(0, 0);
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    const int cur = t & 1;
    if (t + 1 < ntiles) stage_kv(cur ^ 1, t + 1);
    const short* lKc = lK + cur * kOperandElems;

    // CAUSAL: the diagonal tile (tile-uniform) carries the element mask
    const bool diag = CAUSAL && t == qt;

    f32x4 s_acc[4];
#pragma unroll
    for (int kf = 0; kf < 4; ++kf) {
      s_acc[kf] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        s_acc[kf] = mfma_bf16(
            qf[ks], lds_frag128(lKc, kf * 16 + fl.frag_row, ks, fl.frag_k),
            s_acc[kf]);
#pragma unroll
      for (int r = 0; r < 4; ++r) s_acc[kf][r] *= qscale;  // fp32 scale
    }

    // VARLEN: keys of this tile at or beyond kvalid are padding (only
    // in the tail tile); they leave the running max and get p = 0
    const int kvalid = VARLEN ? len - t * BKV : BKV;
    if constexpr (CAUSAL) {
      // diagonal tile only: keys after the query (and padded ones)
      if (diag) {
#pragma unroll
        for (int kf = 0; kf < 4; ++kf)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int kl = kf * 16 + fl.c_col;
            if (kl > wave * 16 + fl.c_sub_row + r || kl >= kvalid)
              s_acc[kf][r] = -1e30f;
          }
      }
    } else if constexpr (VARLEN) {
#pragma unroll
      for (int kf = 0; kf < 4; ++kf)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (kf * 16 + fl.c_col >= kvalid) s_acc[kf][r] = -1e30f;
    }

    float pmax[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float mx = s_acc[0][r];
#pragma unroll
      for (int kf = 1; kf < 4; ++kf) mx = fmaxf(mx, s_acc[kf][r]);
#pragma unroll
      for (int off = 1; off < 16; off <<= 1)
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
      pmax[r] = mx;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float m_new = fmaxf(m_run[r], pmax[r]);
      const float scale = __expf(m_run[r] - m_new);
      const int qrow = qt * BQ + wave * 16 + fl.c_sub_row + r;
      float rowsum = 0.f;
#pragma unroll
      for (int kf = 0; kf < 4; ++kf) {
        float p = __expf(s_acc[kf][r] - m_new);
        if constexpr (CAUSAL) {
          const int kl = kf * 16 + fl.c_col;
          if (diag)
            p = kl <= wave * 16 + fl.c_sub_row + r && kl < kvalid ? p : 0.f;
        } else if constexpr (VARLEN) {
          p = kf * 16 + fl.c_col < kvalid ? p : 0.f;
        }
        rowsum += p;  // l accumulates the UNdropped probabilities
        const float keep = drop_keep(seed, bh, qrow,
                                     t * BKV + kf * 16 + fl.c_col, S, p24,
                                     inv1mp);
        s_acc[kf][r] = p * keep;  // dropped P feeds the PV product
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1)
        rowsum += __shfl_xor(rowsum, off, 64);
      l_run[r] = l_run[r] * scale + rowsum;
      m_run[r] = m_new;
#pragma unroll
      for (int df = 0; df < 8; ++df) o_acc[df][r] *= scale;
    }

    // P round-trip through the wave's own rows of lP (no barrier)
#pragma unroll
    for (int kf = 0; kf < 4; ++kf)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        lds_st16(lP, (wave * 16 + fl.c_sub_row + r) * BKV + kf * 16 + fl.c_col,
                 f2bf(s_acc[kf][r]));
    // O += P V: V^T fragments by transposing reads of the row-major tile
    const unsigned lVc = lV_addr + cur * (kOperandElems * 2);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 af = lds_frag(lP, wave * 16 + fl.frag_row,
                                 ks * 32 + fl.frag_k);
#pragma unroll
      for (int df = 0; df < 8; ++df)
        o_acc[df] = mfma_bf16(
            af,
            tr.frag(lVc + (df >> 2) * (TILE_ELEMS * 2), ks * 32,
                    (df & 3) * 16),
            o_acc[df]);
    }
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_s_waitcnt(0);  // next tile's staging has landed
    __syncthreads();
  }

  const int qrow0 = qt * BQ + wave * 16;
#pragma unroll
  for (int df = 0; df < 8; ++df)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qrow = qrow0 + fl.c_sub_row + r;
      short o = f2bf(o_acc[df][r] / l_run[r]);
      if constexpr (VARLEN)  // tail Q tile: padded rows store zero
        o = qrow < len ? o : (short)0;
      O[obase + (long long)qrow * ors + df * 16 + fl.c_col] = o;
    }
  if (LSE && fl.c_col == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float lse = m_run[r] + __logf(l_run[r]);
      if constexpr (VARLEN) lse = qrow0 + fl.c_sub_row + r < len ? lse : 0.f;
      LSE[(long long)bh * S + qrow0 + fl.c_sub_row + r] = lse;
    }
  }
}

// --------------------------------------------------------- bwd dK/dV

template <bool VARLEN, bool CAUSAL>
__global__ __launch_bounds__(ATHREADS) void attn_d128_bwd_dkdv_k(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ V, const short* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ Drow,
    short* __restrict__ dK, short* __restrict__ dV,
    const long long* __restrict__ seed_p, int S, int H, int rs, int ors,
    int grs, unsigned p24, float inv1mp, const int* __restrict__ seqlens) {
  extern __shared__ __attribute__((aligned(16))) short lds[];
  short* lQ = lds;                       // [2][q][128]
  short* ldO = lds + 2 * kOperandElems;  // [2][q][128]
  short* lT = lds + 4 * kOperandElems;   // PmT / dST round-trip [key][q]

  const int bh = blockIdx.x;
  const int kt = blockIdx.y;
  const long long base =
      ((long long)(bh / H) * S) * rs + (long long)(bh % H) * D128;
  const long long obase =
      ((long long)(bh / H) * S) * ors + (long long)(bh % H) * D128;
  const long long gbase =
      ((long long)(bh / H) * S) * grs + (long long)(bh % H) * D128;
  int len = S;
  if constexpr (VARLEN) {
    len = clamped_len(seqlens, bh / H, S);
    if (kt * BKV >= len) {  // block-uniform: the whole key tile is padding
      zero_tile128(dK + gbase + (long long)kt * BKV * grs, grs, threadIdx.x);
      zero_tile128(dV + gbase + (long long)kt * BKV * grs, grs, threadIdx.x);
      return;
    }
  }
  const unsigned seed = seed_p ? (unsigned)(*seed_p) : 0u;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;  // owns keys [wave*16, +16)

  const FragLane fl(lane);
  const TrLane tr(lane);
  const unsigned lQ_addr = lds_addr(lQ), ldO_addr = lds_addr(ldO);
  const float qscale = rsqrtf((float)D128);

  bf16x8 kfr[4], vfr[4];
  {
    const int krow = kt * BKV + wave * 16 + fl.frag_row;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      kfr[ks] = *(const bf16x8*)(K + base + (long long)krow * rs + ks * 32 +
                                 fl.frag_k);
      vfr[ks] = *(const bf16x8*)(V + base + (long long)krow * rs + ks * 32 +
                                 fl.frag_k);
    }
  }

  f32x4 dv[8], dk[8];
#pragma unroll
  for (int df = 0; df < 8; ++df) {
    dv[df] = {0.f, 0.f, 0.f, 0.f};
    dk[df] = {0.f, 0.f, 0.f, 0.f};
  }

  auto stage_q = [&](int buf, int it) {
    stage_tile128(lQ + buf * kOperandElems,
                  Q + base + (long long)it * BQ * rs, rs, tid);
    stage_tile128(ldO + buf * kOperandElems,
                  dO + obase + (long long)it * BQ * ors, ors, tid);
  };

  // VARLEN: Q tiles beyond the length contribute nothing
  const int ntiles = VARLEN ? (len + BQ - 1) / BQ : S / BQ;
  // CAUSAL: Q tiles before kt see none of these keys; kt < ntiles here
  const int it0 = CAUSAL ? kt : 0;
  stage_q(0, it0);
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();

  for (int it = it0; it < ntiles; ++it) {
    const int cur = (it - it0) & 1;  // trips since the first tile
    if (it + 1 < ntiles) stage_q(cur ^ 1, it + 1);
    const short* lQc = lQ + cur * kOperandElems;
    const short* ldOc = ldO + cur * kOperandElems;

    // CAUSAL: the element mask runs in the diagonal tile and, under
    // VARLEN, in the tail tile (tile-uniform)
    const bool masked = CAUSAL && (it == it0 || (VARLEN && it == ntiles - 1));

    // S^T = K Q^T; dP^T = V dO^T
    f32x4 st[4], dpt[4];
#pragma unroll
    for (int qf = 0; qf < 4; ++qf) {
      st[qf] = {0.f, 0.f, 0.f, 0.f};
      dpt[qf] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        st[qf] = mfma_bf16(
            kfr[ks], lds_frag128(lQc, qf * 16 + fl.frag_row, ks, fl.frag_k),
            st[qf]);
        dpt[qf] = mfma_bf16(
            vfr[ks], lds_frag128(ldOc, qf * 16 + fl.frag_row, ks, fl.frag_k),
            dpt[qf]);
      }
    }

    // per-lane fixed q column: one LSE/Drow scalar per qf
#pragma unroll
    for (int qf = 0; qf < 4; ++qf) {
      const int q = it * BQ + qf * 16 + fl.c_col;
      const float lse = LSE[(long long)bh * S + q];
      const float di = Drow[(long long)bh * S + q];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kt * BKV + wave * 16 + fl.c_sub_row + r;
        float p = __expf(st[qf][r] * qscale - lse);
        const float keep = drop_keep(seed, bh, q, key, S, p24, inv1mp);
        float dst = p * (dpt[qf][r] * keep - di) * qscale;  // dS^T*scale
        if constexpr (CAUSAL) {
          // as below, plus the keys after the query; lse/di of a masked
          // pair may hold anything
          if (masked) {
            const bool valid = key <= q && q < len && key < len;
            p = valid ? p : 0.f;
            dst = valid ? dst : 0.f;
          }
        } else if constexpr (VARLEN) {
          // padded query or key: lse/di may hold anything, so select
          // zeros instead of multiplying by one
          const bool valid = q < len && key < len;
          p = valid ? p : 0.f;
          dst = valid ? dst : 0.f;
        }
        dpt[qf][r] = dst;
        lds_st16(lT, (wave * 16 + fl.c_sub_row + r) * BQ + qf * 16 + fl.c_col,
                 f2bf(p * keep));
      }
    }
    // dV += PmT @ dO: dO^T fragments by transposing reads (lT rows are
    // wave-private)
    const unsigned ldOa = ldO_addr + cur * (kOperandElems * 2);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 af = lds_frag(lT, wave * 16 + fl.frag_row,
                                 ks * 32 + fl.frag_k);
#pragma unroll
      for (int df = 0; df < 8; ++df)
        dv[df] = mfma_bf16(
            af,
            tr.frag(ldOa + (df >> 2) * (TILE_ELEMS * 2), ks * 32,
                    (df & 3) * 16),
            dv[df]);
    }
    __builtin_amdgcn_s_setprio(0);
    // overwrite lT with dS^T (own-wave rows; same-wave LDS ops are
    // processed in order, so the dV reads above see the old values)
#pragma unroll
    for (int qf = 0; qf < 4; ++qf)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        lds_st16(lT, (wave * 16 + fl.c_sub_row + r) * BQ + qf * 16 + fl.c_col,
                 f2bf(dpt[qf][r]));
    // dK += dST @ Q: Q^T fragments by transposing reads
    const unsigned lQa = lQ_addr + cur * (kOperandElems * 2);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 af = lds_frag(lT, wave * 16 + fl.frag_row,
                                 ks * 32 + fl.frag_k);
#pragma unroll
      for (int df = 0; df < 8; ++df)
        dk[df] = mfma_bf16(
            af,
            tr.frag(lQa + (df >> 2) * (TILE_ELEMS * 2), ks * 32,
                    (df & 3) * 16),
            dk[df]);
    }
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
  }

  const int krow0 = kt * BKV + wave * 16;
#pragma unroll
  for (int df = 0; df < 8; ++df)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long long off = gbase +
          (long long)(krow0 + fl.c_sub_row + r) * grs + df * 16 + fl.c_col;
      short gk = f2bf(dk[df][r]), gv = f2bf(dv[df][r]);
      if constexpr (VARLEN) {  // tail key tile: padded rows store zero
        const bool valid = krow0 + fl.c_sub_row + r < len;
        gk = valid ? gk : (short)0;
        gv = valid ? gv : (short)0;
      }
      dK[off] = gk;
      dV[off] = gv;
    }
}

// ----------------------------------------------------------- bwd dQ

template <bool VARLEN, bool CAUSAL>
__global__ __launch_bounds__(ATHREADS) void attn_d128_bwd_dq_k(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ V, const short* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ Drow,
    short* __restrict__ dQ, const long long* __restrict__ seed_p, int S,
    int H, int rs, int ors, int grs, unsigned p24, float inv1mp,
    const int* __restrict__ seqlens) {
  extern __shared__ __attribute__((aligned(16))) short lds[];
  short* lK = lds;                      // [2][key][128]
  short* lV = lds + 2 * kOperandElems;  // [2][key][128]
  short* lDS = lds + 4 * kOperandElems;

  const int bh = blockIdx.x;
  // CAUSAL: longest first, as in attn_d128_fwd_k
  const int qt = CAUSAL ? gridDim.y - 1 - blockIdx.y : blockIdx.y;
  const long long base =
      ((long long)(bh / H) * S) * rs + (long long)(bh % H) * D128;
  const long long obase =
      ((long long)(bh / H) * S) * ors + (long long)(bh % H) * D128;
  const long long gbase =
      ((long long)(bh / H) * S) * grs + (long long)(bh % H) * D128;
  int len = S;
  if constexpr (VARLEN) {
    len = clamped_len(seqlens, bh / H, S);
    if (qt * BQ >= len) {  // block-uniform: the whole Q tile is padding
      zero_tile128(dQ + gbase + (long long)qt * BQ * grs, grs, threadIdx.x);
      return;
    }
  }
  const unsigned seed = seed_p ? (unsigned)(*seed_p) : 0u;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;

  const FragLane fl(lane);
  const TrLane tr(lane);
  const unsigned lK_addr = lds_addr(lK);
  const float qscale = rsqrtf((float)D128);

  bf16x8 qf[4], dof[4];
  {
    const int qrow = qt * BQ + wave * 16 + fl.frag_row;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      qf[ks] = *(const bf16x8*)(Q + base + (long long)qrow * rs + ks * 32 +
                                fl.frag_k);
      dof[ks] = *(const bf16x8*)(dO + obase + (long long)qrow * ors +
                                 ks * 32 + fl.frag_k);
    }
  }
  float lse[4], di[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = qt * BQ + wave * 16 + fl.c_sub_row + r;
    lse[r] = LSE[(long long)bh * S + q];
    di[r] = Drow[(long long)bh * S + q];
  }

  f32x4 dq[8];
#pragma unroll
  for (int df = 0; df < 8; ++df) dq[df] = {0.f, 0.f, 0.f, 0.f};

  auto stage_kv = [&](int buf, int t) {
    stage_tile128(lK + buf * kOperandElems,
                  K + base + (long long)t * BKV * rs, rs, tid);
    stage_tile128(lV + buf * kOperandElems,
                  V + base + (long long)t * BKV * rs, rs, tid);
  };

  // CAUSAL: key tiles 0..qt, as in attn_d128_fwd_k
  const int ntiles =
      CAUSAL ? qt + 1 : VARLEN ? (len + BKV - 1) / BKV : S / BKV;
  stage_kv(0, 0);
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    const int cur = t & 1;
    if (t + 1 < ntiles) stage_kv(cur ^ 1, t + 1);
    const short* lKc = lK + cur * kOperandElems;
    const short* lVc = lV + cur * kOperandElems;

    const bool diag = CAUSAL && t == qt;  // carries the element mask

    f32x4 s_acc[4], dp[4];
#pragma unroll
    for (int kf = 0; kf < 4; ++kf) {
      s_acc[kf] = {0.f, 0.f, 0.f, 0.f};
      dp[kf] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        s_acc[kf] = mfma_bf16(
            qf[ks], lds_frag128(lKc, kf * 16 + fl.frag_row, ks, fl.frag_k),
            s_acc[kf]);
        dp[kf] = mfma_bf16(
            dof[ks], lds_frag128(lVc, kf * 16 + fl.frag_row, ks, fl.frag_k),
            dp[kf]);
      }
    }

#pragma unroll
    for (int kf = 0; kf < 4; ++kf)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = qt * BQ + wave * 16 + fl.c_sub_row + r;
        const int key = t * BKV + kf * 16 + fl.c_col;
        const float p = __expf(s_acc[kf][r] * qscale - lse[r]);
        const float keep = drop_keep(seed, bh, q, key, S, p24, inv1mp);
        float ds = p * (dp[kf][r] * keep - di[r]) * qscale;
        // padded query or key: select zero (lse/di may hold anything)
        if constexpr (CAUSAL) {
          // diagonal tile only: the tiles below it hold valid keys, and
          // a padded query spoils its own dQ row alone, zeroed below
          if (diag) ds = key <= q && q < len && key < len ? ds : 0.f;
        } else if constexpr (VARLEN) {
          ds = q < len && key < len ? ds : 0.f;
        }
        lds_st16(lDS,
                 (wave * 16 + fl.c_sub_row + r) * BKV + kf * 16 + fl.c_col,
                 f2bf(ds));
      }
    // dQ += dS @ K: K^T fragments by transposing reads (lDS rows are
    // wave-private)
    const unsigned lKa = lK_addr + cur * (kOperandElems * 2);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 af = lds_frag(lDS, wave * 16 + fl.frag_row,
                                 ks * 32 + fl.frag_k);
#pragma unroll
      for (int df = 0; df < 8; ++df)
        dq[df] = mfma_bf16(
            af,
            tr.frag(lKa + (df >> 2) * (TILE_ELEMS * 2), ks * 32,
                    (df & 3) * 16),
            dq[df]);
    }
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
  }

  const int qrow0 = qt * BQ + wave * 16;
#pragma unroll
  for (int df = 0; df < 8; ++df)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qrow = qrow0 + fl.c_sub_row + r;
      short g = f2bf(dq[df][r]);
      if constexpr (VARLEN) g = qrow < len ? g : (short)0;
      dQ[gbase + (long long)qrow * grs + df * 16 + fl.c_col] = g;
    }
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// One workgroup per (bh, 64-row tile); the causal kernels reverse
// blockIdx.y where that issues the longest first.
void launch_attn_d128_fwd(const short* Q, const short* K, const short* V,
                          short* O, float* LSE, const long long* seed,
                          int BH, int S, int H, int rs, int ors,
                          float dropout_p, const int* seqlens, bool causal,
                          hipStream_t stream) {
  const unsigned p24 = (unsigned)(dropout_p * 16777216.0f);
  const float inv1mp = dropout_p > 0.f ? 1.f / (1.f - dropout_p) : 1.f;
  const dim3 grid(BH, S / BQ);
#define SPARKDL_D128_FWD(VL, CA)                                          \
  launch_d128<attn_d128_fwd_k<VL, CA>>(grid, stream, Q, K, V, O, LSE,     \
                                       seed, S, H, rs, ors, p24, inv1mp,  \
                                       seqlens)
  if (seqlens) {
    if (causal) SPARKDL_D128_FWD(true, true);
    else SPARKDL_D128_FWD(true, false);
  } else {
    if (causal) SPARKDL_D128_FWD(false, true);
    else SPARKDL_D128_FWD(false, false);
  }
#undef SPARKDL_D128_FWD
}

void launch_attn_d128_bwd(const short* Q, const short* K, const short* V,
                          const short* dO, const float* LSE,
                          const float* Drow, short* dQ, short* dK,
                          short* dV, const long long* seed, int BH, int S,
                          int H, int rs, int ors, int grs, float dropout_p,
                          const int* seqlens, bool causal,
                          hipStream_t stream) {
  const unsigned p24 = (unsigned)(dropout_p * 16777216.0f);
  const float inv1mp = dropout_p > 0.f ? 1.f / (1.f - dropout_p) : 1.f;
  const dim3 grid(BH, S / BQ);
#define SPARKDL_D128_BWD(VL, CA)                                           \
  do {                                                                     \
    launch_d128<attn_d128_bwd_dkdv_k<VL, CA>>(                             \
        grid, stream, Q, K, V, dO, LSE, Drow, dK, dV, seed, S, H, rs, ors, \
        grs, p24, inv1mp, seqlens);                                        \
    launch_d128<attn_d128_bwd_dq_k<VL, CA>>(                               \
        grid, stream, Q, K, V, dO, LSE, Drow, dQ, seed, S, H, rs, ors,     \
        grs, p24, inv1mp, seqlens);                                        \
  } while (0)
  if (seqlens) {
    if (causal) SPARKDL_D128_BWD(true, true);
    else SPARKDL_D128_BWD(true, false);
  } else {
    if (causal) SPARKDL_D128_BWD(false, true);
    else SPARKDL_D128_BWD(false, false);
  }
#undef SPARKDL_D128_BWD
}
