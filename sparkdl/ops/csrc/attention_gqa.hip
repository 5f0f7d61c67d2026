// Grouped-query flash attention (forward + backward) for 128-wide heads,
// bf16, fp32 accumulation:
//
//   O[b, hq] = softmax(Q[b, hq] K[b, hq / G]^T / sqrt(128)) V[b, hq / G]
//
// Hq query heads share Hkv key/value heads in groups of G = Hq / Hkv
// (Hkv = 1: multi-query attention; G = 1: plain multi-head attention).
// Same contract as attention_d128.hip (S % 64 == 0, strided rows,
// right-padded `seqlens` read on the device and indexed by b, the causal
// triangle, LSE, fp32 score scale 2^-3.5 applied the same way in all
// three kernels; template <VARLEN, CAUSAL>) and its tile primitives
// (attention_d128_tile.hip.h). Q, O, dO, dQ, LSE and Drow are indexed by
// the query head b*Hq + hq; K, V, dK and dV by hkv = hq / G through a
// view of their own (batch, head and row strides). K/V are read in
// place: nothing here, launcher included, expands them in memory.
// The dropout hash is (seed, b*Hq + hq, q*S + k): with one seed a call
// drops exactly what the multi-head kernels drop on expanded K/V.
//
// dK/dV: one workgroup per (b, hkv, key tile). It loads its K and V
// fragments once and keeps the dk[8]/dv[8] fp32 accumulators in
// registers across all G query heads of the group and all their Q
// tiles, so the group's sum happens in registers: each dK/dV row is
// written once, as bf16, after a single rounding, with no atomics, no
// [B,Hq,S,128] intermediate and no second pass. (head in group, Q tile)
// is flattened into one trip counter, so the double-buffered Q/dO
// staging prefetches the next head's first tile during the last tile of
// the current head and never drains: one wait and one barrier per trip.
// Under CAUSAL each head's trips start at the key tile's diagonal;
// under VARLEN they stop at the row's length, the same for every head
// of the group. Work per workgroup grows with G while the grid shrinks
// to B*Hkv*S/64 workgroups: at Hkv = 1 that is B*S/64 of them, which
// fills 256 CUs x 2 only when B*S >= 32768.
//
// Forward and dQ: one workgroup per (b, hq, Q tile), one head each,
// reading K/V of head hq / G. blockIdx.x = b*Hq + hq is the fastest
// launch dimension, so the G heads of a group are neighbours in launch
// order, walk the same K/V tiles at about the same time and share them
// in L2. Causal launches reverse blockIdx.y: longest tiles first.
// Running several heads of a group in one workgroup against one staged
// K/V tile was not built: the forward already holds 32 accumulator and
// 16 Q-fragment registers per head next to 16 score registers, and a
// second head's set would put two workgroups per CU at risk; whether it
// would be faster is not measured.
//
// LDS per workgroup: 72 KiB in each kernel (two workgroups per CU), laid
// out as in attention_d128.hip. The all-padding early exit is
// block-uniform and taken before any barrier; masked p / dS are zero by
// selection; no atomics, no memset, no host sync: graph-capturable, and
// the same bits on every run.

// device code of this file is generated without packed fp32 instructions
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

#include "attention_d128_tile.hip.h"

namespace {

// Where head h of batch row b starts in a tensor, and how far apart its
// sequence rows are (elements). Packed [B,S,Hq+2Hkv,128]: bs = S*rs,
// hs = 128, rs = (Hq+2Hkv)*128; plain [B*H,S,128]: bs = H*S*128,
// hs = S*128, rs = 128.
struct HeadView {
  long long bs, hs;
  int rs;
  __device__ __forceinline__ long long at(int b, int h) const {
    return b * bs + h * hs;
  }
};

// ------------------------------------------------------------- fwd

template <bool VARLEN, bool CAUSAL>
__global__ __launch_bounds__(ATHREADS) void attn_gqa_fwd_k(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ V, short* __restrict__ O,
    float* __restrict__ LSE, const long long* __restrict__ seed_p, int S,
    int Hq, int G, HeadView qv, HeadView kvv, HeadView ov, unsigned p24,
    float inv1mp, const int* __restrict__ seqlens) {
  extern __shared__ __attribute__((aligned(16))) short lds[];
  short* lK = lds;                      // [2][key][128], double-buffered
  short* lV = lds + 2 * kOperandElems;  // [2][key][128]
  short* lP = lds + 4 * kOperandElems;  // [q][key]

  const int bh = blockIdx.x;  // b*Hq + hq: a group's heads are adjacent
  const int b = bh / Hq, hq = bh % Hq;
  // CAUSAL: tile qt runs qt+1 trips, the longest are issued first
  const int qt = CAUSAL ? gridDim.y - 1 - blockIdx.y : blockIdx.y;
  const int rs = qv.rs, krs = kvv.rs, ors = ov.rs;
  const long long base = qv.at(b, hq);
  const long long kbase = kvv.at(b, hq / G);  // the group's shared head
  const long long obase = ov.at(b, hq);
  int len = S;
  if constexpr (VARLEN) {
    len = clamped_len(seqlens, b, S);
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
                  K + kbase + (long long)t * BKV * krs, krs, tid);
    stage_tile128(lV + buf * kOperandElems,
                  V + kbase + (long long)t * BKV * krs, krs, tid);
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

// Two waves per SIMD asked of the compiler: without the bound the
// <VARLEN, CAUSAL> instantiation takes 192 VGPRs + 68 AGPRs = 260 and
// one workgroup per CU; with it every instantiation is allocated 213 to
// 224 unified registers, no AGPR copies, no scratch.
template <bool VARLEN, bool CAUSAL>
__global__ __launch_bounds__(ATHREADS, 2) void attn_gqa_bwd_dkdv_k(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ V, const short* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ Drow,
    short* __restrict__ dK, short* __restrict__ dV,
    const long long* __restrict__ seed_p, int S, int Hq, int G,
    HeadView qv, HeadView kvv, HeadView ov, unsigned p24, float inv1mp,
    const int* __restrict__ seqlens) {
  extern __shared__ __attribute__((aligned(16))) short lds[];
  short* lQ = lds;                       // [2][q][128]
  short* ldO = lds + 2 * kOperandElems;  // [2][q][128]
  short* lT = lds + 4 * kOperandElems;   // PmT / dST round-trip [key][q]

  const int Hkv = Hq / G;
  const int b = blockIdx.x / Hkv, hkv = blockIdx.x % Hkv;
  const int kt = blockIdx.y;
  const int rs = qv.rs, krs = kvv.rs, ors = ov.rs;
  const long long kbase = kvv.at(b, hkv);  // K, V and their gradients
  int len = S;
  if constexpr (VARLEN) {
    len = clamped_len(seqlens, b, S);
    if (kt * BKV >= len) {  // block-uniform: the whole key tile is padding
      zero_tile128(dK + kbase + (long long)kt * BKV * krs, krs, threadIdx.x);
      zero_tile128(dV + kbase + (long long)kt * BKV * krs, krs, threadIdx.x);
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

  bf16x8 kfr[4], vfr[4];  // loaded once for the whole group
  {
    const int krow = kt * BKV + wave * 16 + fl.frag_row;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      kfr[ks] = *(const bf16x8*)(K + kbase + (long long)krow * krs +
                                 ks * 32 + fl.frag_k);
      vfr[ks] = *(const bf16x8*)(V + kbase + (long long)krow * krs +
                                 ks * 32 + fl.frag_k);
    }
  }

  f32x4 dv[8], dk[8];  // the group's sum, over heads and Q tiles
#pragma unroll
  for (int df = 0; df < 8; ++df) {
    dv[df] = {0.f, 0.f, 0.f, 0.f};
    dk[df] = {0.f, 0.f, 0.f, 0.f};
  }

  const int hq0 = hkv * G;  // first query head of the group
  auto stage_q = [&](int buf, int g, int it) {
    stage_tile128(lQ + buf * kOperandElems,
                  Q + qv.at(b, hq0 + g) + (long long)it * BQ * rs, rs, tid);
    stage_tile128(ldO + buf * kOperandElems,
                  dO + ov.at(b, hq0 + g) + (long long)it * BQ * ors, ors,
                  tid);
  };

  // VARLEN: Q tiles beyond the length contribute nothing
  const int ntiles = VARLEN ? (len + BQ - 1) / BQ : S / BQ;
  // CAUSAL: Q tiles before kt see none of these keys; kt < ntiles here
  const int it0 = CAUSAL ? kt : 0;
  // one trip counter over (head in group, Q tile): head g runs Q tiles
  // it0 .. ntiles-1, then head g+1 starts at it0 again
  const int trips = G * (ntiles - it0);
  stage_q(0, 0, it0);
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();

  int g = 0, it = it0;
  for (int trip = 0; trip < trips; ++trip) {
    const int cur = trip & 1;
    // the trip after this one: the next Q tile, or the next head's first
    const bool last_it = it + 1 == ntiles;
    const int g_nx = last_it ? g + 1 : g, it_nx = last_it ? it0 : it + 1;
    if (trip + 1 < trips) stage_q(cur ^ 1, g_nx, it_nx);
    const short* lQc = lQ + cur * kOperandElems;
    const short* ldOc = ldO + cur * kOperandElems;
    const int bh = b * Hq + hq0 + g;  // LSE, Drow and the dropout hash

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
    g = g_nx;
    it = it_nx;
  }

  // the only rounding of the group's sum
  const int krow0 = kt * BKV + wave * 16;
#pragma unroll
  for (int df = 0; df < 8; ++df)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long long off = kbase +
          (long long)(krow0 + fl.c_sub_row + r) * krs + df * 16 + fl.c_col;
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
__global__ __launch_bounds__(ATHREADS) void attn_gqa_bwd_dq_k(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ V, const short* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ Drow,
    short* __restrict__ dQ, const long long* __restrict__ seed_p, int S,
    int Hq, int G, HeadView qv, HeadView kvv, HeadView ov, unsigned p24,
    float inv1mp, const int* __restrict__ seqlens) {
  extern __shared__ __attribute__((aligned(16))) short lds[];
  short* lK = lds;                      // [2][key][128]
  short* lV = lds + 2 * kOperandElems;  // [2][key][128]
  short* lDS = lds + 4 * kOperandElems;

  const int bh = blockIdx.x;  // b*Hq + hq, as in attn_gqa_fwd_k
  const int b = bh / Hq, hq = bh % Hq;
  // CAUSAL: longest first, as in attn_gqa_fwd_k
  const int qt = CAUSAL ? gridDim.y - 1 - blockIdx.y : blockIdx.y;
  const int rs = qv.rs, krs = kvv.rs, ors = ov.rs;
  const long long base = qv.at(b, hq);  // Q and dQ
  const long long kbase = kvv.at(b, hq / G);
  const long long obase = ov.at(b, hq);
  int len = S;
  if constexpr (VARLEN) {
    len = clamped_len(seqlens, b, S);
    if (qt * BQ >= len) {  // block-uniform: the whole Q tile is padding
      zero_tile128(dQ + base + (long long)qt * BQ * rs, rs, threadIdx.x);
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
                  K + kbase + (long long)t * BKV * krs, krs, tid);
    stage_tile128(lV + buf * kOperandElems,
                  V + kbase + (long long)t * BKV * krs, krs, tid);
  };

  // CAUSAL: key tiles 0..qt, as in attn_gqa_fwd_k
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
      dQ[base + (long long)qrow * rs + df * 16 + fl.c_col] = g;
    }
}

// The three views of one call. packed: Q, K, V are head ranges of one
// [B,S,Hq+2Hkv,128] buffer and O is [B,S,Hq*128]; otherwise plain
// [B*Hq,S,128] / [B*Hkv,S,128] tensors.
struct GqaViews {
  HeadView q, kv, o;
  GqaViews(int S, int Hq, int Hkv, bool packed) {
    const long long row = (long long)(Hq + 2 * Hkv) * D128;
    if (packed) {
      q = kv = {S * row, D128, (int)row};
      o = {(long long)S * Hq * D128, D128, Hq * D128};
    } else {
      q = o = {(long long)Hq * S * D128, (long long)S * D128, D128};
      kv = {(long long)Hkv * S * D128, (long long)S * D128, D128};
    }
  }
};

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

void launch_attn_gqa_fwd(const short* Q, const short* K, const short* V,
                         short* O, float* LSE, const long long* seed, int B,
                         int S, int Hq, int Hkv, bool packed,
                         float dropout_p, const int* seqlens, bool causal,
                         hipStream_t stream) {
  const unsigned p24 = (unsigned)(dropout_p * 16777216.0f);
  const float inv1mp = dropout_p > 0.f ? 1.f / (1.f - dropout_p) : 1.f;
  const GqaViews vw(S, Hq, Hkv, packed);
  const dim3 grid(B * Hq, S / BQ);
#define SPARKDL_GQA_FWD(VL, CA)                                            \
  launch_d128<attn_gqa_fwd_k<VL, CA>>(grid, stream, Q, K, V, O, LSE, seed, \
                                      S, Hq, Hq / Hkv, vw.q, vw.kv, vw.o,  \
                                      p24, inv1mp, seqlens)
  if (seqlens) {
    if (causal) SPARKDL_GQA_FWD(true, true);
    else SPARKDL_GQA_FWD(true, false);
  } else {
    if (causal) SPARKDL_GQA_FWD(false, true);
    else SPARKDL_GQA_FWD(false, false);
  }
#undef SPARKDL_GQA_FWD
}

void launch_attn_gqa_bwd(const short* Q, const short* K, const short* V,
                         const short* dO, const float* LSE,
                         const float* Drow, short* dQ, short* dK, short* dV,
                         const long long* seed, int B, int S, int Hq,
                         int Hkv, bool packed, float dropout_p,
                         const int* seqlens, bool causal,
                         hipStream_t stream) {
  const unsigned p24 = (unsigned)(dropout_p * 16777216.0f);
  const float inv1mp = dropout_p > 0.f ? 1.f / (1.f - dropout_p) : 1.f;
  const GqaViews vw(S, Hq, Hkv, packed);
  // dK/dV: one workgroup per shared head and key tile; dQ: per query head
  const dim3 kv_grid(B * Hkv, S / BKV), q_grid(B * Hq, S / BQ);
#define SPARKDL_GQA_BWD(VL, CA)                                             \
  do {                                                                      \
    launch_d128<attn_gqa_bwd_dkdv_k<VL, CA>>(                               \
        kv_grid, stream, Q, K, V, dO, LSE, Drow, dK, dV, seed, S, Hq,       \
        Hq / Hkv, vw.q, vw.kv, vw.o, p24, inv1mp, seqlens);                 \
    launch_d128<attn_gqa_bwd_dq_k<VL, CA>>(                                 \
        q_grid, stream, Q, K, V, dO, LSE, Drow, dQ, seed, S, Hq, Hq / Hkv,  \
        vw.q, vw.kv, vw.o, p24, inv1mp, seqlens);                           \
  } while (0)
  if (seqlens) {
    if (causal) SPARKDL_GQA_BWD(true, true);
    else SPARKDL_GQA_BWD(true, false);
  } else {
    if (causal) SPARKDL_GQA_BWD(false, true);
    else SPARKDL_GQA_BWD(false, false);
  }
#undef SPARKDL_GQA_BWD
}
