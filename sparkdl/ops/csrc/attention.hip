// Hand-written flash attention (forward + backward) for D=64 heads,
// bf16, fp32 accumulation — SURVEY.md §2.2 N6 "attention GEMMs";
// replaces torch SDPA (aotriton, Triton-compiled) on the BERT hot path
// (round-1 profile: ~22% of the training step).
//
//   O = softmax(Q K^T / sqrt(D)) V     S % 64 == 0, head dim 64
//
// I/O layouts (zero-copy around the BERT block): the kernels read rows
// through an element stride, so they consume the packed qkv Linear
// output [B,S,3,H,64] directly (rs = 3*H*64) and write O as [B,S,H*64]
// (ors = H*64); the backward emits the packed dqkv the qkv Linear's
// backward consumes. Plain [BH,S,64] tensors use stride 64.
//
// Transposed operands (V^T for the fwd PV product; Q^T/dO^T for dK/dV;
// K^T for dQ) are built ONCE per call by attn_pretranspose_k into
// [BH,64,S] scratch — round 2 profiling showed the original in-kernel
// scalar-scatter transposes re-did the same transpose once per tile
// PAIR. With every operand linear, all staging is global_load_lds and
// each kernel double-buffers its tiles: stage(t+1) issues before
// compute(t), one vmcnt(0)+barrier per tile (the guide's minimum
// 2-phase pattern).
//
// All matrix products use the one mfma_f32_16x16x32_bf16 fragment path
// of mfma_tile.hip.h (operands K-major):
//   fwd:   S   = mfma(Q, K)        P->LDS   O  = mfma(P_lds, Vt)
//   dK/dV: S^T = mfma(K, Q)        dP^T = mfma(V, dO)
//          dV  = mfma(PmT_lds, dOt)  dK = mfma(dST_lds, Qt)
//   dQ:    S   = mfma(Q, K)        dP = mfma(dO, V)
//          dQ  = mfma(dS_lds, Kt)
//
// The forward stores LSE[q] = m + log(l); the backward recomputes
// P = exp(S - LSE) tile by tile, with D_i = rowsum(dO o O) precomputed
// by the host. Dropout (p>0): counter-based hash of (seed, bh, q*S+k)
// regenerated identically in forward and backward; the seed lives in
// DEVICE memory so the op is hipGraph-capture safe.
//
// Variable-length batches (template <bool VARLEN>, chosen by a non-null
// `seqlens`): rows are right-padded, seqlens[bh / H] (DEVICE int32,
// clamped into [0,S]) is the number of valid tokens. Only keys < len
// are attended to; query rows >= len give exactly zero O and dQ and
// feed nothing into dK/dV; dK/dV rows >= len are exactly zero.
//   * A block whose whole tile is padding stores a zero tile (fwd: and
//     LSE = 0) and returns — a block-uniform branch taken before any
//     barrier or global_load_lds. The others loop over ceil(len/64)
//     tiles instead of S/64, so a padded row costs ~len^2, not S^2.
//   * In the tail tile, padded keys are taken out of the running max
//     and get p = 0 by SELECTION (cond ? x : 0, never x * 0: LSE/Drow
//     of padded rows may hold anything). Every processed tile holds at
//     least one valid key, so the running max stays finite.
//   * Tail-tile staging and the pre-transposes still cover full tiles
//     (in bounds: S % 64 == 0). A zero P does not shield an MFMA from
//     a non-finite operand, so padded rows must hold FINITE values.
//   * Dropout keeps hashing (seed, bh, q*S+k): a valid (q,k) pair gets
//     the decision of the unmasked call with the same seed.
// The VARLEN=false instantiations are the fixed-length kernels,
// instruction for instruction.
//
// LDS tiles are [row][64] bf16 with the st_16x32 XOR swizzle on both
// sides (pre-permuted global_load_lds sources + swizzled ds accesses):
// without it the 16-lane column reads are 16-way bank conflicts.
//
// Per-wave layout (4 waves, 256 threads): wave w owns 16 rows of the
// 64-row output tile. P/dS LDS round-trips touch only the owning
// wave's rows, so they need no barriers (same-wave LDS ops complete in
// order).

#include "mfma_tile.hip.h"
#include "kernels.h"

namespace {

constexpr int D = 64;
constexpr int BQ = 64;
constexpr int BKV = 64;
constexpr int ATHREADS = 256;
constexpr int TILE_ELEMS = 64 * 64;

__device__ __forceinline__ float drop_keep(unsigned seed,
                                           unsigned long long bh,
                                           int q, int k, int S,
                                           unsigned p24, float inv1mp) {
  if (p24 == 0) return 1.f;
  const unsigned idx = (unsigned)(bh * 0x9e3779b9u) ^
                       (unsigned)(q * S + k);
  return (drop_hash(seed, idx) & 0xffffffu) >= p24 ? inv1mp : 0.f;
}

// Stage one [64][64] bf16 tile into swizzled LDS (2 sweeps x 256
// threads x 16 B). Source rows are `stride` elements apart.
__device__ __forceinline__ void stage_tile64(short* dst, const short* g,
                                             long long stride, int tid) {
  stage_tile<ATHREADS, 2>(dst, g, stride, tid);
}

// One operand fragment from global memory, multiplied by `scale` and
// rounded back to bf16 (Q enters every product pre-scaled by 1/sqrt(D)).
__device__ __forceinline__ bf16x8 load_frag_scaled(const short* p,
                                                   float scale) {
  bf16x8 raw = *(const bf16x8*)p;
#pragma unroll
  for (int j = 0; j < 8; ++j) raw[j] = f2bf(bf2f(raw[j]) * scale);
  return raw;
}

// Swizzled 2 B store of element `elem` of a [64][64] LDS tile.
__device__ __forceinline__ void lds_st16(short* base, int elem,
                                         short v) {
  *(short*)((char*)base + tile_swz128(elem * 2)) = v;
}

// Variable-length batches (VARLEN): a block whose whole tile lies in the
// padding stores a zero [64][64] tile (rows `stride` elements apart) and
// returns. 256 threads x 2 x 16 B.
__device__ __forceinline__ void zero_tile(short* g, long long stride,
                                          int tid) {
  const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  short* p = g + (long long)(tid / 4) * stride + (tid % 4) * 16;
  *(bf16x8*)p = z;
  *(bf16x8*)(p + 8) = z;
}

// Length of batch row `b`, clamped into [0, S] so that no entry can
// index outside the sequence.
__device__ __forceinline__ int clamped_len(const int* seqlens, int b,
                                           int S) {
  return min(max(seqlens[b], 0), S);
}

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

// ------------------------------------------------------------- fwd

template <bool VARLEN>
__global__ __launch_bounds__(ATHREADS) void attn_fwd_k(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ VT, short* __restrict__ O,
    float* __restrict__ LSE, const long long* __restrict__ seed_p,
    int S, int H, int rs, int ors, unsigned p24, float inv1mp,
    const int* __restrict__ seqlens) {
  __shared__ short lK[2][TILE_ELEMS];   // [key][d], double-buffered
  __shared__ short lVt[2][TILE_ELEMS];  // [d][key]
  __shared__ short lP[TILE_ELEMS];

  const int bh = blockIdx.x;
  const int qt = blockIdx.y;
  const long long base =
      ((long long)(bh / H) * S) * rs + (long long)(bh % H) * 64;
  const long long obase =
      ((long long)(bh / H) * S) * ors + (long long)(bh % H) * 64;
  const short* vtb = VT + (long long)bh * 64 * S;
  int len = S;
  if constexpr (VARLEN) {
    len = clamped_len(seqlens, bh / H, S);
    if (qt * BQ >= len) {  // block-uniform: the whole Q tile is padding
      zero_tile(O + obase + (long long)qt * BQ * ors, ors, threadIdx.x);
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

  const float qscale = rsqrtf((float)D);
  bf16x8 qf[2];
  {
    const int qrow = qt * BQ + wave * 16 + fl.frag_row;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      qf[ks] = load_frag_scaled(
          Q + base + (long long)qrow * rs + ks * 32 + fl.frag_k, qscale);
    }
  }

  float m_run[4], l_run[4];
  f32x4 o_acc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m_run[r] = -1e30f;
    l_run[r] = 0.f;
  }
#pragma unroll
  for (int df = 0; df < 4; ++df) o_acc[df] = {0.f, 0.f, 0.f, 0.f};

  // VARLEN: only the tiles that hold a valid key (each holds >= 1)
  const int ntiles = VARLEN ? (len + BKV - 1) / BKV : S / BKV;
  stage_tile64(lK[0], K + base, rs, tid);
  stage_tile64(lVt[0], vtb, S, tid);
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    const int cur = t & 1;
    if (t + 1 < ntiles) {  // prefetch next K/Vt under this tile's math
      stage_tile64(lK[cur ^ 1], K + base + (long long)(t + 1) * BKV * rs,
                   rs, tid);
      stage_tile64(lVt[cur ^ 1], vtb + (t + 1) * BKV, S, tid);
    }

    f32x4 s_acc[4];
#pragma unroll
    for (int kf = 0; kf < 4; ++kf) {
      s_acc[kf] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 bf = lds_frag(lK[cur], kf * 16 + fl.frag_row,
                                   ks * 32 + fl.frag_k);
        // the builtin, not mfma_bf16: through the wrapper the compiler
        // schedules the fixed-length instantiation differently
        s_acc[kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            qf[ks], bf, s_acc[kf], 0, 0, 0);
      }
    }

    // VARLEN: keys of this tile at or beyond kvalid are padding (only
    // in the tail tile); they leave the running max and get p = 0
    const int kvalid = VARLEN ? len - t * BKV : BKV;
    if constexpr (VARLEN) {
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
        if constexpr (VARLEN) p = kf * 16 + fl.c_col < kvalid ? p : 0.f;
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
      for (int df = 0; df < 4; ++df) o_acc[df][r] *= scale;
    }

#pragma unroll
    for (int kf = 0; kf < 4; ++kf)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        lds_st16(lP, (wave * 16 + fl.c_sub_row + r) * BKV + kf * 16 + fl.c_col,
                 f2bf(s_acc[kf][r]));
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int df = 0; df < 4; ++df) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 af = lds_frag(lP, wave * 16 + fl.frag_row,
                                   ks * 32 + fl.frag_k);
        const bf16x8 bf = lds_frag(lVt[cur], df * 16 + fl.frag_row,
                                   ks * 32 + fl.frag_k);
        o_acc[df] = mfma_bf16(af, bf, o_acc[df]);
      }
    }
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_s_waitcnt(0);  // next tile's staging has landed
    __syncthreads();
  }

  const int qrow0 = qt * BQ + wave * 16;
#pragma unroll
  for (int df = 0; df < 4; ++df)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qrow = qrow0 + fl.c_sub_row + r;
      if constexpr (VARLEN)  // tail Q tile: padded rows store zero
        O[obase + (long long)qrow * ors + df * 16 + fl.c_col] =
            qrow < len ? f2bf(o_acc[df][r] / l_run[r]) : (short)0;
      else
        O[obase + (long long)qrow * ors + df * 16 + fl.c_col] =
            f2bf(o_acc[df][r] / l_run[r]);
    }
  if (LSE && fl.c_col == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if constexpr (VARLEN)
        LSE[(long long)bh * S + qrow0 + fl.c_sub_row + r] =
            qrow0 + fl.c_sub_row + r < len ? m_run[r] + __logf(l_run[r])
                                        : 0.f;
      else
        LSE[(long long)bh * S + qrow0 + fl.c_sub_row + r] =
            m_run[r] + __logf(l_run[r]);
  }
}

// --------------------------------------------------------- bwd dK/dV

template <bool VARLEN>
__global__ __launch_bounds__(ATHREADS) void attn_bwd_dkdv_k(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ V, const short* __restrict__ dO,
    const short* __restrict__ QT, const short* __restrict__ DOT,
    const float* __restrict__ LSE, const float* __restrict__ Drow,
    short* __restrict__ dK, short* __restrict__ dV,
    const long long* __restrict__ seed_p, int S, int H, int rs, int ors,
    int grs, unsigned p24, float inv1mp,
    const int* __restrict__ seqlens) {
  __shared__ short lQ[2][TILE_ELEMS];    // [q][d]
  __shared__ short lQt[2][TILE_ELEMS];   // [d][q]
  __shared__ short ldO[2][TILE_ELEMS];   // [q][d]
  __shared__ short ldOt[2][TILE_ELEMS];  // [d][q]
  __shared__ short lT[TILE_ELEMS];       // PmT / dST round-trip

  const int bh = blockIdx.x;
  const int kt = blockIdx.y;
  const long long base =
      ((long long)(bh / H) * S) * rs + (long long)(bh % H) * 64;
  const long long obase =
      ((long long)(bh / H) * S) * ors + (long long)(bh % H) * 64;
  const long long gbase =
      ((long long)(bh / H) * S) * grs + (long long)(bh % H) * 64;
  const short* qtb = QT + (long long)bh * 64 * S;
  const short* dtb = DOT + (long long)bh * 64 * S;
  int len = S;
  if constexpr (VARLEN) {
    len = clamped_len(seqlens, bh / H, S);
    if (kt * BKV >= len) {  // block-uniform: the whole key tile is padding
      zero_tile(dK + gbase + (long long)kt * BKV * grs, grs, threadIdx.x);
      zero_tile(dV + gbase + (long long)kt * BKV * grs, grs, threadIdx.x);
      return;
    }
  }
  const unsigned seed = seed_p ? (unsigned)(*seed_p) : 0u;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;  // owns keys [wave*16, +16)

  // FragLane's four coordinates as plain locals: through the struct the
  // compiler schedules the VARLEN instantiation differently
  const int frag_row = lane % 16;
  const int frag_k = (lane / 16) * 8;
  const int c_sub_row = (lane / 16) * 4;
  const int c_col = lane % 16;
  const float qscale = rsqrtf((float)D);

  bf16x8 kfr[2], vfr[2];
  {
    const int krow = kt * BKV + wave * 16 + frag_row;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      kfr[ks] = *(const bf16x8*)(K + base + (long long)krow * rs +
                                 ks * 32 + frag_k);
      vfr[ks] = *(const bf16x8*)(V + base + (long long)krow * rs +
                                 ks * 32 + frag_k);
    }
  }

  f32x4 dv[4], dk[4];
#pragma unroll
  for (int df = 0; df < 4; ++df) {
    dv[df] = {0.f, 0.f, 0.f, 0.f};
    dk[df] = {0.f, 0.f, 0.f, 0.f};
  }

  auto stage_q = [&](int buf, int it) {
    stage_tile64(lQ[buf], Q + base + (long long)it * BQ * rs, rs, tid);
    stage_tile64(lQt[buf], qtb + it * BQ, S, tid);
    stage_tile64(ldO[buf], dO + obase + (long long)it * BQ * ors, ors,
                 tid);
    stage_tile64(ldOt[buf], dtb + it * BQ, S, tid);
  };

  // VARLEN: Q tiles beyond the length contribute nothing
  const int ntiles = VARLEN ? (len + BQ - 1) / BQ : S / BQ;
  stage_q(0, 0);
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();

  for (int it = 0; it < ntiles; ++it) {
    const int cur = it & 1;
    if (it + 1 < ntiles) stage_q(cur ^ 1, it + 1);

    // S^T = K Q^T (scaled); dP^T = V dO^T
    f32x4 st[4], dpt[4];
#pragma unroll
    for (int qf = 0; qf < 4; ++qf) {
      st[qf] = {0.f, 0.f, 0.f, 0.f};
      dpt[qf] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 bq = lds_frag(lQ[cur], qf * 16 + frag_row,
                                   ks * 32 + frag_k);
        const bf16x8 bd = lds_frag(ldO[cur], qf * 16 + frag_row,
                                   ks * 32 + frag_k);
        st[qf] = mfma_bf16(kfr[ks], bq, st[qf]);
        dpt[qf] = mfma_bf16(vfr[ks], bd, dpt[qf]);
      }
    }

    // per-lane fixed q column: one LSE/Drow scalar per qf
#pragma unroll
    for (int qf = 0; qf < 4; ++qf) {
      const int q = it * BQ + qf * 16 + c_col;
      const float lse = LSE[(long long)bh * S + q];
      const float di = Drow[(long long)bh * S + q];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kt * BKV + wave * 16 + c_sub_row + r;
        float p = __expf(st[qf][r] * qscale - lse);
        const float keep = drop_keep(seed, bh, q, key, S, p24, inv1mp);
        float dst = p * (dpt[qf][r] * keep - di) * qscale;  // dS^T*sc
        if constexpr (VARLEN) {
          // padded query or key: lse/di may hold anything, so select
          // zeros instead of multiplying by one
          const bool valid = q < len && key < len;
          p = valid ? p : 0.f;
          dst = valid ? dst : 0.f;
        }
        dpt[qf][r] = dst;
        lds_st16(lT,
                 (wave * 16 + c_sub_row + r) * BQ + qf * 16 + c_col,
                 f2bf(p * keep));
      }
    }
    // dV += PmT @ dO  (lT rows wave-private)
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int df = 0; df < 4; ++df)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 af = lds_frag(lT, wave * 16 + frag_row,
                                   ks * 32 + frag_k);
        const bf16x8 bf = lds_frag(ldOt[cur], df * 16 + frag_row,
                                   ks * 32 + frag_k);
        dv[df] = mfma_bf16(af, bf, dv[df]);
      }
    __builtin_amdgcn_s_setprio(0);
    // overwrite lT with dS^T (own-wave rows; same-wave LDS ops are
    // processed in order, so the dV reads above see the old values)
#pragma unroll
    for (int qf = 0; qf < 4; ++qf)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        lds_st16(lT,
                 (wave * 16 + c_sub_row + r) * BQ + qf * 16 + c_col,
                 f2bf(dpt[qf][r]));
    // dK += dST @ Q
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int df = 0; df < 4; ++df)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 af = lds_frag(lT, wave * 16 + frag_row,
                                   ks * 32 + frag_k);
        const bf16x8 bf = lds_frag(lQt[cur], df * 16 + frag_row,
                                   ks * 32 + frag_k);
        dk[df] = mfma_bf16(af, bf, dk[df]);
      }
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
  }

  const int krow0 = kt * BKV + wave * 16;
#pragma unroll
  for (int df = 0; df < 4; ++df)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long long off = gbase +
          (long long)(krow0 + c_sub_row + r) * grs + df * 16 + c_col;
      if constexpr (VARLEN) {  // tail key tile: padded rows store zero
        const bool valid = krow0 + c_sub_row + r < len;
        dK[off] = valid ? f2bf(dk[df][r]) : (short)0;
        dV[off] = valid ? f2bf(dv[df][r]) : (short)0;
      } else {
        dK[off] = f2bf(dk[df][r]);
        dV[off] = f2bf(dv[df][r]);
      }
    }
}

// ----------------------------------------------------------- bwd dQ

template <bool VARLEN>
__global__ __launch_bounds__(ATHREADS) void attn_bwd_dq_k(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ V, const short* __restrict__ dO,
    const short* __restrict__ KT, const float* __restrict__ LSE,
    const float* __restrict__ Drow, short* __restrict__ dQ,
    const long long* __restrict__ seed_p, int S, int H, int rs, int ors,
    int grs, unsigned p24, float inv1mp,
    const int* __restrict__ seqlens) {
  __shared__ short lK[2][TILE_ELEMS];   // [key][d]
  __shared__ short lKt[2][TILE_ELEMS];  // [d][key]
  __shared__ short lV[2][TILE_ELEMS];   // [key][d]
  __shared__ short lDS[TILE_ELEMS];

  const int bh = blockIdx.x;
  const int qt = blockIdx.y;
  const long long base =
      ((long long)(bh / H) * S) * rs + (long long)(bh % H) * 64;
  const long long obase =
      ((long long)(bh / H) * S) * ors + (long long)(bh % H) * 64;
  const long long gbase =
      ((long long)(bh / H) * S) * grs + (long long)(bh % H) * 64;
  const short* ktb = KT + (long long)bh * 64 * S;
  int len = S;
  if constexpr (VARLEN) {
    len = clamped_len(seqlens, bh / H, S);
    if (qt * BQ >= len) {  // block-uniform: the whole Q tile is padding
      zero_tile(dQ + gbase + (long long)qt * BQ * grs, grs, threadIdx.x);
      return;
    }
  }
  const unsigned seed = seed_p ? (unsigned)(*seed_p) : 0u;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;

  const FragLane fl(lane);
  const float qscale = rsqrtf((float)D);

  bf16x8 qf[2], dof[2];
  {
    const int qrow = qt * BQ + wave * 16 + fl.frag_row;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      qf[ks] = load_frag_scaled(
          Q + base + (long long)qrow * rs + ks * 32 + fl.frag_k, qscale);
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

  f32x4 dq[4];
#pragma unroll
  for (int df = 0; df < 4; ++df) dq[df] = {0.f, 0.f, 0.f, 0.f};

  auto stage_kv = [&](int buf, int t) {
    stage_tile64(lK[buf], K + base + (long long)t * BKV * rs, rs, tid);
    stage_tile64(lKt[buf], ktb + t * BKV, S, tid);
    stage_tile64(lV[buf], V + base + (long long)t * BKV * rs, rs, tid);
  };

  const int ntiles = VARLEN ? (len + BKV - 1) / BKV : S / BKV;
  stage_kv(0, 0);
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    const int cur = t & 1;
    if (t + 1 < ntiles) stage_kv(cur ^ 1, t + 1);

    f32x4 s_acc[4], dp[4];
#pragma unroll
    for (int kf = 0; kf < 4; ++kf) {
      s_acc[kf] = {0.f, 0.f, 0.f, 0.f};
      dp[kf] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 bk = lds_frag(lK[cur], kf * 16 + fl.frag_row,
                                   ks * 32 + fl.frag_k);
        const bf16x8 bv = lds_frag(lV[cur], kf * 16 + fl.frag_row,
                                   ks * 32 + fl.frag_k);
        s_acc[kf] = mfma_bf16(qf[ks], bk, s_acc[kf]);
        dp[kf] = mfma_bf16(dof[ks], bv, dp[kf]);
      }
    }

#pragma unroll
    for (int kf = 0; kf < 4; ++kf)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = qt * BQ + wave * 16 + fl.c_sub_row + r;
        const int key = t * BKV + kf * 16 + fl.c_col;
        const float p = __expf(s_acc[kf][r] - lse[r]);
        const float keep = drop_keep(seed, bh, q, key, S, p24, inv1mp);
        float ds = p * (dp[kf][r] * keep - di[r]) * qscale;
        // padded query or key: select zero (lse/di may hold anything)
        if constexpr (VARLEN) ds = q < len && key < len ? ds : 0.f;
        lds_st16(lDS,
                 (wave * 16 + fl.c_sub_row + r) * BKV + kf * 16 + fl.c_col,
                 f2bf(ds));
      }
    // dQ += dS @ K (lDS rows wave-private)
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int df = 0; df < 4; ++df)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 af = lds_frag(lDS, wave * 16 + fl.frag_row,
                                   ks * 32 + fl.frag_k);
        const bf16x8 bf = lds_frag(lKt[cur], df * 16 + fl.frag_row,
                                   ks * 32 + fl.frag_k);
        dq[df] = mfma_bf16(af, bf, dq[df]);
      }
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
  }

  const int qrow0 = qt * BQ + wave * 16;
#pragma unroll
  for (int df = 0; df < 4; ++df)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qrow = qrow0 + fl.c_sub_row + r;
      short g = f2bf(dq[df][r]);
      if constexpr (VARLEN) g = qrow < len ? g : (short)0;
      dQ[gbase + (long long)qrow * grs + df * 16 + fl.c_col] = g;
    }
}

}  // namespace

void launch_attn_pretranspose(const short* X, short* T, int BH, int S,
                              int H, int rs, hipStream_t stream) {
  hipLaunchKernelGGL(attn_pretranspose_k, dim3(BH, S / 64),
                     dim3(ATHREADS), 0, stream, X, T, S, H, rs);
}

void launch_attn_fwd(const short* Q, const short* K, const short* VT,
                     short* O, float* LSE, const long long* seed, int BH,
                     int S, int H, int rs, int ors, float dropout_p,
                     const int* seqlens, hipStream_t stream) {
  const unsigned p24 = (unsigned)(dropout_p * 16777216.0f);
  const float inv1mp = dropout_p > 0.f ? 1.f / (1.f - dropout_p) : 1.f;
  // no lengths: the fixed-length instantiation, untouched by VARLEN
  auto* fwd = seqlens ? attn_fwd_k<true> : attn_fwd_k<false>;
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
                     const int* seqlens, hipStream_t stream) {
  const unsigned p24 = (unsigned)(dropout_p * 16777216.0f);
  const float inv1mp = dropout_p > 0.f ? 1.f / (1.f - dropout_p) : 1.f;
  auto* dkdv = seqlens ? attn_bwd_dkdv_k<true> : attn_bwd_dkdv_k<false>;
  auto* dq = seqlens ? attn_bwd_dq_k<true> : attn_bwd_dq_k<false>;
  hipLaunchKernelGGL(dkdv, dim3(BH, S / BKV), dim3(ATHREADS), 0, stream,
                     Q, K, V, dO, QT, DOT, LSE, Drow, dK, dV, seed, S, H,
                     rs, ors, grs, p24, inv1mp, seqlens);
  hipLaunchKernelGGL(dq, dim3(BH, S / BQ), dim3(ATHREADS), 0, stream, Q,
                     K, V, dO, KT, LSE, Drow, dQ, seed, S, H, rs, ors,
                     grs, p24, inv1mp, seqlens);
}
