// Flash attention (forward + backward) over an UNPADDED, packed token
// buffer, bf16, fp32 accumulation, head width HD = 64 or 128:
//
//   qkv [T, 3, H, HD]  sequences back to back, sequence b = tokens
//                      cu[b] .. cu[b+1]-1 (cu_seqlens: DEVICE int32 [B+1],
//                      non-decreasing, cu[0] = 0, cu[B] <= T)
//   O   [T, H*HD]      LSE, Drow [H, T] fp32
//
// Tokens at or beyond cu[B] are spare capacity: zeros in O and dqkv, 0 in
// LSE. Lengths are read on the device only: no host sync, capturable, and
// cu_seqlens may be refilled in place between graph replays.
//
// One kernel family, template <NH, CAUSAL> with HD = 64 * NH: a [64][HD]
// operand tile is NH swizzled [64][64] half-tiles, so HD=64 is the NH=1
// case of the structure of attention_d128.hip.
//
//   * Tile schedule. The unit of work is (head, sequence b, 64-row tile t
//     of that sequence); the tile starts at token cu[b] + 64*t, wherever
//     that falls. How many tiles there are is known only on the device.
//     The B sequences and the spare range (a pseudo-sequence, b = -1,
//     whose tiles only store zeros) are B+1 ranges of at most T tokens in
//     all, so sum(ceil(len/64)) <= floor(T/64) + B + 1: the grid is sized
//     by that host-side bound. unpad_schedule_k, one block in the same
//     stream, writes the table {count; (b, t, start, len) per tile} with
//     a block scan over the sequences; a sequence's tiles are listed
//     from the last to the first, which for CAUSAL issues the longest
//     first in fwd and dQ (t+1 trips); dK/dV maps the entry to key tile
//     nt-1-t (nt-kt trips), longest first as well. Blocks beyond the
//     count return before any barrier. The table entries are clamped
//     into [0, T], and entries beyond the bound are not written, so no
//     content of cu_seqlens can index outside the buffers.
//   * No pre-transposed operands and no [.., HD, S] scratch: V for P.V,
//     dO and Q for dV and dK, K for dQ are read as MFMA fragments from
//     the row-major staged tile with ds_read_b64_tr_b16 and per-lane
//     addresses that absorb the swizzle (TrLane, as in
//     attention_d128.hip). This holds for HD=64 too: a tile that starts
//     at an arbitrary token has no 16-byte aligned [.., 64, S] image,
//     but a ROW of the packed buffer is always 16-byte aligned.
//   * Loads. Tiles are staged with the width-16 global_load_lds, rows
//     3*H*HD elements apart, double-buffered with one wait and one
//     barrier per tile. A tail tile's staged rows run into the next
//     sequence or the spare capacity; those keys and queries are masked
//     by SELECTION (scores -1e30, p and dS 0, never multiplied away),
//     so they must hold finite values and nothing else is asked of
//     them. Source rows at or beyond T are never read: the row index is
//     clamped to T-1 (staging, fragment loads, LSE and Drow alike).
//   * Stores. O, LSE, dQ, dK and dV rows are written only for tokens of
//     the block's own sequence, predicated per row; the rest of a tile's
//     64 rows belong to the next sequence's blocks. No memset, no
//     atomics, no workspace beyond the table: same bits on every run.
//   * The softmax scale 1/sqrt(HD) is applied in fp32 to the scores,
//     the same way in all three kernels, so the backward's exp(s - LSE)
//     reproduces the forward's P.
//   * CAUSAL: key k is seen from query q of the same sequence iff
//     k <= q (local positions). fwd and dQ loop key tiles 0..t, dK/dV
//     loops Q tiles kt..nt-1; only the diagonal tile carries that mask.
//   * Dropout: drop_keep(seed, b*H + h, local q, local k, max_seqlen),
//     the decision flash_attention_packed takes for the same sequences
//     right-padded to S = max_seqlen with the same seed.
//   * Drow = rowsum(dO o O) per (head, token) is unpad_rowdot_k, one
//     wave per token row.
//
// LDS per workgroup: 2 buffers x 2 operands x NH x 8 KiB + one 8 KiB
// round-trip tile = 40 KiB (HD=64), 72 KiB (HD=128): two workgroups per
// CU either way. Compiler resource report (gfx950, -O3): no kernel uses
// scratch; LDS is the dynamic 40 / 72 KiB above (1 KiB static in the
// schedule kernel). VGPRs / AGPRs:
//            HD=64      HD=64 causal   HD=128     HD=128 causal
//   fwd      144 / 16     144 / 16     174 / 32     166 / 32
//   dK/dV    168 / 36     174 / 36     185 / 68     190 / 68
//   dQ       114 / 32     118 / 32     152 / 32     156 / 32
//   schedule 32 / 0, row dot 32 / 0 (both widths)
// Occupancy by registers is 2 waves per SIMD or more (two workgroups per
// CU) except for the HD=128 causal dK/dV kernel: 190 + 68 = 258 registers,
// two over what occupancy 2 allows, so that one runs one workgroup per CU.

// device code of this file is generated without packed fp32 instructions
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

#include "attention_kernels.hip.h"

namespace {

typedef __attribute__((address_space(3))) short4v* lds_b64_ptr;

__device__ __forceinline__ unsigned lds_addr(const short* p) {
  return (unsigned)(unsigned long long)(
      (const __attribute__((address_space(3))) short*)p);
}

// The lane's part in a transposing fragment read of a swizzled [64][64]
// half-tile, as in attention_d128.hip: read i (0, 1) of the fragment at
// rows r0 .. r0+31, columns c0 .. c0+15 takes 8 bytes of row
// r0 + 8g + 4i + lg/4, columns c0 + 4*(lg%4) .. +4 (g = lane/16,
// lg = lane%16); the swizzled byte offset is
//   row * 128 + (lg & 1) * 8 + ((c0 * 2) ^ (x << 4)),
//   x = ((lg % 4) / 2) ^ (4i + lg / 4).
struct TrLane {
  unsigned off[2], x4[2];
  __device__ __forceinline__ explicit TrLane(int lane) {
    const int lg = lane & 15, g = lane >> 4;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int rl = 4 * i + (lg >> 2);
      off[i] = (8 * g + rl) * 128 + (lg & 1) * 8;
      x4[i] = (((lg & 3) >> 1) ^ rl) << 4;
    }
  }
  // B-operand fragment F[col = c0 + l%16][k = r0 + 8*(l/16) .. +8] =
  // tile[k][col] of the half-tile at LDS byte address `tile`.
  __device__ __forceinline__ bf16x8 frag(unsigned tile, int r0,
                                         int c0) const {
    const short4v v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (lds_b64_ptr)(size_t)(tile + r0 * 128 + off[0] +
                                ((c0 * 2) ^ x4[0])));
    const short4v v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (lds_b64_ptr)(size_t)(tile + r0 * 128 + off[1] +
                                ((c0 * 2) ^ x4[1])));
    return bf16x8{v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
  }
};

template <int NH>
constexpr int lds_bytes() {
  // 2 buffers x 2 operands x [64][64 NH] + one [64][64] round-trip tile
  return (4 * NH + 1) * TILE_ELEMS * 2;
}
static_assert(lds_bytes<2>() <= 80 * 1024, "two workgroups fit a CU's LDS");

// Stage rows row0 .. row0+63 of a [T][..] matrix (`g` points at column 0
// of the head, rows `stride` elements apart) as NH swizzled half-tiles.
// Rows at or beyond T are read from row T-1 instead.
template <int NH>
__device__ __forceinline__ void stage_rows(short* dst, const short* g,
                                           long long stride, int row0, int T,
                                           int tid) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int e = tile_swz128((s * ATHREADS + tid) * 16) / 2;
    const short* src =
        g + (long long)min(row0 + e / 64, T - 1) * stride + e % 64;
#pragma unroll
    for (int hf = 0; hf < NH; ++hf)
      global_load_lds16(src + hf * 64, dst + hf * TILE_ELEMS +
                                           (s * ATHREADS + (tid & ~63)) * 8);
  }
}

// K-major fragment of K-step ks (0 .. 2 NH - 1 over the head dimension)
// of a staged operand tile.
__device__ __forceinline__ bf16x8 lds_frag_ks(const short* tile, int row,
                                              int ks, int frag_k) {
  return lds_frag(tile + (ks >> 1) * TILE_ELEMS, row,
                  (ks & 1) * 32 + frag_k);
}

// Zero rows 0 .. nrows-1 (nrows <= 64) of a [..][64 NH] head slice, rows
// `stride` elements apart. 4 threads per row.
template <int NH>
__device__ __forceinline__ void zero_rows(short* g, long long stride,
                                          int nrows, int tid) {
  const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  if (tid / 4 >= nrows) return;
  short* p = g + (long long)(tid / 4) * stride + (tid % 4) * (16 * NH);
#pragma unroll
  for (int c = 0; c < 2 * NH; ++c) *(bf16x8*)(p + c * 8) = z;
}

// ------------------------------------------------------- tile schedule

// sched[0].x = number of tiles; sched[1 + i] = (b, t, start, len) of tile
// i, b = -1 for the spare range. One block; `cap` entries at the most.
__global__ __launch_bounds__(256) void unpad_schedule_k(
    const int* __restrict__ cu, int B, int T, int cap,
    int4* __restrict__ sched) {
  __shared__ int scan[256];
  const int tid = threadIdx.x;
  int base = 0;
  for (int c0 = 0; c0 <= B; c0 += 256) {  // range B is the spare capacity
    const int b = c0 + tid;
    int start = 0, len = 0;
    if (b <= B) {
      start = min(max(cu[b], 0), T);
      len = (b < B ? min(max(cu[b + 1], start), T) : T) - start;
    }
    const int n = (len + BQ - 1) / BQ;
    scan[tid] = n;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {  // inclusive scan
      const int v = tid >= off ? scan[tid - off] : 0;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    const int first = base + scan[tid] - n;
    for (int j = 0; j < n && first + j < cap; ++j)
      sched[1 + first + j] = make_int4(b < B ? b : -1, n - 1 - j, start, len);
    base += scan[255];
    __syncthreads();
  }
  if (tid == 0) sched[0] = make_int4(min(base, cap), 0, 0, 0);
}

// ------------------------------------------------------------- fwd

template <int NH, bool CAUSAL>
__global__ __launch_bounds__(ATHREADS) void attn_unpad_fwd_k(
    const short* __restrict__ qkv, short* __restrict__ O,
    float* __restrict__ LSE, const long long* __restrict__ seed_p,
    const int4* __restrict__ sched, int T, int H, int max_seqlen,
    unsigned p24, float inv1mp) {
  constexpr int HD = 64 * NH, OPE = NH * TILE_ELEMS;
  extern __shared__ __attribute__((aligned(16))) short lds[];
  short* lK = lds;            // [2][key][HD], double-buffered
  short* lV = lds + 2 * OPE;  // [2][key][HD]
  short* lP = lds + 4 * OPE;  // [q][key]

  if ((int)blockIdx.x >= sched[0].x) return;  // before any barrier
  const int4 e = sched[1 + blockIdx.x];
  const int h = blockIdx.y, qt = e.y, len = e.w;
  const int tok0 = e.z + qt * BQ;         // first token of the Q tile
  const int rows = min(BQ, len - qt * BQ);  // of them in this sequence
  const int tid = threadIdx.x;
  const long long rs = 3LL * H * HD, ors = (long long)H * HD;
  if (e.x < 0) {  // spare capacity: zeros
    zero_rows<NH>(O + tok0 * ors + h * HD, ors, rows, tid);
    if (tid < rows) LSE[(long long)h * T + tok0 + tid] = 0.f;
    return;
  }
  const short* Q = qkv + h * HD;
  const short* K = Q + H * HD;
  const short* V = K + H * HD;
  const unsigned long long bh = (unsigned long long)e.x * H + h;
  const unsigned seed = seed_p ? (unsigned)(*seed_p) : 0u;
  const int lane = tid & 63;
  const int wave = tid >> 6;

  const FragLane fl(lane);
  const TrLane tr(lane);
  const unsigned lV_addr = lds_addr(lV);
  const float qscale = rsqrtf((float)HD);

  bf16x8 qf[2 * NH];
  {
    const int qrow = min(tok0 + wave * 16 + fl.frag_row, T - 1);
#pragma unroll
    for (int ks = 0; ks < 2 * NH; ++ks)
      qf[ks] = *(const bf16x8*)(Q + qrow * rs + ks * 32 + fl.frag_k);
  }

  float m_run[4], l_run[4];
  f32x4 o_acc[4 * NH];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m_run[r] = -1e30f;
    l_run[r] = 0.f;
  }
#pragma unroll
  for (int df = 0; df < 4 * NH; ++df) o_acc[df] = {0.f, 0.f, 0.f, 0.f};

  auto stage_kv = [&](int buf, int t) {
    stage_rows<NH>(lK + buf * OPE, K, rs, e.z + t * BKV, T, tid);
    stage_rows<NH>(lV + buf * OPE, V, rs, e.z + t * BKV, T, tid);
  };

  // every tile holds a key of this sequence; CAUSAL: tiles 0..qt
  const int ntiles = CAUSAL ? qt + 1 : (len + BKV - 1) / BKV;
  stage_kv(0, 0);
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    const int cur = t & 1;
    if (t + 1 < ntiles) stage_kv(cur ^ 1, t + 1);
    const short* lKc = lK + cur * OPE;

    f32x4 s_acc[4];
#pragma unroll
    for (int kf = 0; kf < 4; ++kf) {
      s_acc[kf] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2 * NH; ++ks)
        s_acc[kf] = mfma_bf16(
            qf[ks], lds_frag_ks(lKc, kf * 16 + fl.frag_row, ks, fl.frag_k),
            s_acc[kf]);
#pragma unroll
      for (int r = 0; r < 4; ++r) s_acc[kf][r] *= qscale;  // fp32 scale
    }

    // keys of this tile at or beyond kvalid belong to the neighbour (tail
    // tile only); CAUSAL: the diagonal tile masks the keys after the
    // query. Tile-uniform; masked keys leave the running max and get
    // p = 0 by selection
    const int kvalid = len - t * BKV;
    const bool diag = CAUSAL && t == qt;
    const bool edge = diag || kvalid < BKV;
    if (edge) {
#pragma unroll
      for (int kf = 0; kf < 4; ++kf)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int kl = kf * 16 + fl.c_col;
          if (kl >= kvalid || (diag && kl > wave * 16 + fl.c_sub_row + r))
            s_acc[kf][r] = -1e30f;
        }
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
      const int ql = wave * 16 + fl.c_sub_row + r;  // row inside the tile
      float rowsum = 0.f;
#pragma unroll
      for (int kf = 0; kf < 4; ++kf) {
        const int kl = kf * 16 + fl.c_col;
        float p = __expf(s_acc[kf][r] - m_new);
        if (edge) p = kl < kvalid && !(diag && kl > ql) ? p : 0.f;
        rowsum += p;  // l accumulates the UNdropped probabilities
        const float keep = drop_keep(seed, bh, qt * BQ + ql, t * BKV + kl,
                                     max_seqlen, p24, inv1mp);
        s_acc[kf][r] = p * keep;  // dropped P feeds the PV product
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1)
        rowsum += __shfl_xor(rowsum, off, 64);
      l_run[r] = l_run[r] * scale + rowsum;
      m_run[r] = m_new;
#pragma unroll
      for (int df = 0; df < 4 * NH; ++df) o_acc[df][r] *= scale;
    }

    // P round-trip through the wave's own rows of lP (no barrier)
#pragma unroll
    for (int kf = 0; kf < 4; ++kf)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        lds_st16(lP, (wave * 16 + fl.c_sub_row + r) * BKV + kf * 16 + fl.c_col,
                 f2bf(s_acc[kf][r]));
    // O += P V: V^T fragments by transposing reads of the row-major tile
    const unsigned lVc = lV_addr + cur * (OPE * 2);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 af = lds_frag(lP, wave * 16 + fl.frag_row,
                                 ks * 32 + fl.frag_k);
#pragma unroll
      for (int df = 0; df < 4 * NH; ++df)
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

  // rows of the tile beyond `rows` are the next sequence's to write
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int ql = wave * 16 + fl.c_sub_row + r;
    if (ql >= rows) continue;
    short* orow = O + (tok0 + ql) * ors + h * HD + fl.c_col;
#pragma unroll
    for (int df = 0; df < 4 * NH; ++df)
      orow[df * 16] = f2bf(o_acc[df][r] / l_run[r]);
    if (fl.c_col == 0)
      LSE[(long long)h * T + tok0 + ql] = m_run[r] + __logf(l_run[r]);
  }
}

// --------------------------------------------------------- bwd dK/dV

template <int NH, bool CAUSAL>
__global__ __launch_bounds__(ATHREADS) void attn_unpad_bwd_dkdv_k(
    const short* __restrict__ qkv, const short* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ Drow,
    short* __restrict__ dqkv, const long long* __restrict__ seed_p,
    const int4* __restrict__ sched, int T, int H, int max_seqlen,
    unsigned p24, float inv1mp) {
  constexpr int HD = 64 * NH, OPE = NH * TILE_ELEMS;
  extern __shared__ __attribute__((aligned(16))) short lds[];
  short* lQ = lds;             // [2][q][HD]
  short* ldO = lds + 2 * OPE;  // [2][q][HD]
  short* lT = lds + 4 * OPE;   // PmT / dST round-trip [key][q]

  if ((int)blockIdx.x >= sched[0].x) return;  // before any barrier
  const int4 e = sched[1 + blockIdx.x];
  const int h = blockIdx.y, len = e.w;
  const int ntiles = (len + BQ - 1) / BQ;  // Q tiles of the sequence
  const int kt = ntiles - 1 - e.y;         // CAUSAL: longest (kt = 0) first
  const int tok0 = e.z + kt * BKV;
  const int rows = min(BKV, len - kt * BKV);
  const int tid = threadIdx.x;
  const long long rs = 3LL * H * HD, ors = (long long)H * HD;
  short* dK = dqkv + (H + h) * HD;
  short* dV = dK + H * HD;
  if (e.x < 0) {  // spare capacity: zeros
    zero_rows<NH>(dK + tok0 * rs, rs, rows, tid);
    zero_rows<NH>(dV + tok0 * rs, rs, rows, tid);
    return;
  }
  const short* Q = qkv + h * HD;
  const short* K = Q + H * HD;
  const short* V = K + H * HD;
  const short* dOh = dO + h * HD;
  const float* lse_h = LSE + (long long)h * T;
  const float* drow_h = Drow + (long long)h * T;
  const unsigned long long bh = (unsigned long long)e.x * H + h;
  const unsigned seed = seed_p ? (unsigned)(*seed_p) : 0u;
  const int lane = tid & 63;
  const int wave = tid >> 6;  // owns keys [wave*16, +16)

  const FragLane fl(lane);
  const TrLane tr(lane);
  const unsigned lQ_addr = lds_addr(lQ), ldO_addr = lds_addr(ldO);
  const float qscale = rsqrtf((float)HD);

  bf16x8 kfr[2 * NH], vfr[2 * NH];
  {
    const int krow = min(tok0 + wave * 16 + fl.frag_row, T - 1);
#pragma unroll
    for (int ks = 0; ks < 2 * NH; ++ks) {
      kfr[ks] = *(const bf16x8*)(K + krow * rs + ks * 32 + fl.frag_k);
      vfr[ks] = *(const bf16x8*)(V + krow * rs + ks * 32 + fl.frag_k);
    }
  }

  f32x4 dv[4 * NH], dk[4 * NH];
#pragma unroll
  for (int df = 0; df < 4 * NH; ++df) {
    dv[df] = {0.f, 0.f, 0.f, 0.f};
    dk[df] = {0.f, 0.f, 0.f, 0.f};
  }

  auto stage_q = [&](int buf, int it) {
    stage_rows<NH>(lQ + buf * OPE, Q, rs, e.z + it * BQ, T, tid);
    stage_rows<NH>(ldO + buf * OPE, dOh, ors, e.z + it * BQ, T, tid);
  };

  // CAUSAL: Q tiles before kt see none of these keys
  const int it0 = CAUSAL ? kt : 0;
  stage_q(0, it0);
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();

  for (int it = it0; it < ntiles; ++it) {
    const int cur = (it - it0) & 1;  // trips since the first tile
    if (it + 1 < ntiles) stage_q(cur ^ 1, it + 1);
    const short* lQc = lQ + cur * OPE;
    const short* ldOc = ldO + cur * OPE;

    // S^T = K Q^T; dP^T = V dO^T
    f32x4 st[4], dpt[4];
#pragma unroll
    for (int qf = 0; qf < 4; ++qf) {
      st[qf] = {0.f, 0.f, 0.f, 0.f};
      dpt[qf] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2 * NH; ++ks) {
        st[qf] = mfma_bf16(
            kfr[ks], lds_frag_ks(lQc, qf * 16 + fl.frag_row, ks, fl.frag_k),
            st[qf]);
        dpt[qf] = mfma_bf16(
            vfr[ks], lds_frag_ks(ldOc, qf * 16 + fl.frag_row, ks, fl.frag_k),
            dpt[qf]);
      }
    }

    // per-lane fixed q column: one LSE/Drow scalar per qf
#pragma unroll
    for (int qf = 0; qf < 4; ++qf) {
      const int q = it * BQ + qf * 16 + fl.c_col;  // local position
      const int qtok = min(e.z + q, T - 1);
      const float lse = lse_h[qtok];
      const float di = drow_h[qtok];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kt * BKV + wave * 16 + fl.c_sub_row + r;
        float p = __expf(st[qf][r] * qscale - lse);
        const float keep = drop_keep(seed, bh, q, key, max_seqlen, p24,
                                     inv1mp);
        float dst = p * (dpt[qf][r] * keep - di) * qscale;  // dS^T*scale
        // a query or key of the neighbour, or a key after the query:
        // lse/di may hold anything, so select zeros
        const bool valid = q < len && key < len && (!CAUSAL || key <= q);
        p = valid ? p * keep : 0.f;
        dpt[qf][r] = valid ? dst : 0.f;
        lds_st16(lT, (wave * 16 + fl.c_sub_row + r) * BQ + qf * 16 + fl.c_col,
                 f2bf(p));
      }
    }
    // dV += PmT @ dO: dO^T fragments by transposing reads (lT rows are
    // wave-private)
    const unsigned ldOa = ldO_addr + cur * (OPE * 2);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 af = lds_frag(lT, wave * 16 + fl.frag_row,
                                 ks * 32 + fl.frag_k);
#pragma unroll
      for (int df = 0; df < 4 * NH; ++df)
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
    const unsigned lQa = lQ_addr + cur * (OPE * 2);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 af = lds_frag(lT, wave * 16 + fl.frag_row,
                                 ks * 32 + fl.frag_k);
#pragma unroll
      for (int df = 0; df < 4 * NH; ++df)
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

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int kl = wave * 16 + fl.c_sub_row + r;
    if (kl >= rows) continue;  // the next sequence's rows
    const long long off = (tok0 + kl) * rs + fl.c_col;
#pragma unroll
    for (int df = 0; df < 4 * NH; ++df) {
      dK[off + df * 16] = f2bf(dk[df][r]);
      dV[off + df * 16] = f2bf(dv[df][r]);
    }
  }
}

// ----------------------------------------------------------- bwd dQ

template <int NH, bool CAUSAL>
__global__ __launch_bounds__(ATHREADS) void attn_unpad_bwd_dq_k(
    const short* __restrict__ qkv, const short* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ Drow,
    short* __restrict__ dqkv, const long long* __restrict__ seed_p,
    const int4* __restrict__ sched, int T, int H, int max_seqlen,
    unsigned p24, float inv1mp) {
  constexpr int HD = 64 * NH, OPE = NH * TILE_ELEMS;
  extern __shared__ __attribute__((aligned(16))) short lds[];
  short* lK = lds;            // [2][key][HD]
  short* lV = lds + 2 * OPE;  // [2][key][HD]
  short* lDS = lds + 4 * OPE;

  if ((int)blockIdx.x >= sched[0].x) return;  // before any barrier
  const int4 e = sched[1 + blockIdx.x];
  const int h = blockIdx.y, qt = e.y, len = e.w;
  const int tok0 = e.z + qt * BQ;
  const int rows = min(BQ, len - qt * BQ);
  const int tid = threadIdx.x;
  const long long rs = 3LL * H * HD, ors = (long long)H * HD;
  short* dQ = dqkv + h * HD;
  if (e.x < 0) {  // spare capacity: zeros
    zero_rows<NH>(dQ + tok0 * rs, rs, rows, tid);
    return;
  }
  const short* Q = qkv + h * HD;
  const short* K = Q + H * HD;
  const short* V = K + H * HD;
  const unsigned long long bh = (unsigned long long)e.x * H + h;
  const unsigned seed = seed_p ? (unsigned)(*seed_p) : 0u;
  const int lane = tid & 63;
  const int wave = tid >> 6;

  const FragLane fl(lane);
  const TrLane tr(lane);
  const unsigned lK_addr = lds_addr(lK);
  const float qscale = rsqrtf((float)HD);

  bf16x8 qf[2 * NH], dof[2 * NH];
  {
    const int qrow = min(tok0 + wave * 16 + fl.frag_row, T - 1);
#pragma unroll
    for (int ks = 0; ks < 2 * NH; ++ks) {
      qf[ks] = *(const bf16x8*)(Q + qrow * rs + ks * 32 + fl.frag_k);
      dof[ks] = *(const bf16x8*)(dO + qrow * ors + h * HD + ks * 32 +
                                 fl.frag_k);
    }
  }
  float lse[4], di[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qtok = min(tok0 + wave * 16 + fl.c_sub_row + r, T - 1);
    lse[r] = LSE[(long long)h * T + qtok];
    di[r] = Drow[(long long)h * T + qtok];
  }

  f32x4 dq[4 * NH];
#pragma unroll
  for (int df = 0; df < 4 * NH; ++df) dq[df] = {0.f, 0.f, 0.f, 0.f};

  auto stage_kv = [&](int buf, int t) {
    stage_rows<NH>(lK + buf * OPE, K, rs, e.z + t * BKV, T, tid);
    stage_rows<NH>(lV + buf * OPE, V, rs, e.z + t * BKV, T, tid);
  };

  // CAUSAL: key tiles 0..qt, as in attn_unpad_fwd_k
  const int ntiles = CAUSAL ? qt + 1 : (len + BKV - 1) / BKV;
  stage_kv(0, 0);
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();

  for (int t = 0; t < ntiles; ++t) {
    const int cur = t & 1;
    if (t + 1 < ntiles) stage_kv(cur ^ 1, t + 1);
    const short* lKc = lK + cur * OPE;
    const short* lVc = lV + cur * OPE;

    f32x4 s_acc[4], dp[4];
#pragma unroll
    for (int kf = 0; kf < 4; ++kf) {
      s_acc[kf] = {0.f, 0.f, 0.f, 0.f};
      dp[kf] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2 * NH; ++ks) {
        s_acc[kf] = mfma_bf16(
            qf[ks], lds_frag_ks(lKc, kf * 16 + fl.frag_row, ks, fl.frag_k),
            s_acc[kf]);
        dp[kf] = mfma_bf16(
            dof[ks], lds_frag_ks(lVc, kf * 16 + fl.frag_row, ks, fl.frag_k),
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
        const float keep = drop_keep(seed, bh, q, key, max_seqlen, p24,
                                     inv1mp);
        float ds = p * (dp[kf][r] * keep - di[r]) * qscale;
        // a query or key of the neighbour, or a key after the query:
        // select zero (lse/di may hold anything)
        ds = q < len && key < len && (!CAUSAL || key <= q) ? ds : 0.f;
        lds_st16(lDS,
                 (wave * 16 + fl.c_sub_row + r) * BKV + kf * 16 + fl.c_col,
                 f2bf(ds));
      }
    // dQ += dS @ K: K^T fragments by transposing reads (lDS rows are
    // wave-private)
    const unsigned lKa = lK_addr + cur * (OPE * 2);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 af = lds_frag(lDS, wave * 16 + fl.frag_row,
                                 ks * 32 + fl.frag_k);
#pragma unroll
      for (int df = 0; df < 4 * NH; ++df)
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

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int ql = wave * 16 + fl.c_sub_row + r;
    if (ql >= rows) continue;  // the next sequence's rows
    short* grow = dQ + (tok0 + ql) * rs + fl.c_col;
#pragma unroll
    for (int df = 0; df < 4 * NH; ++df) grow[df * 16] = f2bf(dq[df][r]);
  }
}

// ------------------------------------------------------ row dot product

// Drow[h][t] = sum_d dO[t][h*HD + d] * O[t][h*HD + d], fp32. One wave per
// token row; HD/8 lanes hold one head's 16 B pieces and reduce by
// shuffles (the loop bound H*HD/8 is a multiple of that group, so a
// group is active or idle as a whole).
template <int NH>
__global__ __launch_bounds__(256) void unpad_rowdot_k(
    const short* __restrict__ dO, const short* __restrict__ O,
    float* __restrict__ Drow, int T, int H) {
  constexpr int G = 8 * NH;  // lanes per head
  const int tok = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tok >= T) return;
  const int lane = threadIdx.x & 63;
  const long long row = (long long)tok * H * (64 * NH);
  for (int c = lane; c < H * G; c += 64) {
    const bf16x8 a = *(const bf16x8*)(dO + row + c * 8);
    const bf16x8 b = *(const bf16x8*)(O + row + c * 8);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += bf2f(a[j]) * bf2f(b[j]);
#pragma unroll
    for (int off = 1; off < G; off <<= 1) s += __shfl_xor(s, off, 64);
    if (c % G == 0) Drow[(long long)(c / G) * T + tok] = s;
  }
}

// One launch of KERNEL with NH's dynamic LDS (above the 64 KiB default
// for NH = 2).
template <auto KERNEL, int NH, typename... Args>
void launch_unpad(dim3 grid, hipStream_t stream, Args... args) {
  static const hipError_t lds_set =
      hipFuncSetAttribute((const void*)KERNEL,
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          lds_bytes<NH>());
  (void)lds_set;
  hipLaunchKernelGGL(KERNEL, grid, dim3(ATHREADS), lds_bytes<NH>(), stream,
                     args...);
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

int attn_unpad_max_tiles(int T, int B) { return T / BQ + B + 1; }

void launch_attn_unpad_schedule(const int* cu_seqlens, int B, int T,
                                int* sched, hipStream_t stream) {
  hipLaunchKernelGGL(unpad_schedule_k, dim3(1), dim3(256), 0, stream,
                     cu_seqlens, B, T, attn_unpad_max_tiles(T, B),
                     (int4*)sched);
}

void launch_attn_unpad_rowdot(const short* dO, const short* O, float* Drow,
                              int T, int H, int D, hipStream_t stream) {
  const dim3 grid((T + 3) / 4);
  if (D == 128)
    hipLaunchKernelGGL(unpad_rowdot_k<2>, grid, dim3(256), 0, stream, dO, O,
                       Drow, T, H);
  else
    hipLaunchKernelGGL(unpad_rowdot_k<1>, grid, dim3(256), 0, stream, dO, O,
                       Drow, T, H);
}

// One workgroup per (schedule entry, head).
void launch_attn_unpad_fwd(const short* qkv, short* O, float* LSE,
                           const long long* seed, const int* sched, int B,
                           int T, int H, int D, int max_seqlen,
                           float dropout_p, bool causal,
                           hipStream_t stream) {
  const unsigned p24 = (unsigned)(dropout_p * 16777216.0f);
  const float inv1mp = dropout_p > 0.f ? 1.f / (1.f - dropout_p) : 1.f;
  const dim3 grid(attn_unpad_max_tiles(T, B), H);
#define SPARKDL_UNPAD_FWD(NH, CA)                                          \
  launch_unpad<attn_unpad_fwd_k<NH, CA>, NH>(grid, stream, qkv, O, LSE,    \
                                             seed, (const int4*)sched, T,  \
                                             H, max_seqlen, p24, inv1mp)
  if (D == 128) {
    if (causal) SPARKDL_UNPAD_FWD(2, true);
    else SPARKDL_UNPAD_FWD(2, false);
  } else {
    if (causal) SPARKDL_UNPAD_FWD(1, true);
    else SPARKDL_UNPAD_FWD(1, false);
  }
#undef SPARKDL_UNPAD_FWD
}

void launch_attn_unpad_bwd(const short* qkv, const short* dO,
                           const float* LSE, const float* Drow, short* dqkv,
                           const long long* seed, const int* sched, int B,
                           int T, int H, int D, int max_seqlen,
                           float dropout_p, bool causal,
                           hipStream_t stream) {
  const unsigned p24 = (unsigned)(dropout_p * 16777216.0f);
  const float inv1mp = dropout_p > 0.f ? 1.f / (1.f - dropout_p) : 1.f;
  const dim3 grid(attn_unpad_max_tiles(T, B), H);
#define SPARKDL_UNPAD_BWD(NH, CA)                                          \
  do {                                                                     \
    launch_unpad<attn_unpad_bwd_dkdv_k<NH, CA>, NH>(                       \
        grid, stream, qkv, dO, LSE, Drow, dqkv, seed, (const int4*)sched,  \
        T, H, max_seqlen, p24, inv1mp);                                    \
    launch_unpad<attn_unpad_bwd_dq_k<NH, CA>, NH>(                         \
        grid, stream, qkv, dO, LSE, Drow, dqkv, seed, (const int4*)sched,  \
        T, H, max_seqlen, p24, inv1mp);                                    \
  } while (0)
  if (D == 128) {
    if (causal) SPARKDL_UNPAD_BWD(2, true);
    else SPARKDL_UNPAD_BWD(2, false);
  } else {
    if (causal) SPARKDL_UNPAD_BWD(1, true);
    else SPARKDL_UNPAD_BWD(1, false);
  }
#undef SPARKDL_UNPAD_BWD
}
