// Fused BatchNorm(+residual add)(+ReLU), bf16 NHWC activations with fp32
// statistics and affine parameters (the BN+ReLU
// epilogue of the ResNet conv blocks).
//
// channels_last [N,C,H,W] tensors are exactly [rows=N*H*W, C] row-major,
// so the channel dim is the contiguous innermost axis. All kernels use
// short8 (16 B/lane) vector access.
//
// Per-channel reductions (batch statistics, dgamma/dbeta) run in two
// stages with no float atomics anywhere (Guideline 12, partial-slab
// reducer), so they are bitwise reproducible from run to run:
//   1. bn_stats_k / bn_bwd_reduce_k: G blocks grid-stride over the rows,
//      kUnroll rows of independent 16 B loads in flight per thread,
//      accumulating in registers. Each block folds its threads' partials
//      in a fixed order (bn_block_fold) and writes its 2*C sums with
//      plain vector stores to its own row of an fp32 slab [G][2*C].
//      Every one of the G rows is written in every call, so the slab is
//      neither zeroed nor reused across calls.
//   2. bn_finalize_k / bn_bwd_finalize_k: 64 threads per channel sum the
//      G slab rows in a fixed order, then compute the per-channel
//      statistics and coefficients.
//
// Reduce grid G (bn_reduce_blocks), chosen per site:
//   G = min(row_blocks, max(256, min(512, rows / 64)))
//   - row_blocks = ceil(rows / rows-per-block): never a block without
//     rows.
//   - rows / 64: a block sums at least 64 rows, so slab write plus
//     read-back (16*G*C bytes) is at most 1/8 of the bf16 input
//     (2*rows*C bytes); at the batch-512 ResNet-50 sites it is
//     0.06-12.5 %.
//   - cap 512: two blocks per CU with kUnroll rows of loads per thread
//     already stream at 5.2-6.7 TB/s at the batch-512 ResNet-50 sites
//     (profiles/bn_microbench.txt); 768-2048 blocks are within a few
//     percent either way and only add slab rows to write and read back.
//   - floor 256: one block per CU. Sites this small are latency-bound,
//     and the slab there is at most 256 rows (<= 4 MB at C=2048).
//
// Replaces the MIOpen BN + eager ReLU + eager residual-add chain (and
// their autocast fp32 round-trips) with:
//   fwd: stats (1 pass over x) -> finalize -> apply (1 pass)
//   bwd: reduce (1 pass) -> finalize -> apply (1 pass)
// vs MIOpen's separate BN fwd/bwd + ReLU fwd/bwd + add kernels.
//
// The backward is one reduce and one apply kernel, templated on where
// the masked gradient dym of a pixel comes from (a gradient source:
// load() issues the global loads of one row, eval() turns them into
// dym). Geometry, unroll, fold, slab and the per-element expressions
// (bn_xhat, bn_dx) are the kernels', so every source gives bitwise the
// dx, dgamma and dbeta of the unfused chain it stands for:
//   DySrc<RELU>: dy loaded and, with RELU, masked.
//   SumSrc<RELU>: the output has two consumers (a bottleneck's bn3
//     output feeds the next block's conv1 and its residual branch), and
//     autograd would first add the two incoming gradients in a pass of
//     its own (3 tensors of traffic). The reduce kernel takes both
//     parts instead, forms s = mask ? bf16(u + v) : 0 with ATen's
//     rounding, writes s and accumulates over it; the apply kernel
//     runs on DySrc<false> over s, reading x and s only. s is also the
//     gradient of the residual input, so the chain moves 7 tensors
//     where add + reduce + apply (with its dres store) moved 9.
//   PoolSrc: the ResNet stem, BN + ReLU + MaxPool2d(3, stride 2, pad 1)
//     as one chain with bn_apply_pool_k. The full-resolution y, the
//     pool's int64 indices and the full-resolution dy are never
//     written: the forward writes the pooled bf16 and one byte per
//     pooled element (the winning tap kh*3+kw, or kPoolDead where the
//     ReLU passes no gradient), and the source gathers each input
//     pixel's dy from the 1, 2 or 4 windows that contain it. The
//     forward rounds with bn_affine as bn_apply_k does and the gather
//     adds in ATen's order, so every result is bitwise what
//     bn_apply_k -> ATen max-pool (and back) gives.

#include "common.hip.h"
#include "kernels.h"

namespace {

constexpr int kBlock = 256;
constexpr int kVec = 8;
// Rows of independent loads in flight per thread in the reduce loops.
// Measured at the ResNet-50 sites: 2 beats 1 by up to 35 % at G <= 512;
// 4 gains nothing in bn_stats_k and loses in bn_bwd_reduce_k.
constexpr int kUnroll = 2;
// Block-fold tile: rows-per-block * 2*C floats <= 256 threads * 16.
constexpr int kFoldFloats = kBlock * 2 * kVec;  // 16 KB
// Second stage: each block finalizes kFinCh channels with
// kBlock / kFinCh = 64 slab-row lanes per channel.
constexpr int kFinCh = 4;

// Rows that one block pass covers: cols / kVec threads hold a row
// (cols % 8 == 0), and past 256 of them a row takes the whole block.
__host__ __device__ inline int bn_rows_per_block(int cols) {
  return kBlock / min(cols / kVec, kBlock);
}

// A thread's place in that pass: its row (row_off < rpb, else idle) and
// the first of its kVec columns.
struct BnGeom {
  int rpb, lane_col, row_off;
};
__device__ __forceinline__ BnGeom bn_geom(int cols) {
  const int tpr = cols / kVec;
  return {bn_rows_per_block(cols), (int)((threadIdx.x % tpr) * kVec),
          (int)(threadIdx.x / tpr)};
}

// The kVec per-channel floats of a lane, from p = base + lane_col.
struct Chan8 {
  float4v lo, hi;
  __device__ __forceinline__ float operator[](int j) const {
    return j < 4 ? lo[j] : hi[j - 4];
  }
};
__device__ __forceinline__ Chan8 bn_chan8(const float* __restrict__ p) {
  return {*(const float4v*)(p), *(const float4v*)(p + 4)};
}

// Per-element expressions, shared by the plain and the pooled kernels
// so that both contract and round alike.
__device__ __forceinline__ float bn_affine(short x, float scale,
                                           float shift) {
  return bf2f(x) * scale + shift;
}
__device__ __forceinline__ float bn_xhat(short x, float mean, float rstd) {
  return (bf2f(x) - mean) * rstd;
}
__device__ __forceinline__ float bn_dx(float d, float xh, float k1,
                                       float k2, float k3) {
  return k1 * (d - k2 - xh * k3);
}

// --------------------------------------------------------------------
// Forward
// --------------------------------------------------------------------

// Store an accumulator pair as 16 B vectors: a at p[0..8), b at
// p[cols..cols+8).
__device__ __forceinline__ void bn_store_pair(
    float* p, int cols, const float (&a)[kVec], const float (&b)[kVec]) {
  *(float4v*)(p) = float4v{a[0], a[1], a[2], a[3]};
  *(float4v*)(p + 4) = float4v{a[4], a[5], a[6], a[7]};
  *(float4v*)(p + cols) = float4v{b[0], b[1], b[2], b[3]};
  *(float4v*)(p + cols + 4) = float4v{b[4], b[5], b[6], b[7]};
}

// Fold the per-thread [kVec] accumulator pairs of a block into one
// [2*cols] row and store it to the block's slab row. Threads that hold
// the same columns sit `tpr` apart; their partials go to an LDS tile
// [rpb][2*cols] and are summed by a halving tree over the row index
// (rows [s, n) add into rows [0, n-s)), which fixes the order of every
// addition for any rpb, power of two or not. Row 0 ends with the block
// total in registers. Called by all kBlock threads.
__device__ __forceinline__ void bn_block_fold(
    float* lds, float (&a)[kVec], float (&b)[kVec], int rpb, int row_off,
    int lane_col, int cols, float* __restrict__ slab_row) {
  const bool active = row_off < rpb;
  // only dereferenced by active threads: row_off < rpb keeps it in-tile
  float* mine = lds + (size_t)row_off * 2 * cols + lane_col;
  if (active) bn_store_pair(mine, cols, a, b);
  int s = 1;
  while (s < rpb) s <<= 1;
  int n = rpb;  // live rows
  for (s >>= 1; s >= 1; s >>= 1) {
    __syncthreads();
    if (row_off < s && row_off + s < n) {
      const float* peer = mine + (size_t)s * 2 * cols;
      const float4v pa0 = *(const float4v*)(peer);
      const float4v pa1 = *(const float4v*)(peer + 4);
      const float4v pb0 = *(const float4v*)(peer + cols);
      const float4v pb1 = *(const float4v*)(peer + cols + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a[j] += pa0[j];
        a[j + 4] += pa1[j];
        b[j] += pb0[j];
        b[j + 4] += pb1[j];
      }
      // rows [0, s) are read again at the next step
      if (s > 1) bn_store_pair(mine, cols, a, b);
    }
    n = min(n, s);
  }
  if (row_off == 0) bn_store_pair(slab_row + lane_col, cols, a, b);
}

// Second stage: sum column c and column cols+c of the G slab rows for
// the block's kFinCh channels. Thread t takes channel t % kFinCh and
// slab rows t / kFinCh, +64, ...; the 16 row lanes of a wave fold by
// butterfly, the 4 waves through LDS, all in a fixed order. Threads
// 0..kFinCh-1 return the totals of channel blk*kFinCh + t.
__device__ __forceinline__ void bn_slab_sum(
    const float* __restrict__ slab, int G, int cols, int blk, float* red,
    float& sum_a, float& sum_b) {
  const int c = blk * kFinCh + threadIdx.x % kFinCh;
  float sa = 0.f, sb = 0.f;
#pragma unroll 4
  for (int g = threadIdx.x / kFinCh; g < G; g += kBlock / kFinCh) {
    const float* row = slab + (size_t)g * 2 * cols;
    sa += row[c];
    sb += row[cols + c];
  }
#pragma unroll
  for (int off = kFinCh; off < WAVE; off <<= 1) {
    sa += __shfl_xor(sa, off, WAVE);
    sb += __shfl_xor(sb, off, WAVE);
  }
  const int lane = threadIdx.x % WAVE;
  const int wid = threadIdx.x / WAVE;
  if (lane < kFinCh) {
    red[wid * 2 * kFinCh + lane] = sa;
    red[wid * 2 * kFinCh + kFinCh + lane] = sb;
  }
  __syncthreads();
  sum_a = 0.f;
  sum_b = 0.f;
  if (threadIdx.x < kFinCh) {
#pragma unroll
    for (int w = 0; w < kBlock / WAVE; ++w) {
      sum_a += red[w * 2 * kFinCh + threadIdx.x];
      sum_b += red[w * 2 * kFinCh + kFinCh + threadIdx.x];
    }
  }
}

// Channel group of a finalize block. Consecutive blocks are dealt
// round-robin to the 8 XCDs, whose L2s are separate; with 16 B of a
// 128 B slab line per block, eight neighbours would pull every line
// into eight L2s (measured at C=2048, G=392: 11.4 us against 5.2). Giving
// each XCD one contiguous channel range fetches a line once. Only a
// placement hint: any mapping is correct as long as it is a bijection.
__device__ __forceinline__ int bn_fin_block() {
  const int nb = gridDim.x;
  if (nb % 8) return blockIdx.x;
  return (blockIdx.x % 8) * (nb / 8) + blockIdx.x / 8;
}

// slab row layout: [0..C) sum, [C..2C) sumsq
template <int U>
__global__ __launch_bounds__(kBlock) void bn_stats_k(
    const short* __restrict__ x, float* __restrict__ slab,
    long long rows, int cols) {
  __shared__ __attribute__((aligned(16))) float lds[kFoldFloats];
  const BnGeom t = bn_geom(cols);

  float s[kVec] = {0.f}, ss[kVec] = {0.f};
  if (t.row_off < t.rpb) {
    const long long stride = (long long)gridDim.x * t.rpb;
    long long r = (long long)blockIdx.x * t.rpb + t.row_off;
    // U rows of loads issued before the first use
    for (; r + (U - 1) * stride < rows; r += U * stride) {
      short8 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u)
        v[u] = *(const short8*)(x + (r + u * stride) * cols + t.lane_col);
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int j = 0; j < kVec; ++j) {
          const float f = bf2f(v[u][j]);
          s[j] += f;
          ss[j] += f * f;
        }
      }
    }
    for (; r < rows; r += stride) {
      const short8 v = *(const short8*)(x + r * cols + t.lane_col);
#pragma unroll
      for (int j = 0; j < kVec; ++j) {
        const float f = bf2f(v[j]);
        s[j] += f;
        ss[j] += f * f;
      }
    }
  }
  bn_block_fold(lds, s, ss, t.rpb, t.row_off, t.lane_col, cols,
                slab + (size_t)blockIdx.x * 2 * cols);
}

// Second stage of the statistics (grid = cols / kFinCh blocks): sum the
// G slab rows per channel, then batch stats, running-stat update, and
// the fused apply coefficients scale=gamma*rstd, shift=beta-mean*scale.
__global__ __launch_bounds__(kBlock) void bn_finalize_k(
    const float* __restrict__ slab, int G, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ running_mean,
    float* __restrict__ running_var, float* __restrict__ save_mean,
    float* __restrict__ save_rstd, float* __restrict__ scale,
    float* __restrict__ shift, long long rows, int cols, float momentum,
    float eps, int training) {
  __shared__ float red[kBlock / WAVE * 2 * kFinCh];
  float sum = 0.f, sumsq = 0.f;
  const int blk = bn_fin_block();
  if (training) bn_slab_sum(slab, G, cols, blk, red, sum, sumsq);  // uniform
  if (threadIdx.x >= kFinCh) return;
  const int c = blk * kFinCh + threadIdx.x;
  float mean, rstd;
  if (training) {
    mean = sum / rows;
    const float var = fmaxf(sumsq / rows - mean * mean, 0.f);
    rstd = rsqrtf(var + eps);
    // torch semantics: running_var tracks the UNBIASED batch variance.
    const float unbiased = rows > 1 ? var * rows / (rows - 1) : var;
    running_mean[c] += momentum * (mean - running_mean[c]);
    running_var[c] += momentum * (unbiased - running_var[c]);
    save_mean[c] = mean;
    save_rstd[c] = rstd;
  } else {
    mean = running_mean[c];
    rstd = rsqrtf(running_var[c] + eps);
    save_mean[c] = mean;
    save_rstd[c] = rstd;
  }
  const float sc = gamma[c] * rstd;
  scale[c] = sc;
  shift[c] = beta[c] - mean * sc;
}

// y = relu?(scale*x + shift [+ residual]); block processes whole rows.
// With RELU, the activation mask is packed 1 bit/elem (one byte per
// vec8 lane slot) so backward never re-reads y.
template <bool RELU, bool RES>
__global__ __launch_bounds__(kBlock) void bn_apply_k(
    const short* __restrict__ x, const short* __restrict__ res,
    const float* __restrict__ scale, const float* __restrict__ shift,
    short* __restrict__ y, unsigned char* __restrict__ mask,
    long long rows, int cols) {
  const BnGeom t = bn_geom(cols);
  if (t.row_off >= t.rpb) return;
  const Chan8 sc = bn_chan8(scale + t.lane_col);
  const Chan8 sh = bn_chan8(shift + t.lane_col);

  for (long long r = (long long)blockIdx.x * t.rpb + t.row_off; r < rows;
       r += (long long)gridDim.x * t.rpb) {
    const long long base = r * cols + t.lane_col;
    const short8 v = *(const short8*)(x + base);
    short8 o;
    unsigned char mbits = 0;
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      float f = bn_affine(v[j], sc[j], sh[j]);
      if (RES) f += bf2f(res[base + j]);
      if (RELU) {
        if (f > 0.f) mbits |= (unsigned char)(1u << j);
        f = fmaxf(f, 0.f);
      }
      o[j] = f2bf(f);
    }
    *(short8*)(y + base) = o;
    if (RELU) mask[(r * cols + t.lane_col) / kVec] = mbits;
  }
}

// --------------------------------------------------------------------
// Backward
// --------------------------------------------------------------------
// Image and pooled sizes of the stem chain (PoolSrc).
struct PoolGeom {
  int H, W, Ho, Wo;
};

// A gradient source gives dym = dy * relu_mask (mask from the saved
// output y > 0) of the kVec elements at offset base = r*cols + lane_col:
//   Row load(base, r, cols, lane_col): every global load the row needs
//     and no arithmetic on what they return, so that the reduce kernel
//     can issue U rows of loads before the first use. base comes from
//     the kernel, which addresses x with it; a source that forms it
//     again costs the apply kernels registers and occupancy;
//   float eval(row, j): dym of element j from the loaded values, one
//     element at a time inside the kernels' own loop over j. With a
//     row's gradients formed ahead of that loop the compiler no longer
//     folds dres = bf16(dym) of an unmasked dy to dy;
//   make(bytes, ga, gb, s, g): the source over the kernels' operands: a
//     byte plane of the forward, up to two gradients, a row to write
//     back, the pool geometry. They are kernel parameters of their own
//     because only those carry __restrict__ (on struct members it is
//     ignored): with the pointers inside a struct argument the masked
//     reduce kernel no longer issues its loads ahead of the first use;
//   kStores: the source also writes the row back (store(row, base)),
//     which only the reduce kernel does.
// The measurements behind the choices in load, eval and make are in
// profiles/bn_refactor_isa.txt.

// dy * mask; without RELU the mask is neither loaded nor applied.
template <bool RELU>
struct DySrc {
  static constexpr bool kStores = false;
  const unsigned char* mask;
  const short* dy;
  static __device__ __forceinline__ DySrc make(
      const unsigned char* mask, const short* dy, const short*, short*,
      const PoolGeom&) {
    return {mask, dy};
  }
  struct Row {
    short8 dy;
    unsigned char mbits;
  };
  __device__ __forceinline__ Row load(long long base, long long, int,
                                      int) const {
    Row t;
    t.dy = *(const short8*)(dy + base);
    t.mbits = 0xffu;
    if (RELU) t.mbits = mask[base / kVec];
    return t;
  }
  __device__ __forceinline__ float eval(const Row& t, int j) const {
    float d = bf2f(t.dy[j]);
    if (RELU && !(t.mbits & (1u << j))) d = 0.f;
    return d;
  }
};

// The output fed two consumers and dy = u + v arrives as its two parts.
// s = mask ? bf16(u + v) : 0 is the dy * mask of DySrc and, rounded as
// ATen rounds its bf16 add, also its dres. Only the reduce kernel runs
// on this source: it stores s, the apply kernel then reads it back as
// DySrc<false> in place of dy and the mask, and the caller hands it on
// as the residual gradient.
template <bool RELU>
struct SumSrc {
  static constexpr bool kStores = true;
  const unsigned char* mask;
  const short* dya;
  const short* dyb;
  short* s;
  static __device__ __forceinline__ SumSrc make(
      const unsigned char* mask, const short* dya, const short* dyb,
      short* s, const PoolGeom&) {
    return {mask, dya, dyb, s};
  }
  struct Row {
    short8 ua, ub, sv;  // sv: s of the row, filled by eval
    unsigned char mbits;
  };
  __device__ __forceinline__ Row load(long long base, long long, int,
                                      int) const {
    Row t;
    t.ua = *(const short8*)(dya + base);
    t.ub = *(const short8*)(dyb + base);
    t.mbits = 0xffu;
    if (RELU) t.mbits = mask[base / kVec];
    return t;
  }
  __device__ __forceinline__ float eval(Row& t, int j) const {
    short sb = f2bf(bf2f(t.ua[j]) + bf2f(t.ub[j]));
    if (RELU && !(t.mbits & (1u << j))) sb = 0;
    t.sv[j] = sb;
    return bf2f(sb);
  }
  __device__ __forceinline__ void store(const Row& t,
                                        long long base) const {
    *(short8*)(s + base) = t.sv;
  }
};

// slab row layout: [0..C) sum(dym), [C..2C) sum(dym * xhat)
template <class Src, int U>
__global__ __launch_bounds__(kBlock) void bn_bwd_reduce_k(
    const short* __restrict__ x, const unsigned char* __restrict__ bytes,
    const short* __restrict__ ga, const short* __restrict__ gb,
    short* __restrict__ s, PoolGeom g,
    const float* __restrict__ save_mean,
    const float* __restrict__ save_rstd, float* __restrict__ slab,
    long long rows, int cols) {
  __shared__ __attribute__((aligned(16))) float lds[kFoldFloats];
  const Src src = Src::make(bytes, ga, gb, s, g);
  const BnGeom t = bn_geom(cols);

  float s1[kVec] = {0.f}, s2[kVec] = {0.f};
  if (t.row_off < t.rpb) {
    const Chan8 mean = bn_chan8(save_mean + t.lane_col);
    const Chan8 rstd = bn_chan8(save_rstd + t.lane_col);
    auto accum = [&](const short8& xv, typename Src::Row& row,
                     long long base) {
#pragma unroll
      for (int j = 0; j < kVec; ++j) {
        const float d = src.eval(row, j);
        const float xh = bn_xhat(xv[j], mean[j], rstd[j]);
        s1[j] += d;
        s2[j] += d * xh;
      }
      if constexpr (Src::kStores) src.store(row, base);
    };
    const long long stride = (long long)gridDim.x * t.rpb;
    long long r = (long long)blockIdx.x * t.rpb + t.row_off;
    // U rows of loads issued before the first use
    for (; r + (U - 1) * stride < rows; r += U * stride) {
      short8 xv[U];
      typename Src::Row row[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long ru = r + u * stride;
        const long long base = ru * cols + t.lane_col;
        xv[u] = *(const short8*)(x + base);
        row[u] = src.load(base, ru, cols, t.lane_col);
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        accum(xv[u], row[u], (r + u * stride) * cols + t.lane_col);
    }
    for (; r < rows; r += stride) {
      const long long base = r * cols + t.lane_col;
      const short8 xv = *(const short8*)(x + base);
      typename Src::Row row = src.load(base, r, cols, t.lane_col);
      accum(xv, row, base);
    }
  }
  bn_block_fold(lds, s1, s2, t.rpb, t.row_off, t.lane_col, cols,
                slab + (size_t)blockIdx.x * 2 * cols);
}

// Second stage of the backward reduction (grid = cols / kFinCh blocks):
// dgamma = sum(dym*xhat), dbeta = sum(dym); coefficients for the apply.
__global__ __launch_bounds__(kBlock) void bn_bwd_finalize_k(
    const float* __restrict__ slab, int G, const float* __restrict__ gamma,
    const float* __restrict__ save_rstd, float* __restrict__ dgamma,
    float* __restrict__ dbeta, float* __restrict__ c1,
    float* __restrict__ c2, float* __restrict__ c3, long long rows,
    int cols, int training) {
  __shared__ float red[kBlock / WAVE * 2 * kFinCh];
  float sum_dym, sum_dymxh;
  const int blk = bn_fin_block();
  bn_slab_sum(slab, G, cols, blk, red, sum_dym, sum_dymxh);
  if (threadIdx.x >= kFinCh) return;
  const int c = blk * kFinCh + threadIdx.x;
  dgamma[c] = sum_dymxh;
  dbeta[c] = sum_dym;
  c1[c] = gamma[c] * save_rstd[c];
  if (training) {
    c2[c] = sum_dym / rows;
    c3[c] = sum_dymxh / rows;
  } else {
    c2[c] = 0.f;  // eval mode: stats are constants
    c3[c] = 0.f;
  }
}

// dx = c1*(dym - c2 - xhat*c3); optional dres = dym.
template <class Src, bool RES>
__global__ __launch_bounds__(kBlock) void bn_bwd_apply_k(
    const short* __restrict__ x, const unsigned char* __restrict__ bytes,
    const short* __restrict__ ga, const short* __restrict__ gb,
    short* __restrict__ s, PoolGeom g,
    const float* __restrict__ save_mean,
    const float* __restrict__ save_rstd, const float* __restrict__ c1,
    const float* __restrict__ c2, const float* __restrict__ c3,
    short* __restrict__ dx, short* __restrict__ dres, long long rows,
    int cols) {
  static_assert(!Src::kStores, "only the reduce kernel writes a row back");
  const Src src = Src::make(bytes, ga, gb, s, g);
  const BnGeom t = bn_geom(cols);
  if (t.row_off >= t.rpb) return;
  const Chan8 mean = bn_chan8(save_mean + t.lane_col);
  const Chan8 rstd = bn_chan8(save_rstd + t.lane_col);
  const Chan8 k1 = bn_chan8(c1 + t.lane_col);
  const Chan8 k2 = bn_chan8(c2 + t.lane_col);
  const Chan8 k3 = bn_chan8(c3 + t.lane_col);

  for (long long r = (long long)blockIdx.x * t.rpb + t.row_off; r < rows;
       r += (long long)gridDim.x * t.rpb) {
    const long long base = r * cols + t.lane_col;
    const short8 xv = *(const short8*)(x + base);
    typename Src::Row row = src.load(base, r, cols, t.lane_col);
    short8 odx, odr;
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      const float d = src.eval(row, j);
      const float xh = bn_xhat(xv[j], mean[j], rstd[j]);
      odx[j] = f2bf(bn_dx(d, xh, k1[j], k2[j], k3[j]));
      if (RES) odr[j] = f2bf(d);
    }
    *(short8*)(dx + base) = odx;
    if (RES) *(short8*)(dres + base) = odr;
  }
}

// --------------------------------------------------------------------
// BN + ReLU + MaxPool2d(3, stride 2, pad 1, floor mode), fused
// --------------------------------------------------------------------
// x is [N*H*W, C], the pooled tensors are [N*Ho*Wo, C] with
// Ho = (H-1)/2 + 1, Wo = (W-1)/2 + 1. Row numbers fit 32 bits (checked
// by the launchers), element offsets are 64-bit.

typedef unsigned uint2v __attribute__((ext_vector_type(2)));

// Code of a window whose maximum gets no gradient through the ReLU.
constexpr unsigned kPoolDead = 9;
// Never stored: what a window that does not exist is compared against.
constexpr unsigned kPoolNone = 0xffu;

// pooled = maxpool(relu(scale*x + shift)), one thread per output pixel
// and 8 channels. Every tap is computed and rounded to bf16 as
// bn_apply_k does before it is compared; the winner is the first
// maximum in scan order (kh outer, kw inner, strict >, taps outside
// the image skipped), as in ATen's NHWC kernel. code = winning tap
// kh*3+kw, or kPoolDead where bn_apply_k would clear the winner's mask
// bit (f > 0 is false).
//
// Blocks take rows in launch order, like the plain kernels. Dealing
// each XCD a contiguous range of blocks (bn_fin_block), so that the
// rows shared by neighbouring blocks come from one L2, measured 1-2 %
// slower over the forward chain and over forward+backward
// (profiles/README.md, "Round 5").
__global__ __launch_bounds__(kBlock) void bn_apply_pool_k(
    const short* __restrict__ x, const float* __restrict__ scale,
    const float* __restrict__ shift, short* __restrict__ pooled,
    unsigned char* __restrict__ code, long long orows, int cols,
    PoolGeom g) {
  const BnGeom t = bn_geom(cols);
  if (t.row_off >= t.rpb) return;
  const Chan8 sc = bn_chan8(scale + t.lane_col);
  const Chan8 sh = bn_chan8(shift + t.lane_col);
  const unsigned opix = (unsigned)(g.Ho * g.Wo);

  for (long long o = (long long)blockIdx.x * t.rpb + t.row_off; o < orows;
       o += (long long)gridDim.x * t.rpb) {
    const unsigned n = (unsigned)o / opix;
    const unsigned rem = (unsigned)o - n * opix;
    const int oh = (int)(rem / (unsigned)g.Wo);
    const int ow = (int)(rem - (unsigned)oh * (unsigned)g.Wo);
    // all 9 loads issued before the first use; a tap outside the image
    // reads the clamped (in-image) pixel and is not compared
    short8 v[9];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int ih = min(max(2 * oh - 1 + kh, 0), g.H - 1);
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int iw = min(max(2 * ow - 1 + kw, 0), g.W - 1);
        const long long r = ((long long)n * g.H + ih) * g.W + iw;
        v[kh * 3 + kw] = *(const short8*)(x + r * cols + t.lane_col);
      }
    }
    float best[kVec], bestf[kVec];
    unsigned tap[kVec];
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      best[j] = -INFINITY;
      bestf[j] = 0.f;
      tap[j] = 0;
    }
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int ih = 2 * oh - 1 + kh;
      const bool hin = ih >= 0 && ih < g.H;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int iw = 2 * ow - 1 + kw;
        const bool in = hin && iw >= 0 && iw < g.W;
#pragma unroll
        for (int j = 0; j < kVec; ++j) {
          const float f = bn_affine(v[kh * 3 + kw][j], sc[j], sh[j]);
          const float q = bf2f(f2bf(fmaxf(f, 0.f)));
          // a branch, not selects: most taps replace no maximum, and
          // the branch-free form measured slower (stem forward chain
          // 586 against 510 us)
          if (in && q > best[j]) {
            best[j] = q;
            bestf[j] = f;
            tap[j] = kh * 3 + kw;
          }
        }
      }
    }
    short8 ov;
    unsigned c0 = 0, c1 = 0;
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      union { float f; unsigned u; } b;
      b.f = best[j];  // a bf16 value: the low half is zero
      ov[j] = (short)(b.u >> 16);
      const unsigned c = bestf[j] > 0.f ? tap[j] : kPoolDead;
      if (j < 4) c0 |= c << (8 * j);
      else c1 |= c << (8 * (j - 4));
    }
    const long long base = o * cols + t.lane_col;
    *(short8*)(pooled + base) = ov;
    *(uint2v*)(code + base) = uint2v{c0, c1};
  }
}

// The pooled gradients and codes of the up to 2x2 windows that contain
// input pixel r, loaded before any is used. Windows that do not exist
// (even ih or iw, or past the last pooled row/column) load the first
// window again and are given kPoolNone to match against.
struct PoolTaps {
  short8 dy[4];
  uint2v code[4];
  unsigned want[4];
};

__device__ __forceinline__ PoolTaps bn_pool_taps(
    const short* __restrict__ dyp, const unsigned char* __restrict__ code,
    long long r, int cols, int lane_col, const PoolGeom& g) {
  const unsigned ipix = (unsigned)(g.H * g.W);
  const unsigned n = (unsigned)r / ipix;
  const unsigned rem = (unsigned)r - n * ipix;
  const int ih = (int)(rem / (unsigned)g.W);
  const int iw = (int)(rem - (unsigned)ih * (unsigned)g.W);
  // window oh0 = ih/2 sees row ih as tap 1 (ih even) or 2 (ih odd); an
  // odd row is also tap 0 of window oh0+1, if that window exists
  const int oh0 = ih >> 1, ow0 = iw >> 1;
  const unsigned kh0 = 1 + (ih & 1), kw0 = 1 + (iw & 1);
  const bool h2 = (ih & 1) && oh0 + 1 < g.Ho;
  const bool w2 = (iw & 1) && ow0 + 1 < g.Wo;
  PoolTaps t;
  // oh ascending, then ow ascending: ATen's order of accumulation
#pragma unroll
  for (int a = 0; a < 2; ++a) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const bool on = (a == 0 || h2) && (b == 0 || w2);
      const int oh = on ? oh0 + a : oh0;
      const int ow = on ? ow0 + b : ow0;
      const long long base =
          (((long long)n * g.Ho + oh) * g.Wo + ow) * cols + lane_col;
      t.dy[a * 2 + b] = *(const short8*)(dyp + base);
      t.code[a * 2 + b] = *(const uint2v*)(code + base);
      t.want[a * 2 + b] =
          on ? (a ? 0u : kh0) * 3 + (b ? 0u : kw0) : kPoolNone;
    }
  }
  return t;
}

// dym of the pixel: fp32 sum of the pooled gradients whose code names
// it, rounded to bf16, which is the dy * mask that the unfused chain
// hands to bn_bwd_reduce_k / bn_bwd_apply_k.
__device__ __forceinline__ float bn_pool_dym(const PoolTaps& t, int j) {
  float d = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const unsigned c =
        ((j < 4 ? t.code[w][0] : t.code[w][1]) >> (8 * (j & 3))) & 0xffu;
    if (c == t.want[w]) d += bf2f(t.dy[w][j]);
  }
  return bf2f(f2bf(d));
}

// dym gathered from the pooled gradient instead of loaded: the source
// of the stem's backward (DySrc<true> of the unfused chain).
struct PoolSrc {
  static constexpr bool kStores = false;
  const unsigned char* code;
  const short* dyp;
  PoolGeom g;
  static __device__ __forceinline__ PoolSrc make(
      const unsigned char* code, const short* dyp, const short*, short*,
      const PoolGeom& g) {
    return {code, dyp, g};
  }
  using Row = PoolTaps;
  __device__ __forceinline__ Row load(long long, long long r, int cols,
                                      int lane_col) const {
    return bn_pool_taps(dyp, code, r, cols, lane_col, g);
  }
  __device__ __forceinline__ float eval(const Row& t, int j) const {
    return bn_pool_dym(t, j);
  }
};

long long bn_row_blocks(long long rows, int cols) {
  const int rpb = bn_rows_per_block(cols);
  return (rows + rpb - 1) / rpb;
}

int bn_grid(long long rows, int cols) {
  return (int)min(bn_row_blocks(rows, cols), 2048LL);
}

}  // namespace

// Reduce grid = slab rows; the rule is derived in the header comment.
int bn_reduce_blocks(long long rows, int cols) {
  const long long g = max(256LL, min(512LL, rows / 64));
  return (int)max(1LL, min(bn_row_blocks(rows, cols), g));
}

// Scratch of one chain: the slab [G][2C], then the per-channel
// coefficients, [C] each: scale, shift forward; c1, c2, c3 backward.
long long bn_scratch_floats(long long rows, int cols) {
  return (long long)bn_reduce_blocks(rows, cols) * 2 * cols + 3LL * cols;
}
static float* bn_scratch_coef(float* scratch, int G, int cols) {
  return scratch + (size_t)G * 2 * cols;
}

static void bn_finalize(const float* slab, int G, const float* gamma,
                        const float* beta, float* running_mean,
                        float* running_var, float* save_mean,
                        float* save_rstd, float* coef, long long rows,
                        int cols, float momentum, float eps, bool training,
                        hipStream_t stream) {
  hipLaunchKernelGGL(bn_finalize_k, dim3(cols / kFinCh), dim3(kBlock), 0,
                     stream, slab, G, gamma, beta, running_mean,
                     running_var, save_mean, save_rstd, coef, coef + cols,
                     rows, cols, momentum, eps, (int)training);
}

// Statistics (training only) and finalize over scratch; returns the
// coefficients: scale [C], then shift [C].
static float* bn_stats_finalize(const short* x, const float* gamma,
                                const float* beta, float* running_mean,
                                float* running_var, float* save_mean,
                                float* save_rstd, float* scratch,
                                long long rows, int cols, float momentum,
                                float eps, bool training,
                                hipStream_t stream) {
  const int G = bn_reduce_blocks(rows, cols);
  if (training)
    hipLaunchKernelGGL(bn_stats_k<kUnroll>, dim3(G), dim3(kBlock), 0,
                       stream, x, scratch, rows, cols);
  float* coef = bn_scratch_coef(scratch, G, cols);
  bn_finalize(scratch, G, gamma, beta, running_mean, running_var,
              save_mean, save_rstd, coef, rows, cols, momentum, eps,
              training, stream);
  return coef;
}

static void bn_apply(const short* x, const short* res, const float* coef,
                     short* y, unsigned char* mask, long long rows,
                     int cols, bool relu, hipStream_t stream) {
  auto ap = relu ? (res ? bn_apply_k<true, true> : bn_apply_k<true, false>)
                 : (res ? bn_apply_k<false, true>
                        : bn_apply_k<false, false>);
  hipLaunchKernelGGL(ap, dim3(bn_grid(rows, cols)), dim3(kBlock), 0, stream,
                     x, res, coef, coef + cols, y, mask, rows, cols);
}

// What a source is made of (Src::make), as the launchers hold it.
struct BnSrcArgs {
  const unsigned char* bytes;
  const short* ga;
  const short* gb;
  short* s;
  PoolGeom g;
};

// reduce over source RSrc of r -> finalize -> apply (the kernel ak,
// over its source of a).
template <class RSrc, class ApplyK>
static void bn_bwd_chain(const short* x, const BnSrcArgs& r,
                         const BnSrcArgs& a, ApplyK ak, const float* gamma,
                         const float* save_mean, const float* save_rstd,
                         float* scratch, float* dgamma, float* dbeta,
                         short* dx, short* dres, long long rows, int cols,
                         bool training, hipStream_t stream) {
  const int G = bn_reduce_blocks(rows, cols);
  hipLaunchKernelGGL((bn_bwd_reduce_k<RSrc, kUnroll>), dim3(G),
                     dim3(kBlock), 0, stream, x, r.bytes, r.ga, r.gb,
                     r.s, r.g, save_mean, save_rstd, scratch, rows, cols);
  float* c1 = bn_scratch_coef(scratch, G, cols);
  float* c2 = c1 + cols;
  float* c3 = c2 + cols;
  hipLaunchKernelGGL(bn_bwd_finalize_k, dim3(cols / kFinCh), dim3(kBlock),
                     0, stream, scratch, G, gamma, save_rstd, dgamma, dbeta,
                     c1, c2, c3, rows, cols, (int)training);
  hipLaunchKernelGGL(ak, dim3(bn_grid(rows, cols)), dim3(kBlock), 0, stream,
                     x, a.bytes, a.ga, a.gb, a.s, a.g, save_mean, save_rstd,
                     c1, c2, c3, dx, dres, rows, cols);
}

void launch_bn_fwd(const short* x, const short* res, const float* gamma,
                   const float* beta, float* running_mean,
                   float* running_var, float* save_mean, float* save_rstd,
                   float* scratch, short* y, unsigned char* mask,
                   long long rows, int cols, float momentum, float eps,
                   bool training, bool relu, hipStream_t stream) {
  const float* coef = bn_stats_finalize(
      x, gamma, beta, running_mean, running_var, save_mean, save_rstd,
      scratch, rows, cols, momentum, eps, training, stream);
  bn_apply(x, res, coef, y, mask, rows, cols, relu, stream);
}

void launch_bn_fwd_slab(const short* x, const short* res,
                        const float* slab, int G, const float* gamma,
                        const float* beta, float* running_mean,
                        float* running_var, float* save_mean,
                        float* save_rstd, float* coef, short* y,
                        unsigned char* mask, long long rows, int cols,
                        float momentum, float eps, bool relu,
                        hipStream_t stream) {
  // the slab's G rows come from the caller's kernel
  bn_finalize(slab, G, gamma, beta, running_mean, running_var, save_mean,
              save_rstd, coef, rows, cols, momentum, eps, true, stream);
  bn_apply(x, res, coef, y, mask, rows, cols, relu, stream);
}

void launch_bn_bwd(const short* x, const unsigned char* mask,
                   const short* dy, const float* gamma,
                   const float* save_mean, const float* save_rstd,
                   float* scratch, float* dgamma, float* dbeta, short* dx,
                   short* dres, long long rows, int cols, bool training,
                   bool relu, hipStream_t stream) {
  const BnSrcArgs a{mask, dy, nullptr, nullptr, {}};
  auto run = [&](auto src) {
    using S = decltype(src);
    bn_bwd_chain<S>(x, a, a, dres ? bn_bwd_apply_k<S, true>
                                   : bn_bwd_apply_k<S, false>,
                    gamma, save_mean, save_rstd, scratch, dgamma, dbeta, dx,
                    dres, rows, cols, training, stream);
  };
  if (relu) run(DySrc<true>{});
  else run(DySrc<false>{});
}

void launch_bn_bwd2(const short* x, const unsigned char* mask,
                    const short* dya, const short* dyb, const float* gamma,
                    const float* save_mean, const float* save_rstd,
                    float* scratch, float* dgamma, float* dbeta, short* dx,
                    short* s, long long rows, int cols, bool training,
                    bool relu, hipStream_t stream) {
  // the apply reads s, already masked, as its dy and stores no dres
  using A = DySrc<false>;
  const BnSrcArgs r{mask, dya, dyb, s, {}};
  const BnSrcArgs a{nullptr, s, nullptr, nullptr, {}};
  auto run = [&](auto src) {
    bn_bwd_chain<decltype(src)>(x, r, a, bn_bwd_apply_k<A, false>, gamma,
                                save_mean, save_rstd, scratch, dgamma,
                                dbeta, dx, nullptr, rows, cols, training,
                                stream);
  };
  if (relu) run(SumSrc<true>{});
  else run(SumSrc<false>{});
}

void launch_bn_pool_fwd(const short* x, const float* gamma,
                        const float* beta, float* running_mean,
                        float* running_var, float* save_mean,
                        float* save_rstd, float* scratch, short* pooled,
                        unsigned char* code, int n, int h, int w, int cols,
                        float momentum, float eps, bool training,
                        hipStream_t stream) {
  const PoolGeom g{h, w, (h - 1) / 2 + 1, (w - 1) / 2 + 1};
  const long long rows = (long long)n * h * w;
  const long long orows = (long long)n * g.Ho * g.Wo;
  const float* coef = bn_stats_finalize(
      x, gamma, beta, running_mean, running_var, save_mean, save_rstd,
      scratch, rows, cols, momentum, eps, training, stream);
  hipLaunchKernelGGL(bn_apply_pool_k, dim3(bn_grid(orows, cols)),
                     dim3(kBlock), 0, stream, x, coef, coef + cols, pooled,
                     code, orows, cols, g);
}

void launch_bn_pool_bwd(const short* x, const unsigned char* code,
                        const short* dyp, const float* gamma,
                        const float* save_mean, const float* save_rstd,
                        float* scratch, float* dgamma, float* dbeta,
                        short* dx, int n, int h, int w, int cols,
                        bool training, hipStream_t stream) {
  const PoolGeom g{h, w, (h - 1) / 2 + 1, (w - 1) / 2 + 1};
  const long long rows = (long long)n * h * w;
  const BnSrcArgs a{code, dyp, nullptr, nullptr, g};
  bn_bwd_chain<PoolSrc>(x, a, a, bn_bwd_apply_k<PoolSrc, false>, gamma,
                        save_mean, save_rstd, scratch, dgamma, dbeta, dx,
                        nullptr, rows, cols, training, stream);
}
