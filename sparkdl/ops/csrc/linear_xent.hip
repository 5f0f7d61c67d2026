// Fused vocabulary projection + cross-entropy (the BERT MLM loss):
//
//   loss[row] = logsumexp_col(z[row, :]) - z[row, labels[row]],
//   z = h[M,K] @ W[V,K]^T + bias[V]   (bf16 operands, fp32 z)
//
// z is never written to memory. lce_k<PASS> is one MFMA main loop with
// two epilogues over the fp32 accumulators:
//
//   PASS 0 (forward)  per 256-column vocabulary tile and row, the pair
//                     (max, sum exp(z - max)) -> ws[tile][row], and the
//                     label's logit -> zlab[row]
//   PASS 1 (backward) z again by the identical instruction sequence (so
//                     bit for bit the forward's z), then
//                     d = (exp(z - lse[row]) - [col == label]) * g[row]
//                     -> dZ bf16, and the fp32 column sums of d
//                     -> slab[band][col] for dbias
//
// Main loop: the geometry of gemm_bias_act_k (gemm_gelu.hip): 256x256
// tile, K-step 64, 16 waves 4x4, 4x4 fragments of
// v_mfma_f32_16x16x32_bf16 per wave, 128 KiB double-buffered swizzled
// LDS staged with global_load_lds16, source rows clamped at the M and V
// edges. The loop is written out here and not shared with that kernel,
// so that kernel's instruction stream stays what was measured.
//
// Grid: (row bands) x (vocabulary tiles) in one dimension, the row band
// the fast index of the xcd_remap'ed id: the workgroups that share one
// 384 KB tile of W (K = 768) run together on one XCD, W streams from
// HBM about once and h is re-read from cache.
//
// Forward epilogue, per lane: its 16 rows, 4 columns (j fragments) each;
// max and sum first over j, then over the 16 lanes of a fragment row by
// xor shuffles, then over the four column waves through LDS
// (red[row][wave], after the K loop). A wave whose 64 columns all lie
// beyond V holds (-inf, 0), which the fold below treats as the neutral
// element; column 0 of a tile is always valid, so a tile's max is
// finite.
//
// lce_rows_k folds the tiles of a row in order into lse and the per-row
// loss (0 on ignored rows, NaN for a label outside [0, V)); lce_total_k
// counts the valid rows and sums the losses in one block in a fixed
// order. No float atomics anywhere: every result is bitwise
// reproducible.
//
// Backward epilogue: per-row (lse, g, label) sit in LDS since the
// prologue (rows >= M: lse = +inf, g = 0, so d = 0 there and the clamped
// duplicate rows add nothing to the column sums). g = gout[row] /
// max(count, 1), all read through device pointers. d is rounded to
// bf16 into the freed K-loop LDS and leaves as row-contiguous 16 B
// stores; the row stride ldz of dZ is V rounded up to 64 elements, so
// every row is 16 B aligned (30522 % 8 == 2), and the padding columns
// are written as zeros. The column sums go lane (16 rows) -> the four
// lane groups by xor shuffles -> the four row waves through LDS.
// lce_dbias_k adds the bands in order.

#include <cmath>

#include "mfma_tile.hip.h"
#include "kernels.h"

// device code of this file is generated without packed fp32 instructions
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

constexpr int kBM = 256;
constexpr int kBN = 256;
constexpr int kBK = 64;
constexpr int kThreads = 1024;
constexpr size_t kTileLds = 2 * 2 * (size_t)kBM * kBK * sizeof(short);
// behind the tiles: rowlab int[256], rowlse float[256], rowg float[256],
// red float[2048] (forward float2[256][4], backward float[4][256])
constexpr size_t kLds = kTileLds + (3 * kBM + 2048) * sizeof(float);

template <int PASS>
__global__ __launch_bounds__(kThreads) void lce_k(
    const short* __restrict__ A, const short* __restrict__ W,
    const float* __restrict__ bias, const long long* __restrict__ labels,
    int M, int V, int K, long long ignore_index,
    float2* __restrict__ ws, float* __restrict__ zlab,        // PASS 0
    const float* __restrict__ lse, const float* __restrict__ gout,
    int gstride, const int* __restrict__ count,               // PASS 1
    short* __restrict__ dZ, int ldz, float* __restrict__ slab) {
  extern __shared__ short lds[];
  int* rowlab = (int*)((char*)lds + kTileLds);
  float* rowlse = (float*)(rowlab + kBM);
  float* rowg = rowlse + kBM;
  float* red = rowg + kBM;

  const int wgid = xcd_remap(blockIdx.x, gridDim.x);
  const int nbm = (M + kBM - 1) / kBM;
  const int band = wgid % nbm;  // fast: one W tile, all its row bands
  const int vt = wgid / nbm;
  const long long a_row0 = (long long)band * kBM;
  const int b_row0 = vt * kBN;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 2;  // 0..3 -> output rows [wr*64, +64)
  const int wc = wave & 3;   // 0..3 -> output cols [wc*64, +64)
  const FragLane fl(lane);

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  auto bufA = [&](int b) { return lds + (size_t)b * 2 * kBM * kBK; };
  auto bufB = [&](int b) { return lds + ((size_t)b * 2 + 1) * kBM * kBK; };

  // Stage one 256x64 operand tile: stage_tile<kThreads, 2> with the
  // source rows clamped to the operand's last row.
  auto stage = [&](short* ldst, const short* g, long long row0, int k0,
                   int ld, int nrows) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int e = tile_swz128((s * kThreads + tid) * 16) / 2;
      const int row = e / kBK, kk = e % kBK;
      long long grow = row0 + row;
      if (grow >= nrows) grow = nrows - 1;
      global_load_lds16(g + grow * (long long)ld + k0 + kk,
                        ldst + (s * kThreads + (tid & ~63)) * 8);
    }
  };

  stage(bufA(0), A, a_row0, 0, K, M);
  stage(bufB(0), W, b_row0, 0, K, V);

  // Per-row parameters of the epilogue, once per workgroup. lab == -1
  // matches no column: ignored rows, rows >= M, labels outside [0, V).
  if (tid < kBM) {
    const long long grow = a_row0 + tid;
    int lab = -1;
    float l = INFINITY, g = 0.f;
    if (grow < M) {
      const long long lb = labels[grow];
      const bool valid = lb != ignore_index;
      if (valid && lb >= 0 && lb < V) lab = (int)lb;
      if (PASS == 1) {
        l = lse[grow];
        if (valid) {
          const int cnt = count ? max(*count, 1) : 1;
          g = gout[grow * gstride] / (float)cnt;
        }
      }
    }
    rowlab[tid] = lab;
    if (PASS == 1) {
      rowlse[tid] = l;
      rowg[tid] = g;
    }
  }
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();

  int cur = 0;
  const int ntiles = K / kBK;
  for (int t = 0; t < ntiles; ++t) {
    if (t + 1 < ntiles) {
      stage(bufA(cur ^ 1), A, a_row0, (t + 1) * kBK, K, M);
      stage(bufB(cur ^ 1), W, b_row0, (t + 1) * kBK, K, V);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        a[i] = lds_frag(bufA(cur), wr * 64 + i * 16 + fl.frag_row,
                        ks * 32 + fl.frag_k);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        b[j] = lds_frag(bufB(cur), wc * 64 + j * 16 + fl.frag_row,
                        ks * 32 + fl.frag_k);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = mfma_bf16(a[i], b[j], acc[i][j]);
      __builtin_amdgcn_s_setprio(0);
    }
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    cur ^= 1;
  }

  // The epilogue's lane coordinates are derived again from an opaque
  // copy of tid: derived from tid itself, the compiler forms its row and
  // address values before the K loop and, at the 128-register budget,
  // spills one of them across it.
  int etid = tid;
  asm volatile("" : "+v"(etid));
  const int elane = etid & 63;
  const int ewr = etid >> 8, ewc = (etid >> 6) & 3;
  const int c_col = elane % 16, c_sub_row = (elane / 16) * 4;

  // This lane's four global columns and their bias.
  int col[4];
  float bv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    col[j] = b_row0 + ewc * 64 + j * 16 + c_col;
    bv[j] = (bias && col[j] < V) ? bias[col[j]] : 0.f;
  }

  if (PASS == 0) {
    float2* red2 = (float2*)red;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int row = ewr * 64 + i * 16 + c_sub_row + rr;
        const int lab = rowlab[row];
        float z[4];
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          z[j] = col[j] < V ? acc[i][j][rr] + bv[j] : -INFINITY;
          m = fmaxf(m, z[j]);
          if (col[j] == lab) zlab[a_row0 + row] = z[j];
        }
#pragma unroll
        for (int off = 1; off < 16; off <<= 1)
          m = fmaxf(m, __shfl_xor(m, off, WAVE));
        const float ms = m == -INFINITY ? 0.f : m;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) s += expf(z[j] - ms);
#pragma unroll
        for (int off = 1; off < 16; off <<= 1)
          s += __shfl_xor(s, off, WAVE);
        if (c_col == 0) red2[row * 4 + ewc] = make_float2(m, s);
      }
    __syncthreads();
    if (etid < kBM && a_row0 + etid < M) {
      float2 p[4];
      float m = -INFINITY;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        p[w] = red2[etid * 4 + w];
        m = fmaxf(m, p[w].x);
      }
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) s += p[w].y * expf(p[w].x - m);
      ws[(long long)vt * M + a_row0 + etid] = make_float2(m, s);
    }
  } else {
    float cs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int row = ewr * 64 + i * 16 + c_sub_row + rr;
        const int lab = rowlab[row];
        const float l = rowlse[row], g = rowg[row];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float p = expf(acc[i][j][rr] + bv[j] - l);
          const float d =
              col[j] < V ? (p - (col[j] == lab ? 1.f : 0.f)) * g : 0.f;
          cs[j] += d;
          lds[row * kBN + ewc * 64 + j * 16 + c_col] = f2bf(d);
        }
      }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      cs[j] += __shfl_xor(cs[j], 16, WAVE);
      cs[j] += __shfl_xor(cs[j], 32, WAVE);
      if (elane < 16) red[ewr * kBN + ewc * 64 + j * 16 + elane] = cs[j];
    }
    __syncthreads();
    if (etid < kBN && b_row0 + etid < ldz)
      slab[(long long)band * ldz + b_row0 + etid] =
          ((red[etid] + red[kBN + etid]) + red[2 * kBN + etid]) +
          red[3 * kBN + etid];
    // 1024 threads x 16 B = 32 rows per sweep; 8 sweeps for 256 rows.
    // ldz % 64 == 0: every row is 16 B aligned and no pack straddles ldz.
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int row = s * 32 + etid / 32;
      const long long grow = a_row0 + row;
      const int c = (etid % 32) * 8;
      if (grow < M && b_row0 + c < ldz)
        *(bf16x8*)&dZ[grow * ldz + b_row0 + c] =
            *(const bf16x8*)&lds[row * kBN + c];
    }
  }
}

// lse[row] from the row's ntn tile pairs, folded in tile order, and the
// per-row loss.
__global__ __launch_bounds__(256) void lce_rows_k(
    const float2* __restrict__ ws, const float* __restrict__ zlab,
    const long long* __restrict__ labels, float* __restrict__ loss,
    float* __restrict__ lse, int M, int V, int ntn, long long ignore_index) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= M) return;
  float m = -INFINITY;
  for (int t = 0; t < ntn; ++t) m = fmaxf(m, ws[(long long)t * M + row].x);
  float s = 0.f;
  for (int t = 0; t < ntn; ++t) {
    const float2 p = ws[(long long)t * M + row];
    s += p.y * expf(p.x - m);
  }
  const float l = m + logf(s);
  lse[row] = l;
  const long long lb = labels[row];
  loss[row] = lb == ignore_index ? 0.f
              : (lb >= 0 && lb < V) ? l - zlab[row]
                                    : NAN;
}

// One block: the number of rows that count and, for "sum" / "mean", the
// reduced loss; strided partials, then a tree, both in a fixed order.
__global__ __launch_bounds__(kThreads) void lce_total_k(
    const float* __restrict__ loss, const long long* __restrict__ labels,
    int M, long long ignore_index, int mean, int* __restrict__ count,
    float* __restrict__ total) {
  __shared__ float ss[kThreads];
  __shared__ int sc[kThreads];
  const int tid = threadIdx.x;
  float s = 0.f;
  int c = 0;
  for (int r = tid; r < M; r += kThreads) {
    s += loss[r];
    c += labels[r] != ignore_index;
  }
  ss[tid] = s;
  sc[tid] = c;
  __syncthreads();
  for (int off = kThreads / 2; off > 0; off >>= 1) {
    if (tid < off) {
      ss[tid] += ss[tid + off];
      sc[tid] += sc[tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) {
    count[0] = sc[0];
    if (total) total[0] = mean ? ss[0] / (float)max(sc[0], 1) : ss[0];
  }
}

__global__ __launch_bounds__(256) void lce_dbias_k(
    const float* __restrict__ slab, float* __restrict__ dbias, int bands,
    int ldz, int V) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= V) return;
  float s = 0.f;
  for (int b = 0; b < bands; ++b) s += slab[(long long)b * ldz + c];
  dbias[c] = s;
}

template <int PASS, typename... Args>
void launch_lce_k(int grid, hipStream_t stream, Args... args) {
  static const hipError_t lds_set = hipFuncSetAttribute(
      (const void*)&lce_k<PASS>, hipFuncAttributeMaxDynamicSharedMemorySize,
      (int)kLds);
  (void)lds_set;
  hipLaunchKernelGGL((lce_k<PASS>), dim3(grid), dim3(kThreads), kLds, stream,
                     args...);
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

bool lce_supported(long long M, long long V, long long K) {
  return K >= kBK && K % kBK == 0 && K < (1LL << 24) && M >= 1 &&
         M < (1LL << 31) - kBM && V >= 1 && V <= (1LL << 30) &&
         ((M + kBM - 1) / kBM) * ((V + kBN - 1) / kBN) < (1LL << 31);
}

int lce_bands(int M) { return (M + kBM - 1) / kBM; }
int lce_vtiles(int V) { return (V + kBN - 1) / kBN; }
int lce_ldz(int V) { return (V + 63) / 64 * 64; }

void launch_lce_forward(const short* h, const short* W, const float* bias,
                        const long long* labels, float2* ws, float* zlab,
                        float* loss, float* lse, int* count, float* total,
                        bool mean, int M, int V, int K,
                        long long ignore_index, hipStream_t stream) {
  const int ntn = lce_vtiles(V);
  launch_lce_k<0>(lce_bands(M) * ntn, stream, h, W, bias, labels, M, V, K,
                  ignore_index, ws, zlab, (const float*)nullptr,
                  (const float*)nullptr, 0, (const int*)nullptr,
                  (short*)nullptr, 0, (float*)nullptr);
  hipLaunchKernelGGL(lce_rows_k, dim3((M + 255) / 256), dim3(256), 0, stream,
                     (const float2*)ws, (const float*)zlab, labels, loss, lse,
                     M, V, ntn, ignore_index);
  hipLaunchKernelGGL(lce_total_k, dim3(1), dim3(kThreads), 0, stream,
                     (const float*)loss, labels, M, ignore_index, (int)mean,
                     count, total);
}

void launch_lce_backward(const short* h, const short* W, const float* bias,
                         const long long* labels, const float* lse,
                         const float* gout, int gstride, const int* count,
                         short* dZ, float* slab, float* dbias, int M, int V,
                         int K, long long ignore_index, hipStream_t stream) {
  const int bands = lce_bands(M), ldz = lce_ldz(V);
  launch_lce_k<1>(bands * lce_vtiles(V), stream, h, W, bias, labels, M, V, K,
                  ignore_index, (float2*)nullptr, (float*)nullptr, lse, gout,
                  gstride, count, dZ, ldz, slab);
  hipLaunchKernelGGL(lce_dbias_k, dim3((V + 255) / 256), dim3(256), 0, stream,
                     (const float*)slab, dbias, bands, ldz, V);
}
