// Read-once 1x1 convolution forward with the BatchNorm statistics folded
// into its epilogue: C[M,N] = A[M,K] @ W[N,K]^T (bf16 in, fp32
// accumulate, bf16 out) plus, per workgroup, one row of the fp32 slab
// [G][2N] that bn_finalize_k reads: [0..N) column sums and [N..2N) column
// sums of squares of the STORED bf16 values. bn_stats_k's pass over the
// convolution output disappears at the sites that run this kernel.
//
// gemm_stream_k gives a workgroup one 64-wide N-block, so A is fetched
// N/64 times, by workgroups on different XCDs (separate L2s). Here a
// workgroup owns rows and covers NB = 64*NCH columns, all of N where the
// W panel fits (NB*K*2 <= 128 KiB of the 160 KiB LDS):
//
//   - W panel [NB][K] staged once per workgroup, swizzled as in
//     gemm_stream_k;
//   - the unit of work is a block of R rows of ONE WAVE: its A fragments
//     for the whole of K are loaded from global memory once into
//     registers (R*K/128 VGPRs) and reused for every 64-column chunk;
//   - per chunk: R/16 x 4 MFMA accumulators, B fragments from LDS, then
//     16 rows at a time through the wave's private 2 KiB bounce: bf16
//     stores to LDS in C-fragment layout, row-contiguous 16 B global
//     stores, and a column read-back (lane l reads column l of the 16
//     rows) that adds v and v*v of the stored bf16 into two registers
//     per chunk. The statistics cost 2*NCH VGPRs, where accumulating in
//     C-fragment layout would cost NB/8;
//   - no barrier in the main loop: the 16 waves free-run over their own
//     row blocks, which hides the global latency of the A fragments;
//   - rows are split contiguously over all G*16 waves of an N-block
//     (block q*nblk/Q .. (q+1)*nblk/Q), so a workgroup carries at most
//     16 row blocks more than the mean;
//   - the end folds the 16 waves' partials through LDS (the W panel is
//     dead by then) in wave order and writes the slab row with plain
//     stores. No float atomics; every slab row is fully written by every
//     call (a wave without rows contributes zeros), so the slab is
//     neither zeroed nor reused across calls.
//
// Where N > NB the N-blocks of the same rows are placed on one XCD
// (consecutive workgroup ids are dealt round-robin to the 8 XCDs) so
// that A comes from HBM once and from that L2 afterwards. Only a
// placement hint: the mapping is a bijection either way.

#include "mfma_tile.hip.h"
#include "kernels.h"

namespace {

constexpr int CTHREADS = 1024;
constexpr int CWAVES = CTHREADS / 64;
constexpr int CCH = 64;          // columns per chunk
constexpr int kMaxPanel = 128 * 1024;
constexpr int kCUs = 256;

// Orders the wave's own LDS traffic for the compiler: lanes exchange
// data through the bounce without a workgroup barrier (the hardware
// executes one wave's LDS instructions in order).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int K, int R, int NCH>
__global__ __launch_bounds__(CTHREADS) void conv1x1_stats_k(
    const short* __restrict__ A, const short* __restrict__ W,
    short* __restrict__ C, float* __restrict__ slab, long long M, int N,
    int G) {
  constexpr int NB = NCH * CCH;
  constexpr int RI = R / 16;
  constexpr int NTK = K / 32;
  constexpr int row_shift = K == 64 ? 7 : (K == 128 ? 8 : 9);
  static_assert(NB * K * 2 <= kMaxPanel, "W panel exceeds its LDS share");
  static_assert(CWAVES * 2 * NB * 4 <= NB * K * 2, "fold tile fits panel");
  static_assert(2 * NB <= CTHREADS, "one thread per slab-row entry");
  __shared__ __attribute__((aligned(16))) short lW[NB * K];
  __shared__ __attribute__((aligned(16))) short lC[CWAVES * 16 * CCH];

  const int nnb = N / NB;
  int g, nbk;
  if (G % 8 == 0) {
    nbk = (blockIdx.x / 8) % nnb;
    g = (blockIdx.x / (8 * nnb)) * 8 + blockIdx.x % 8;
  } else {
    nbk = blockIdx.x % nnb;
    g = blockIdx.x / nnb;
  }

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const FragLane fl(lane);

  // stage the W panel once; pre-permuted source so that the swizzled
  // fragment reads see linear data
  for (int e0 = tid * 8; e0 < NB * K; e0 += CTHREADS * 8) {
    const int e = tile_swz(e0 * 2, row_shift) / 2;
    const int row = e / K, kk = e % K;
    global_load_lds16(W + ((long long)nbk * NB + row) * K + kk,
                      lW + (e0 - lane * 8));  // wave-uniform base
  }
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();

  float s[NCH], ss[NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) s[ch] = ss[ch] = 0.f;

  const long long nblk = (M + R - 1) / R;
  const long long Q = (long long)G * CWAVES;
  const long long q = (long long)g * CWAVES + wave;
  const long long b0 = q * nblk / Q, b1 = (q + 1) * nblk / Q;
  short* myC = lC + wave * (16 * CCH);

  for (long long blk = b0; blk < b1; ++blk) {
    const long long m0 = blk * R;
    bf16x8 a[RI][NTK];
#pragma unroll
    for (int i = 0; i < RI; ++i) {
      long long row = m0 + i * 16 + fl.frag_row;
      if (row >= M) row = M - 1;  // clamped; stores and sums predicated
#pragma unroll
      for (int ks = 0; ks < NTK; ++ks)
        a[i][ks] = *(const bf16x8*)(A + row * K + ks * 32 + fl.frag_k);
    }

    // not unrolled: one chunk's fragments and accumulators live at a time
#pragma unroll 1
    for (int ch = 0; ch < NCH; ++ch) {
      const short* lWc = lW + ch * (CCH * K);  // whole swizzle periods
      f32x4 acc[RI][4];
#pragma unroll
      for (int i = 0; i < RI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

#pragma unroll
      for (int ks = 0; ks < NTK; ++ks) {
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bf16x8 b = *(const bf16x8*)(
              (const char*)lWc +
              tile_swz(((j * 16 + fl.frag_row) * K + ks * 32 + fl.frag_k) * 2,
                       row_shift));
#pragma unroll
          for (int i = 0; i < RI; ++i)
            acc[i][j] = mfma_bf16(a[i][ks], b, acc[i][j]);
        }
        __builtin_amdgcn_s_setprio(0);
      }

#pragma unroll
      for (int i = 0; i < RI; ++i) {
        wave_lds_sync();  // the previous read-back is done
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int rr = 0; rr < 4; ++rr)
            myC[(fl.c_sub_row + rr) * CCH + j * 16 + fl.c_col] =
                f2bf(acc[i][j][rr]);
        wave_lds_sync();
        const long long gr0 = m0 + i * 16;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int r = t * 8 + lane / 8;
          const int c = (lane % 8) * 8;
          const long long grow = gr0 + r;
          if (grow < M) {
            const bf16x8 v = *(const bf16x8*)&myC[r * CCH + c];
            *(bf16x8*)&C[grow * N + (long long)nbk * NB + ch * CCH + c] = v;
          }
        }
        // statistics over the stored values of the rows < M
        const long long left = M - gr0;
        const int nvalid = left >= 16 ? 16 : (left > 0 ? (int)left : 0);
        float t1 = 0.f, t2 = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (r < nvalid) {
            const float v = bf2f(myC[r * CCH + lane]);
            t1 += v;
            t2 += v * v;
          }
        }
        // ch is a loop variable: select the chunk's registers
#pragma unroll
        for (int c2 = 0; c2 < NCH; ++c2) {
          s[c2] += c2 == ch ? t1 : 0.f;
          ss[c2] += c2 == ch ? t2 : 0.f;
        }
      }
    }
  }

  // fold the waves in wave order; the W panel is dead after the barrier
  __syncthreads();
  float* red = (float*)lW;  // [CWAVES][2][NB]
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    red[(wave * 2 + 0) * NB + ch * CCH + lane] = s[ch];
    red[(wave * 2 + 1) * NB + ch * CCH + lane] = ss[ch];
  }
  __syncthreads();
  if (tid < 2 * NB) {
    const int half = tid / NB, c = tid % NB;
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < CWAVES; ++w) t += red[(w * 2 + half) * NB + c];
    slab[(size_t)g * 2 * N + (size_t)half * N + (size_t)nbk * NB + c] = t;
  }
}

// Rows of a wave's block: 32 where its A fragments (R*K/128 VGPRs), the
// accumulators (R) and the per-chunk sums (2*NCH) fit the 128 VGPRs of a
// 16-wave workgroup without scratch, else 16.
constexpr int rows_per_block(int K, int nch) {
  return K == 256 || (K == 128 && nch >= 4) ? 16 : 32;
}

template <int K, int NCH>
void launch_one(const short* A, const short* W, short* C, float* slab,
                long long M, int N, int G, hipStream_t stream) {
  const int nnb = N / (NCH * CCH);
  hipLaunchKernelGGL((conv1x1_stats_k<K, rows_per_block(K, NCH), NCH>),
                     dim3(G * nnb), dim3(CTHREADS), 0, stream, A, W, C,
                     slab, M, N, G);
}

template <int K>
void launch_k(int nch, const short* A, const short* W, short* C,
              float* slab, long long M, int N, int G, hipStream_t stream) {
  if constexpr (K * 8 * CCH * 2 <= kMaxPanel) {
    if (nch == 8)
      return launch_one<K, 8>(A, W, C, slab, M, N, G, stream);
  }
  if (nch == 4) return launch_one<K, 4>(A, W, C, slab, M, N, G, stream);
  if (nch == 2) return launch_one<K, 2>(A, W, C, slab, M, N, G, stream);
  launch_one<K, 1>(A, W, C, slab, M, N, G, stream);
}

}  // namespace

bool conv1x1_stats_supported(long long M, int N, int K) {
  return (K == 64 || K == 128 || K == 256) && N >= CCH && N % CCH == 0 &&
         M >= 1;
}

// Launch plan, mirrored by tests/ops/_conv1x1_stats.py.
//   nch: the widest of 8, 4, 2, 1 chunks whose N-block divides N and
//        whose W panel fits 128 KiB.
//   G:   one workgroup per CU over all N-blocks, in multiples of 8 (the
//        XCD placement), but at most one workgroup per 16 full row
//        blocks: a workgroup then sums >= 256 rows, so the slab
//        (16*G*N bytes written and read back) stays below 1/8 of the
//        output. max_workers > 0 lowers G further (tests reach the
//        multi-trip loop at a few thousand rows with it).
void conv1x1_stats_plan(long long M, int N, int K, int max_workers,
                        int* nch, int* G) {
  int c = 8;
  while (c > 1 && (N % (c * CCH) != 0 || c * CCH * K * 2 > kMaxPanel))
    c /= 2;
  const int nnb = N / (c * CCH);
  const int R = rows_per_block(K, c);
  long long g = kCUs / nnb / 8 * 8;
  if (g < 8) g = 8;
  const long long by_rows = M / ((long long)CWAVES * R);
  if (g > by_rows) g = by_rows;
  if (g < 1) g = 1;
  if (max_workers > 0 && g > max_workers) g = max_workers;
  *nch = c;
  *G = (int)g;
}

void launch_conv1x1_stats(const short* A, const short* W, short* C,
                          float* slab, long long M, int N, int K,
                          int max_workers, hipStream_t stream) {
  int nch, G;
  conv1x1_stats_plan(M, N, K, max_workers, &nch, &G);
  if (K == 64)
    launch_k<64>(nch, A, W, C, slab, M, N, G, stream);
  else if (K == 128)
    launch_k<128>(nch, A, W, C, slab, M, N, G, stream);
  else
    launch_k<256>(nch, A, W, C, slab, M, N, G, stream);
}
