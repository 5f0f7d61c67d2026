// Tile primitives of the 128-wide flash attention kernels, shared by
// attention_d128.hip and attention_gqa.hip: the [64][128] operand tile as
// two swizzled [64][64] half-tiles, its staging, its K-major fragment
// reads, the transposing ds_read_b64_tr_b16 fragment reads (described at
// the top of attention_d128.hip), the zero tile of the all-padding exit
// and the launch with 72 KiB of dynamic LDS.
//
// Include it after attention_kernels.hip.h and inside the including
// file's no-packed-fp32-ops attribute region.
#pragma once

#include "attention_kernels.hip.h"

namespace {

constexpr int D128 = 128;
constexpr int kOperandElems = 2 * TILE_ELEMS;  // [64][128] as two halves
// 2 buffers x 2 operands x [64][128] + one [64][64] round-trip tile
constexpr int kLds = (4 * kOperandElems + TILE_ELEMS) * 2;
static_assert(kLds <= 80 * 1024, "two workgroups fit a CU's LDS");

typedef __attribute__((address_space(3))) short4v* lds_b64_ptr;

__device__ __forceinline__ unsigned lds_addr(const short* p) {
  return (unsigned)(unsigned long long)(
      (const __attribute__((address_space(3))) short*)p);
}

// The lane's part in a transposing fragment read of a swizzled [64][64]
// half-tile (see the top of attention_d128.hip). Read i (0, 1) of the
// fragment at rows r0 .. r0+31, columns c0 .. c0+15 (r0 % 32 == 0,
// c0 % 16 == 0) takes 8 bytes of row r0 + 8g + 4i + lg/4, columns
// c0 + 4*(lg%4) .. +4. The row's low bits are 4i + lg/4 and the 16 B
// chunk of the columns is c0/8 + (lg%4)/2, so the swizzled byte offset is
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

// Stage one [64][128] bf16 operand tile as two swizzled half-tiles.
__device__ __forceinline__ void stage_tile128(short* dst, const short* g,
                                              long long stride, int tid) {
  stage_tile64(dst, g, stride, tid);
  stage_tile64(dst + TILE_ELEMS, g + 64, stride, tid);
}

// K-major fragment of K-step ks (0..3 over the 128-wide head dimension)
// of a staged [64][128] operand tile.
__device__ __forceinline__ bf16x8 lds_frag128(const short* tile, int row,
                                              int ks, int frag_k) {
  return lds_frag(tile + (ks >> 1) * TILE_ELEMS, row,
                  (ks & 1) * 32 + frag_k);
}

// VARLEN: zero a [64][128] tile (rows `stride` elements apart).
// 256 threads x 4 x 16 B.
__device__ __forceinline__ void zero_tile128(short* g, long long stride,
                                             int tid) {
  const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  short* p = g + (long long)(tid / 4) * stride + (tid % 4) * 32;
#pragma unroll
  for (int c = 0; c < 4; ++c) *(bf16x8*)(p + c * 8) = z;
}

// One launch of KERNEL with the 72 KiB of dynamic LDS it needs.
template <auto KERNEL, typename... Args>
void launch_d128(dim3 grid, hipStream_t stream, Args... args) {
  static const hipError_t lds_set = hipFuncSetAttribute(
      (const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, kLds);
  (void)lds_set;
  hipLaunchKernelGGL(KERNEL, grid, dim3(ATHREADS), kLds, stream, args...);
}

}  // namespace
