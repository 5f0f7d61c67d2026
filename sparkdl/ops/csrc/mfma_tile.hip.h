// Shared MFMA tile vocabulary for the bf16 GEMM and attention kernels
// (gemm_gelu.hip, gemm_stream.hip, wgrad.hip, attention.hip): vector
// types, lane -> fragment coordinates, the st_16x32 LDS swizzle, the
// width-16 global_load_lds staging and the swizzled fragment read.
// Device-only; every helper inlines to the arithmetic it names.
//
// MFMA fragment layout for mfma_f32_16x16x32_bf16 (HW-verified), with
// both operands K-major (A[row][k], B[col][k]):
//   A-operand: lane l holds A[row = l%16][k = 8*(l/16) .. +8]
//   B-operand: lane l holds B[col = l%16][k = 8*(l/16) .. +8]
//   C/D:       lane l reg r holds C[row = (l/16)*4 + r][col = l%16]
#pragma once

#include "common.hip.h"

typedef short8 bf16x8;   // 8 x bf16: one MFMA A/B operand, one 16 B access
typedef float4v f32x4;   // 4 x fp32: one MFMA C/D fragment

// Lane coordinates in the layout above. Operand fragments: row (or col)
// frag_row, k offset frag_k inside a 32-wide K-step. C/D fragments: rows
// c_sub_row .. +4 (one per register), column c_col.
struct FragLane {
  int frag_row, frag_k, c_sub_row, c_col;
  __device__ __forceinline__ explicit FragLane(int lane)
      : frag_row(lane % 16),
        frag_k((lane / 16) * 8),
        c_sub_row((lane / 16) * 4),
        c_col(lane % 16) {}
};

__device__ __forceinline__ f32x4 mfma_bf16(bf16x8 a, bf16x8 b, f32x4 acc) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
}

// st_16x32 XOR swizzle on a byte offset into a row-major bf16 tile whose
// rows are (1 << row_shift) bytes: XOR byte bits 4-6 with row bits 0-2.
// Involution; keeps 16 B chunks intact; kills the 16-way ds_read_b128
// bank conflict of a 16-lane column read.
__device__ __forceinline__ int tile_swz(int byte_off, int row_shift) {
  return byte_off ^ (((byte_off >> row_shift) & 7) << 4);
}
// [row][64] bf16 tiles: 128-byte rows.
__device__ __forceinline__ int tile_swz128(int byte_off) {
  return tile_swz(byte_off, 7);
}

// One width-16 global_load_lds: every lane names its own 16 B global
// source; the wave's 64 x 16 B land LINEARLY at the wave-uniform LDS
// address `lds_wave_base` (+ lane * 16 is implied by the hardware).
__device__ __forceinline__ void global_load_lds16(const short* g,
                                                  short* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) unsigned int*)g,
      (__attribute__((address_space(3))) unsigned int*)lds_wave_base, 16, 0,
      0);
}

// Stage a [SWEEPS * THREADS / 8][64] bf16 tile into swizzled LDS: SWEEPS
// cooperative global_load_lds16 calls x THREADS threads x 16 B. Source
// rows are `stride` elements apart. The LDS write is linear, so the
// swizzle is applied by pre-permuting the per-lane GLOBAL source with the
// involution the fragment reads apply.
template <int THREADS, int SWEEPS>
__device__ __forceinline__ void stage_tile(short* dst, const short* g,
                                           long long stride, int tid) {
#pragma unroll
  for (int s = 0; s < SWEEPS; ++s) {
    const int e = tile_swz128((s * THREADS + tid) * 16) / 2;
    global_load_lds16(g + (long long)(e / 64) * stride + e % 64,
                      dst + (s * THREADS + (tid & ~63)) * 8);
  }
}

// Swizzled 16 B fragment read: elements [row][kk .. +8] of a [row][64]
// bf16 tile staged by stage_tile.
__device__ __forceinline__ bf16x8 lds_frag(const short* tile, int row,
                                           int kk) {
  return *(const bf16x8*)((const char*)tile +
                          tile_swz128((row * 64 + kk) * 2));
}

// XCD-aware bijective workgroup remap of (blockIdx.x, gridDim.x): the
// hardware deals consecutive workgroup ids round-robin over the 8 XCDs
// (private L2s); this hands each XCD a contiguous run of logical ids.
__device__ __forceinline__ int xcd_remap(unsigned bid, unsigned grid) {
  const int nwg = grid;
  const int q = nwg / 8, r = nwg % 8;
  const int xcd = bid % 8, idx = bid / 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}
