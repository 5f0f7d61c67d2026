// 3x3 stride-1 pad-1 convolution, bf16 NHWC, as an implicit GEMM on
// mfma_f32_16x16x32_bf16 (the bottleneck conv2):
//
//   y[n,h,w,co] = sum_{kh,kw,ci} x[n,h+kh-1,w+kw-1,ci] * wt[co,kh,kw,ci]
//
// x [N,H,W,Cin], wt [Cout,3,3,Cin] (the memory of a channels_last
// [Cout,Cin,3,3] weight), y [N,H,W,Cout]; fp32 accumulation, zero padding,
// no bias, f2bf store. M = N*H*W, N = Cout, K = 9*Cin. The data gradient
// is the same kernel on dy with the taps flipped and the channel roles
// swapped, so conv3x3_k serves forward and dgrad. The weight gradient
// (conv3x3_wgrad_k, further down) runs on the same tiles and halo staging.
//
// gemm_stream_k's "A fragments straight from global" would fetch every
// input pixel nine times. Here the nine taps share one staged input halo:
//
// Geometry (conv3x3_plan)
//   - a tile is made of whole output rows: `rows` consecutive rows of one
//     image (a band; bands never cross an image, the last band of an image
//     may be short), or, where a whole image has at most 256 pixels,
//     `imgs` whole images. Bands are balanced: ceil(H / nbands) rows with
//     nbands = ceil(H / max rows). At most VMT = 256 output pixels and
//     VHALO = 416 halo pixels per tile: 4 rows at W=56 (224 px), 7 rows at
//     W=28 (196), one 14x14 image (196), five 7x7 images (245);
//   - one 64-wide block of output channels per workgroup (VBN);
//   - 4 waves; wave v owns pixel slots 64v .. 64v+63 of the tile as 4 M
//     fragments x 4 N fragments = 16 accumulator fragments. That grid
//     reads 8 operand fragments per 16 MFMAs, the lowest LDS traffic per
//     MFMA a 256x64 tile allows (8 waves of 2x4 read 6 per 8);
//   - workgroups are persistent: worker w of an N-block takes tiles
//     w, w + workers, ... of it.
//
// K loop: Cin in slices of VBK = 64 channels, 9 taps x 2 K-steps each.
// Per slice, staged with global_load_lds16 and single-buffered:
//   - the halo [imgs * (rows+2)][W+2] pixels x 64 channels: the tile's
//     rows plus one above and below, and one pad column at each end of
//     every row. Pixel p is the 128-byte row p, swizzled as tile_swz128
//     (16 B chunk index XOR p & 7). The A fragment of tap (kh,kw) for the
//     output pixel with halo index b is pixel b + kh*(W+2) + kw: one add
//     per tap, no masks. Border slots hold zeros written by plain LDS
//     stores: the pad columns once per launch, the rows outside the image
//     once per tile. They are never the target of a load; a lane of a
//     partly filled wave of a load is switched off, its address clamped;
//   - the weight slice as 9 tiles [64 co][64 ci], one per tap, each a
//     st_16x32 tile read with the usual swizzled B fragment read. With
//     Cin = 64 the slice is the whole panel and is staged once per
//     workgroup instead.
// Output pixels of a tile that do not exist (short band, fewer images,
// slots past rows*W) read whatever their halo slots hold; a row of A
// only reaches the same row of C, and those rows are not stored.
//
// LDS map (dynamic, 132 KiB of the 160 KiB of a CU):
//   [0, 53248)        halo, 416 pixels x 128 B
//   [53248, 126976)   weights, 9 x 8 KiB
//   [126976, 135168)  output bounce, 2 KiB per wave
// Two slices would need 248 KiB, so the slice is single-buffered: stage,
// barrier, 288 MFMAs per wave, barrier. One workgroup per CU.
//
// Registers: 64 accumulator + 32 A + 32 B operand registers per tap, 4
// halo bases, 8 B offsets; launch_bounds(256) allows 512. Measured use,
// scratch (0) and occupancy: profiles/README.md.
//
// Bank conflicts: the 16 lanes of an A read share one k chunk and hold 16
// consecutive output pixels, which are consecutive halo pixels except
// where the run wraps to the next row (+3). Eight consecutive pixels have
// eight different p & 7, so the XOR spreads them over the eight 16 B
// chunks of the 128-byte period: conflict-free like a st_16x32 column
// read. A run that wraps inside a group of eight repeats at most two
// values of p & 7 (2-way, on at most one group in four at W=56). The B
// reads are st_16x32 column reads.
//
// Output: per M fragment through the wave's private bounce to
// row-contiguous 16 B stores. The pixels of a tile are contiguous in y,
// so the store predicate is one compare against the tile's valid count.

#include "mfma_tile.hip.h"
#include "kernels.h"

// device code of this file is generated without packed fp32 instructions
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

constexpr int VTHREADS = 256;
constexpr int VWAVES = VTHREADS / 64;
constexpr int VBN = 64;     // output channels per workgroup
constexpr int VBK = 64;     // input channels per slice
constexpr int VMT = 256;    // output pixel slots per tile
constexpr int VHALO = 416;  // halo pixels per tile
constexpr int kHaloElems = VHALO * VBK;
constexpr int kTapElems = VBN * VBK;  // one tap's [64 co][64 ci] tile
constexpr int kWElems = 9 * kTapElems;
constexpr int kBounceElems = VWAVES * 16 * VBN;
constexpr int kLds = (kHaloElems + kWElems + kBounceElems) * 2;
constexpr int kCUs = 256;
static_assert(VMT == VWAVES * 64, "64 pixel slots per wave");
static_assert(kLds <= 160 * 1024, "one workgroup fits a CU's LDS");

struct Geom {
  int n, h, w, cin, cout;
  int rows, imgs, nbands, tiles;
};

// Orders the wave's own LDS traffic for the compiler (conv1x1_stats.hip).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// XOR applied to the 16 B chunk index of halo pixel p. conv3x3_k reads 16 B
// per lane and 16 pixels per read: all three bits. conv3x3_wgrad_k reads
// 8 B per lane and 4 pixels x 32 B per 16-lane group: the 32 B pair index.
struct SwzPix8 {
  static __device__ __forceinline__ int of(int p) { return p & 7; }
};
struct SwzPix4Pair {
  static __device__ __forceinline__ int of(int p) { return (p & 3) << 1; }
};

// The two pad columns of every halo row: zero for the whole launch.
__device__ __forceinline__ void zero_halo_pads(short* lH, int hrows, int W2,
                                               int tid) {
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int q = tid; q < hrows * 16; q += VTHREADS) {
    const int pix = (q >> 4) * W2 + ((q & 8) ? W2 - 1 : 0);
    *(bf16x8*)(lH + pix * VBK + (q & 7) * 8) = zero8;
  }
}

// Halo slice ci0 .. ci0+63 of the tile at (img0, h0): the waves take halo
// rows in turn. A row inside the image is loaded (its W pixels; the pads
// stay zero), a row outside is zeroed if `first` and left alone otherwise.
template <class Swz>
__device__ __forceinline__ void stage_halo(short* lH,
                                           const short* __restrict__ x,
                                           const Geom& g, int img0, int h0,
                                           int ci0, bool first, int wave,
                                           int lane) {
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  const int W2 = g.w + 2;
  const int hrows_seg = g.rows + 2;
  const int hrows = g.imgs * hrows_seg;
  const int row_chunks = g.w * 8;  // 16 B chunks inside a halo row
  int seg = 0, hr = wave;          // hrow = seg * hrows_seg + hr
  for (int hrow = wave; hrow < hrows; hrow += VWAVES, hr += VWAVES) {
    while (hr >= hrows_seg) {
      hr -= hrows_seg;
      ++seg;
    }
    const int img = img0 + seg, ih = h0 + hr - 1;
    if (img >= g.n) break;  // the tile has fewer images
    const int pix0 = hrow * W2 + 1;
    if (ih >= 0 && ih < g.h) {
      const short* src =
          x + (((long long)img * g.h + ih) * g.w) * g.cin + ci0;
      for (int j0 = 0; j0 < row_chunks; j0 += 64) {
        const bool on = j0 + lane < row_chunks;
        const int j = on ? j0 + lane : 0;  // a valid address in any lane
        const int kc = (j & 7) ^ Swz::of(pix0 + (j >> 3));
        const short* gp = src + (long long)(j >> 3) * g.cin + kc * 8;
        if (on) global_load_lds16(gp, lH + (pix0 * 8 + j0) * 8);
      }
    } else if (first) {
      for (int j = lane; j < row_chunks; j += 64)
        *(bf16x8*)(lH + (pix0 * 8 + j) * 8) = zero8;
    }
  }
}

__global__ __launch_bounds__(VTHREADS) void conv3x3_k(
    const short* __restrict__ x, const short* __restrict__ wt,
    short* __restrict__ y, const Geom g) {
  extern __shared__ __attribute__((aligned(16))) short lds[];
  short* lH = lds;
  short* lW = lds + kHaloElems;
  short* lC = lW + kWElems;

  const int nnb = g.cout / VBN;
  const int nb = blockIdx.x % nnb;    // N-block
  const int widx = blockIdx.x / nnb;  // worker of the N-block
  const int nworkers = gridDim.x / nnb;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const FragLane fl(lane);
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

  const int W2 = g.w + 2;
  const int hrows_seg = g.rows + 2;
  const int seg_px = g.rows * g.w;     // output pixels of a segment
  const int seg_hp = hrows_seg * W2;   // halo pixels of a segment
  const int tile_px = g.imgs * seg_px;
  const int hrows = g.imgs * hrows_seg;
  const int row_chunks = g.w * 8;      // 16 B chunks inside a halo row

  zero_halo_pads(lH, hrows, W2, tid);

  // halo index of the lane's output pixel in each of the 4 M fragments
  int hb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int p = wave * 64 + i * 16 + fl.frag_row;
    if (p >= tile_px) p = 0;  // no such pixel: any slot, never stored
    const int seg = p / seg_px;
    const int r = (p - seg * seg_px) / g.w;
    const int c = p - seg * seg_px - r * g.w;
    hb[i] = seg * seg_hp + r * W2 + c;
  }
  // byte offsets of the lane's B fragments inside a tap tile
  int boff[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      boff[j][ks] = tile_swz128(
          ((j * 16 + fl.frag_row) * VBK + ks * 32 + fl.frag_k) * 2);

  // weight slice: 9 tap tiles, pre-permuted source, whole waves
  auto stage_w = [&](int ci0) {
    for (int q = tid; q < 9 * VBN * 8; q += VTHREADS) {
      const int t = q >> 9, row = (q >> 3) & 63;
      const int kc = (q & 7) ^ (row & 7);
      global_load_lds16(
          wt + ((long long)(nb * VBN + row) * 9 + t) * g.cin + ci0 + kc * 8,
          lW + (q - lane) * 8);  // wave-uniform base
    }
  };

  const int nslices = g.cin / VBK;
  if (nslices == 1) stage_w(0);  // the whole panel: resident

  short* myC = lC + wave * (16 * VBN);
  for (int tile = widx; tile < g.tiles; tile += nworkers) {
    const int ti = tile / g.nbands;
    const int img0 = ti * g.imgs;
    const int h0 = (tile - ti * g.nbands) * g.rows;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

    for (int s = 0; s < nslices; ++s) {
      __syncthreads();  // the previous slice's fragment reads are done
      stage_halo<SwzPix8>(lH, x, g, img0, h0, s * VBK, s == 0, wave, lane);
      if (nslices > 1) stage_w(s * VBK);
      __builtin_amdgcn_s_waitcnt(0);
      __syncthreads();

#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int toff = (t / 3) * W2 + t % 3;
        bf16x8 a[4][2], b[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int pix = hb[i] + toff;
          const int off = pix * 128 + (((fl.frag_k >> 3) ^ (pix & 7)) << 4);
          a[i][0] = *(const bf16x8*)((const char*)lH + off);
          // K-step 1 is chunk + 4: bit 6 of the byte offset
          a[i][1] = *(const bf16x8*)((const char*)lH + (off ^ 64));
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
            b[j][ks] = *(const bf16x8*)((const char*)(lW + t * kTapElems) +
                                        boff[j][ks]);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              acc[i][j] = mfma_bf16(a[i][ks], b[j][ks], acc[i][j]);
        __builtin_amdgcn_s_setprio(0);
      }
    }

    // the tile's pixels are contiguous in y: slot p is pixel base_px + p
    const int vimgs = g.n - img0 < g.imgs ? g.n - img0 : g.imgs;
    const int vrows = g.h - h0 < g.rows ? g.h - h0 : g.rows;
    const int nvalid = (vimgs - 1) * seg_px + vrows * g.w;
    const long long base_px = ((long long)img0 * g.h + h0) * g.w;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      wave_lds_sync();  // the previous read-back is done
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
          myC[(fl.c_sub_row + rr) * VBN + j * 16 + fl.c_col] =
              f2bf(acc[i][j][rr]);
      wave_lds_sync();
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int r = u * 8 + lane / 8;
        const int c = (lane % 8) * 8;
        const int p = wave * 64 + i * 16 + r;
        if (p < nvalid) {
          const bf16x8 v = *(const bf16x8*)&myC[r * VBN + c];
          *(bf16x8*)&y[(base_px + p) * g.cout + nb * VBN + c] = v;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------
// Weight gradient (conv3x3_wgrad_k + conv3x3_wgrad_reduce_k)
//
//   dw[co,kh,kw,ci] = sum_{n,h,w} dy[n,h,w,co] * x[n,h+kh-1,w+kw-1,ci]
//
// Per tap a GEMM with M = co, N = ci and the contraction over pixels, on
// the tiles of the forward: the staged halo serves all nine taps.
//
// Work split
//   - one workgroup per (64-co block, 64-ci block) pair and worker; it
//     owns all nine taps of the pair: 9 x 64 x 64 fp32 accumulators that
//     stay in registers over all of the worker's tiles w, w + workers, ...;
//   - 4 waves; wave v owns all 64 co, the 16-ci fragment v and the 9 taps:
//     4 x 9 = 36 accumulator fragments. A 32-pixel K-step reads 4 dy
//     fragments and 9 x fragments (26 b64 transpose reads) for 36 MFMAs;
//     16 co x 64 ci per wave would read 74, 32 x 32 would read 40;
//   - each worker stores its accumulators once, fp32, into its own slab
//     [worker][Cout,3,3,Cin]; conv3x3_wgrad_reduce_k adds the slabs in a
//     fixed order and stores bf16. No atomics, no memset: every slab
//     entry is written, and the result does not depend on timing.
//
// Operands are pixel-major in LDS (as in memory), MFMA wants them
// contraction-major: ds_read_b64_tr_b16 transposes on the read. A 16-lane
// group reads 4 pixels x 16 channels; lane l names pixel l/4, channels
// 4*(l%4) .. +4 and receives channel l%16 of the 4 pixels. Two reads
// (pixels 8g .. 8g+3 and 8g+4 .. 8g+7 of the K-step for group g) make one
// operand fragment. Every lane supplies its own address, so the pixel of
// a lane may lie anywhere: for x it is slot -> halo index (table lT, built
// once per launch) + kh*(W+2) + kw, the forward's one add per tap.
//
// LDS map (dynamic, 85 KiB; one workgroup per CU):
//   [0, 53248)       halo, 416 pixels x 128 B, staged as in the forward
//                    but with the chunk XOR of SwzPix4Pair
//   [53248, 86016)   dy, 256 pixel slots x 128 B (64 co), a linear copy:
//                    the tile's pixels are contiguous in dy; same XOR
//   [86016, 87040)   lT: halo index of each pixel slot (int)
// Single-buffered: barrier, stage, barrier, up to 8 K-steps of 36 MFMAs.
//
// Slots that are no pixel (short band, fewer images, slots past rows*W,
// tail of the last K-step) contribute exactly zero whatever LDS held:
// their dy slots are zeroed with plain stores up to the end of the last
// K-step that holds a pixel (later K-steps are skipped) and are never a
// load target, and their x reads go to halo pixel 0, a pad slot that is
// zero for the whole launch, so no stale Inf or NaN meets the zero.
//
// Bank conflicts: a 16-lane group reads 4 pixels x 32 B. Rows are 128 B,
// so unswizzled the four would share 32 B of the 128-byte period. XOR of
// the 32 B pair index with p & 3 puts 4 consecutive pixels on the four
// pairs: conflict-free for dy (groups start at multiples of 4) and for x
// wherever the 4 halo pixels are consecutive; a group that wraps to the
// next halo row (+2) can repeat one value (2-way). That is per 16-lane
// group only; the counters say the whole picture is worse: bank-conflict
// cycles are 45-54 % of the LDS-active cycles at the four ResNet-50 sites
// (profiles/README.md), so the groups of a wave, or the waves, collide.
//
// Registers: 144 accumulator + 16 dy + 36 x operand registers, 2 halo
// indices, 4 dy offsets; launch_bounds(256) allows 512. Measured use,
// scratch (0) and occupancy: profiles/README.md.
// ---------------------------------------------------------------------

constexpr int kDyElems = VMT * VBN;
constexpr int kWgLds = (kHaloElems + kDyElems) * 2 + VMT * 4;
static_assert(kWgLds <= 160 * 1024, "one workgroup fits a CU's LDS");

typedef __attribute__((address_space(3))) short4v* lds_b64_ptr;

// One hardware transpose read at LDS byte address a (see above).
__device__ __forceinline__ short4v lds_tr_b64(unsigned a) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_b64_ptr)a);
}
// The operand fragment made of the reads at a0 and a1.
__device__ __forceinline__ bf16x8 tr_frag2(unsigned a0, unsigned a1) {
  const short4v v0 = lds_tr_b64(a0), v1 = lds_tr_b64(a1);
  return bf16x8{v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
}

__global__ __launch_bounds__(VTHREADS) void conv3x3_wgrad_k(
    const short* __restrict__ x, const short* __restrict__ dy,
    float* __restrict__ slabs, const Geom g) {
  extern __shared__ __attribute__((aligned(16))) short lds[];
  short* lH = lds;
  short* lD = lds + kHaloElems;
  int* lT = (int*)(lD + kDyElems);

  const int ncib = g.cin / VBK;
  const int npairs = (g.cout / VBN) * ncib;
  const int pair = blockIdx.x % npairs;
  const int widx = blockIdx.x / npairs;  // worker of the pair
  const int nworkers = gridDim.x / npairs;
  const int cob = pair / ncib, cib = pair - cob * ncib;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const FragLane fl(lane);
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

  const int W2 = g.w + 2;
  const int seg_px = g.rows * g.w;
  const int seg_hp = (g.rows + 2) * W2;
  const int tile_px = g.imgs * seg_px;

  zero_halo_pads(lH, g.imgs * (g.rows + 2), W2, tid);
  // halo index of every pixel slot; slots past the tile are never valid
  for (int p = tid; p < VMT; p += VTHREADS) {
    int hb = 0;
    if (p < tile_px) {
      const int seg = p / seg_px;
      const int r = (p - seg * seg_px) / g.w;
      hb = seg * seg_hp + r * W2 + (p - seg * seg_px - r * g.w);
    }
    lT[p] = hb;
  }

  // the lane's part in a transpose read: pixel slot sl (+4 for the second
  // read) of the K-step, 8 bytes at lgoff of the 32 B of its fragment
  const int lg = lane & 15;
  const int sl = (lane >> 4) * 8 + (lg >> 2);
  const int lgoff = (lg & 3) * 8;
  const unsigned hbase = (unsigned)(unsigned long long)(
      (__attribute__((address_space(3))) short*)lH) + lgoff;
  // dy fragment i: slot s & 3 == lg >> 2, so the pair index is i ^ (lg >> 2)
  unsigned dbase[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    dbase[i] = (unsigned)(unsigned long long)(
                   (__attribute__((address_space(3))) short*)lD) +
               sl * 128 + ((i ^ (lg >> 2)) << 5) + lgoff;

  f32x4 acc[4][9];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[i][t] = {0.f, 0.f, 0.f, 0.f};

  for (int tile = widx; tile < g.tiles; tile += nworkers) {
    const int ti = tile / g.nbands;
    const int img0 = ti * g.imgs;
    const int h0 = (tile - ti * g.nbands) * g.rows;
    // slot p < nvalid is pixel base_px + p of x and dy
    const int vimgs = g.n - img0 < g.imgs ? g.n - img0 : g.imgs;
    const int vrows = g.h - h0 < g.rows ? g.h - h0 : g.rows;
    const int nvalid = (vimgs - 1) * seg_px + vrows * g.w;
    const long long base_px = ((long long)img0 * g.h + h0) * g.w;
    const int nk = (nvalid + 31) >> 5;  // K-steps that hold a pixel

    __syncthreads();  // the previous tile's fragment reads are done
    stage_halo<SwzPix4Pair>(lH, x, g, img0, h0, cib * VBK, true, wave, lane);
    const short* src = dy + base_px * g.cout + cob * VBN;
    const int nchunks = nvalid * 8;  // 16 B chunks that hold dy
    for (int q0 = wave * 64; q0 < nchunks; q0 += VTHREADS) {
      const bool on = q0 + lane < nchunks;
      const int q = on ? q0 + lane : 0;  // a valid address in any lane
      const int kc = (q & 7) ^ SwzPix4Pair::of(q >> 3);
      const short* gp = src + (long long)(q >> 3) * g.cout + kc * 8;
      if (on) global_load_lds16(gp, lD + q0 * 8);
    }
    for (int q = nchunks + tid; q < nk * 32 * 8; q += VTHREADS)
      *(bf16x8*)(lD + q * 8) = zero8;
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();

    for (int ks = 0; ks < nk; ++ks) {
      const int s0 = ks * 32 + sl;
      const int hb0 = lT[s0], hb1 = lT[s0 + 4];
      const bool ok0 = s0 < nvalid, ok1 = s0 + 4 < nvalid;
      bf16x8 a[4], b[9];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned d = dbase[i] + ks * (32 * 128);
        a[i] = tr_frag2(d, d + 4 * 128);
      }
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int toff = (t / 3) * W2 + t % 3;
        const int p0 = ok0 ? hb0 + toff : 0, p1 = ok1 ? hb1 + toff : 0;
        b[t] = tr_frag2(hbase + p0 * 128 + ((wave ^ (p0 & 3)) << 5),
                        hbase + p1 * 128 + ((wave ^ (p1 & 3)) << 5));
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          acc[i][t] = mfma_bf16(a[i], b[t], acc[i][t]);
      __builtin_amdgcn_s_setprio(0);
    }
  }

  // C fragment (i, t): co = 16 i + c_sub_row + r, ci = 16 wave + c_col
  float* slab = slabs + (long long)widx * g.cout * 9 * g.cin;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const long long co = cob * VBN + i * 16 + fl.c_sub_row + rr;
      float* row = slab + co * 9 * g.cin + cib * VBK + wave * 16 + fl.c_col;
#pragma unroll
      for (int t = 0; t < 9; ++t) row[t * g.cin] = acc[i][t][rr];
    }
}

// dw = bf16(sum of the slabs). A block takes RQ float4 columns; thread
// (q, part) adds the slabs part*per .. part*per+per-1 in order, then part 0
// adds the RP partial sums in order: a fixed tree, 1/RP of the chain.
constexpr int RQ = 32, RP = 8;
static_assert(VBN * VBK * 9 / 4 % RQ == 0, "whole blocks of float4 columns");

__global__ __launch_bounds__(RQ* RP) void conv3x3_wgrad_reduce_k(
    const float4v* __restrict__ slabs, short4v* __restrict__ dw,
    long long quads, int workers) {
  __shared__ float4v part[RP][RQ];
  const int qi = threadIdx.x % RQ, pt = threadIdx.x / RQ;
  const long long q = (long long)blockIdx.x * RQ + qi;
  const int per = (workers + RP - 1) / RP;
  const int w1 = (pt + 1) * per < workers ? (pt + 1) * per : workers;
  float4v s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int w = pt * per; w < w1; ++w) s += slabs[w * quads + q];
  part[pt][qi] = s;
  __syncthreads();
  if (pt == 0) {
#pragma unroll
    for (int k = 1; k < RP; ++k) s += part[k][qi];
    dw[q] = short4v{f2bf(s[0]), f2bf(s[1]), f2bf(s[2]), f2bf(s[3])};
  }
}

int ceil_div(int a, int b) { return (a + b - 1) / b; }

// rows, imgs, nbands of the tiling described in the header
void tile_shape(int h, int w, int* rows, int* imgs, int* nbands) {
  const long long px = (long long)h * w, hp = (long long)(h + 2) * (w + 2);
  if (px <= VMT && hp <= VHALO) {
    const int by_px = VMT / (int)px, by_hp = VHALO / (int)hp;
    *rows = h;
    *imgs = by_px < by_hp ? by_px : by_hp;
    *nbands = 1;
    return;
  }
  int maxr = VMT / w;
  if (maxr > VHALO / (w + 2) - 2) maxr = VHALO / (w + 2) - 2;
  if (maxr > h) maxr = h;
  *nbands = ceil_div(h, maxr);
  *rows = ceil_div(h, *nbands);
  *imgs = 1;
}

// rows, imgs, nbands and tiles of g, and the workers per block of the
// `blocks` output blocks that share the CUs
int plan(Geom* g, int blocks, int max_workers) {
  tile_shape(g->h, g->w, &g->rows, &g->imgs, &g->nbands);
  g->tiles = g->nbands > 1 ? g->n * g->nbands : ceil_div(g->n, g->imgs);
  int workers = kCUs / blocks;
  if (workers < 1) workers = 1;
  if (workers > g->tiles) workers = g->tiles;
  if (max_workers > 0 && workers > max_workers) workers = max_workers;
  return workers;
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

bool conv3x3_supported(long long n, long long h, long long w, int cin,
                       int cout) {
  return cin >= VBK && cin % VBK == 0 && cout >= VBN && cout % VBN == 0 &&
         n >= 1 && h >= 1 && w >= 1 && w <= 56 &&
         n * h < (1LL << 31) && n * h * w < (1LL << 31);
}

// Launch plan.
//   rows, imgs: the tile (header); one of them is 1 unless H*W <= 256.
//   tiles:      per N-block: N * bands per image, or ceil(N / imgs).
//   workers:    per N-block: one workgroup per CU over all N-blocks (LDS
//               admits one workgroup per CU), at most one per tile;
//               max_workers > 0 lowers it further.
void conv3x3_plan(int n, int h, int w, int cin, int cout, int max_workers,
                  int* rows, int* imgs, int* tiles, int* workers) {
  Geom g{n, h, w, cin, cout, 0, 0, 0, 0};
  *workers = plan(&g, cout / VBN, max_workers);
  *rows = g.rows;
  *imgs = g.imgs;
  *tiles = g.tiles;
}

void launch_conv3x3(const short* x, const short* wt, short* y, int n, int h,
                    int w, int cin, int cout, int max_workers,
                    hipStream_t stream) {
  static const hipError_t lds_set = hipFuncSetAttribute(
      (const void*)&conv3x3_k, hipFuncAttributeMaxDynamicSharedMemorySize,
      kLds);
  (void)lds_set;
  Geom g{n, h, w, cin, cout, 0, 0, 0, 0};
  const int workers = plan(&g, cout / VBN, max_workers);
  hipLaunchKernelGGL(conv3x3_k, dim3((cout / VBN) * workers),
                     dim3(VTHREADS), kLds, stream, x, wt, y, g);
}

// Launch plan of the weight gradient: the forward's tile, tiles per
// (co-block, ci-block) pair, and workers per pair: one workgroup per CU
// over all pairs, at most one per tile; max_workers > 0 lowers it further.
void conv3x3_wgrad_plan(int n, int h, int w, int cin, int cout,
                        int max_workers, int* rows, int* imgs, int* tiles,
                        int* workers) {
  Geom g{n, h, w, cin, cout, 0, 0, 0, 0};
  *workers = plan(&g, (cout / VBN) * (cin / VBK), max_workers);
  *rows = g.rows;
  *imgs = g.imgs;
  *tiles = g.tiles;
}

void launch_conv3x3_wgrad(const short* x, const short* dy, float* slabs,
                          short* dw, int n, int h, int w, int cin, int cout,
                          int max_workers, hipStream_t stream) {
  static const hipError_t lds_set = hipFuncSetAttribute(
      (const void*)&conv3x3_wgrad_k,
      hipFuncAttributeMaxDynamicSharedMemorySize, kWgLds);
  (void)lds_set;
  Geom g{n, h, w, cin, cout, 0, 0, 0, 0};
  const int pairs = (cout / VBN) * (cin / VBK);
  const int workers = plan(&g, pairs, max_workers);
  hipLaunchKernelGGL(conv3x3_wgrad_k, dim3(pairs * workers), dim3(VTHREADS),
                     kWgLds, stream, x, dy, slabs, g);
  const long long quads = (long long)cout * 9 * cin / 4;
  hipLaunchKernelGGL(conv3x3_wgrad_reduce_k, dim3((unsigned)(quads / RQ)),
                     dim3(RQ * RP), 0, stream, (const float4v*)slabs,
                     (short4v*)dw, quads, workers);
}
