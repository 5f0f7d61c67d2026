// 3x3 stride-2 pad-1 convolution, bf16 NHWC, forward and data gradient,
// as implicit GEMMs on mfma_f32_16x16x32_bf16 (the
// conv2 of the bottlenecks that open ResNet-50's stages 2, 3 and 4).
// Ho = (H-1)/2 + 1, Wo = (W-1)/2 + 1; fp32 accumulation, zero padding, no
// bias, f2bf store. Both kernels tile the Ho x Wo grid in whole rows (a
// band of one image) or whole small images, take one 64-wide block of
// output channels per workgroup, run 4 waves and are persistent: worker w
// of a block takes tiles w, w + workers, ... (the scheme of conv3x3.hip).
// No atomics, no memset, no scratch buffer: every output element is
// written once by one lane, the same bits on every run.
//
// ---------------------------------------------------------------------
// Forward (conv3x3_s2_k)
//
//   y[n,ho,wo,co] = sum_{kh,kw,ci} x[n,2ho+kh-1,2wo+kw-1,ci] * wt[co,kh,kw,ci]
//
// x [N,H,W,Cin], wt [Cout,3,3,Cin], y [N,Ho,Wo,Cout]. M = N*Ho*Wo,
// N = Cout, K = 9*Cin.
//
// Geometry (conv3x3_s2_plan)
//   - a tile has at most FMT = 256 output pixels and FHALO = 1152 halo
//     pixels: `rows` output rows of one image, balanced as in conv3x3.hip,
//     or `imgs` whole images. 7 rows at Wo = 28 (196 px, halo 15 x 57 =
//     855), one 14x14 image (196, 29 x 29 = 841), five 7x7 images (245,
//     5 x 15 x 15 = 1125);
//   - wave v owns pixel slots 64v .. 64v+63: 4 M x 4 N accumulator
//     fragments, 8 operand fragment reads per 16 MFMAs, as conv3x3_k.
//
// K loop: Cin in slices of FBK = 32 channels, so a halo pixel is 64 B and
// a tap is one MFMA K-step: 9 x 16 = 144 MFMAs per wave and slice. Per
// slice, staged with global_load_lds16 and single-buffered:
//   - the halo: imgs x (2*rows+1) rows (input rows 2*h0-1 .. 2*h0+2*rows-1)
//     of 2*Wo+1 pixels (input columns -1 .. 2*Wo-1). A halo row is stored
//     as two planes: first the Wo+1 odd columns -1, 1, .., 2*Wo-1, then
//     the Wo even columns 0, 2, .., 2*Wo-2. Output pixel (r, c) has base
//     2r*(2Wo+1) + c, and tap (kh, kw) is pixel base + kh*(2Wo+1) + d(kw)
//     with d = 0, Wo+1, 1 for kw = 0, 1, 2 (odd plane at c, even plane at
//     c, odd plane at c+1): one add per tap, no masks, and a run of output
//     pixels reads a run of LDS pixels. Column -1 of every row, and column
//     2*Wo-1 where W is odd, are zeroed once per launch with plain stores;
//     rows outside the image are zeroed once per tile. None of these is
//     ever the target of a load: the lane of a load that would write one
//     is switched off, its address clamped;
//   - the weight slice as 9 tiles [64 co][32 ci], one per tap. Cin is at
//     least two slices, so no panel is resident.
// Output pixels of a tile that do not exist read whatever their halo slots
// hold; a row of A only reaches the same row of C, which is not stored.
//
// LDS map (dynamic, 116 KiB of the 160 KiB of a CU, one workgroup per CU):
//   [0, 73728)         halo, 1152 pixels x 64 B
//   [73728, 110592)    weights, 9 x 64 x 64 B = 9 x 4 KiB
//   [110592, 118784)   output bounce, 2 KiB per wave
// With 64-channel slices the halo alone would be 144 KiB.
//
// Registers: 64 accumulator + 16 A + 16 B operand registers per tap, 4
// halo bases, 4 B offsets.
//
// Bank conflicts: rows (halo pixels, weight rows) are 64 B, so a 128-byte
// period holds two rows of four 16 B chunks. Chunk k of row p is stored at
// chunk k ^ ((p >> 1) & 3) of its row. The 16 lanes of a fragment read
// share k and hold 16 consecutive rows (output pixels c, c+1, .. read
// consecutive pixels of one plane; B reads consecutive co). Eight
// consecutive rows have four different p >> 1 & 3, each with both values
// of p & 1: eight different 16 B positions of the 128-byte period,
// conflict-free by the same count as SwzPix8 in conv3x3.hip. Had the halo
// kept its columns in input order, the lanes would hold every second
// pixel, p & 1 would be constant and every position would repeat (2-way).
// A run that wraps to the next output row jumps by 3*Wo + 2 pixels and can
// repeat values inside one group of eight (2-way on that group).
//
// Output: per M fragment through the wave's bounce to row-contiguous 16 B
// stores; a tile's pixels are contiguous in y.
//
// ---------------------------------------------------------------------
// Data gradient (conv3x3_s2_dgrad_k)
//
//   dx[n,h,w,ci] = sum dy[n,ho,wo,co] * wd[ci,kh,kw,co]
//                  over (kh,kw,ho,wo) with h = 2ho+kh-1, w = 2wo+kw-1
//
// dy [N,Ho,Wo,Cout], wd [Cin,3,3,Cout] (unflipped: wd[ci,kh,kw,co] =
// w[co,ci,kh,kw]), dx [N,H,W,Cin]. Organised by cells of the dy grid:
// cell (i, j) owns dx pixels (2i+dr, 2j+dc), the four parity classes
// (dr, dc). Row 2i+dr = 2ho+kh-1 has the solutions kh = 1, ho = i for
// dr = 0 and kh = 0, ho = i+1 or kh = 2, ho = i for dr = 1; the same for
// columns. So tap (kh, kw) belongs to class (kh != 1, kw != 1) and reads
// dy at (i + (kh == 0), j + (kw == 0)): 1 + 2 + 2 + 4 = 9 tap-GEMMs per
// cell with K = Cout, the forward's FLOPs, nothing multiplied by an
// inserted zero.
//
// Geometry (conv3x3_s2_dgrad_plan)
//   - a tile has at most DMT = 128 cells and DHALO = 256 dy halo pixels:
//     `rows` rows of cells of one image or `imgs` whole dy images. 4 rows
//     at Wo = 28 (112 cells, halo 5 x 29 = 145), 7 rows at Wo = 14 (98,
//     8 x 15 = 120), two 7x7 images (98, 2 x 8 x 8 = 128);
//   - wave v owns cell slots 32v .. 32v+31: 2 M fragments x 4 classes x 4
//     N fragments = 32 accumulator fragments, 128 registers. 256 cells
//     would need 256; classes outside the K loop would need 64 but stage
//     dy four times. A 32-channel K-step reads 2 x 4 dy fragments (the
//     four dy positions of a cell) and 9 x 4 weight fragments for 72
//     MFMAs: 44 reads per 72, against 8 per 16 in the forward.
//
// K loop: Cout in slices of 64 channels, 2 K-steps. Per slice:
//   - the dy halo: imgs x (rows+1) rows (dy rows i0 .. i0+rows) of Wo+1
//     pixels (columns 0 .. Wo), 128 B each, chunk XOR p & 7 as conv3x3_k.
//     Column Wo is zeroed once per launch, rows >= Ho once per tile, so
//     the taps of a cell's last row and column, and the classes that an
//     odd H or W lacks, read zeros or unused data inside the halo;
//   - the weight slice as 9 tiles [64 ci][64 co], st_16x32 swizzled;
//     with Cout = 64 it is the whole panel and staged once per workgroup.
//
// LDS map (dynamic, 112 KiB, one workgroup per CU):
//   [0, 32768)         dy halo, 256 pixels x 128 B
//   [32768, 106496)    weights, 9 x 8 KiB
//   [106496, 114688)   output bounce, 2 KiB per wave
//
// Registers: 128 accumulator + 32 A + 16 B operand registers per tap, 2
// halo bases, 8 B offsets, 4 x 3 store coordinates; launch_bounds(256)
// allows 512. Measured use, scratch (0) and occupancy of both kernels:
// profiles/README.md.
//
// Bank conflicts: as conv3x3_k. The 16 lanes of an A read hold 16
// consecutive cells, consecutive halo pixels except where the run wraps
// (+1); eight consecutive pixels have eight values of p & 7.
//
// Output: per (M fragment, class) through the wave's bounce; a bounce row
// is the 128 B of one dx pixel and 64 channels, stored by eight lanes. A
// pixel is stored if its cell exists in the tile and its row 2i+dr < H
// and column 2j+dc < W.

#include "mfma_tile.hip.h"
#include "kernels.h"

// device code of this file is generated without packed fp32 instructions
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

constexpr int STHREADS = 256;
constexpr int SWAVES = STHREADS / 64;
constexpr int SBN = 64;  // output channels per workgroup
constexpr int kCUs = 256;
constexpr int kBounceElems = SWAVES * 16 * SBN;

// forward
constexpr int FBK = 32;      // input channels per slice
constexpr int FMT = 256;     // output pixel slots per tile
constexpr int FHALO = 1152;  // halo pixels per tile
constexpr int kFHaloElems = FHALO * FBK;
constexpr int kFTapElems = SBN * FBK;  // one tap's [64 co][32 ci] tile
constexpr int kFWElems = 9 * kFTapElems;
constexpr int kFLds = (kFHaloElems + kFWElems + kBounceElems) * 2;
static_assert(FMT == SWAVES * 64, "64 pixel slots per wave");
static_assert(kFLds <= 160 * 1024, "one workgroup fits a CU's LDS");

// data gradient
constexpr int DBK = 64;     // dy channels per slice
constexpr int DMT = 128;    // cell slots per tile
constexpr int DHALO = 256;  // dy halo pixels per tile
constexpr int kDHaloElems = DHALO * DBK;
constexpr int kDTapElems = SBN * DBK;  // one tap's [64 ci][64 co] tile
constexpr int kDWElems = 9 * kDTapElems;
constexpr int kDLds = (kDHaloElems + kDWElems + kBounceElems) * 2;
static_assert(DMT == SWAVES * 32, "32 cell slots per wave");
static_assert(kDLds <= 160 * 1024, "one workgroup fits a CU's LDS");

// rows, imgs, nbands and tiles describe the tiling of the ho x wo grid
struct GeomS2 {
  int n, h, w, ho, wo, cin, cout;
  int rows, imgs, nbands, tiles;
};

// Orders the wave's own LDS traffic for the compiler (conv1x1_stats.hip).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// XOR applied to the 16 B chunk index (0 .. 3) of the 64-byte row p.
__device__ __forceinline__ int swz64(int p) { return (p >> 1) & 3; }

__global__ __launch_bounds__(STHREADS) void conv3x3_s2_k(
    const short* __restrict__ x, const short* __restrict__ wt,
    short* __restrict__ y, const GeomS2 g) {
  extern __shared__ __attribute__((aligned(16))) short lds[];
  short* lH = lds;
  short* lW = lds + kFHaloElems;
  short* lC = lW + kFWElems;

  const int nnb = g.cout / SBN;
  const int nb = blockIdx.x % nnb;    // N-block
  const int widx = blockIdx.x / nnb;  // worker of the N-block
  const int nworkers = gridDim.x / nnb;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const FragLane fl(lane);
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

  const int HW = 2 * g.wo + 1;          // pixels of a halo row
  const int hrows_seg = 2 * g.rows + 1;
  const int seg_px = g.rows * g.wo;     // output pixels of a segment
  const int seg_hp = hrows_seg * HW;    // halo pixels of a segment
  const int tile_px = g.imgs * seg_px;
  const int hrows = g.imgs * hrows_seg;
  const int row_chunks = HW * 4;        // 16 B chunks of a halo row

  // columns -1 and, for odd W, 2*Wo-1 = W of every halo row: slots 0 and
  // Wo of the odd plane, zero for the whole launch
  for (int q = tid; q < hrows * 8; q += STHREADS) {
    if ((q & 4) && !(g.w & 1)) continue;
    const int pix = (q >> 3) * HW + ((q & 4) ? g.wo : 0);
    *(bf16x8*)(lH + pix * FBK + (q & 3) * 8) = zero8;
  }

  // halo base of the lane's output pixel in each of the 4 M fragments
  int hb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int p = wave * 64 + i * 16 + fl.frag_row;
    if (p >= tile_px) p = 0;  // no such pixel: any slot, never stored
    const int seg = p / seg_px;
    const int r = (p - seg * seg_px) / g.wo;
    const int c = p - seg * seg_px - r * g.wo;
    hb[i] = seg * seg_hp + 2 * r * HW + c;
  }
  // byte offsets of the lane's B fragments inside a tap tile
  int boff[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = j * 16 + fl.frag_row;
    boff[j] = row * (FBK * 2) + (((fl.frag_k >> 3) ^ swz64(row)) << 4);
  }
  const int tapd[3] = {0, g.wo + 1, 1};  // kw -> plane and slot

  // Halo slice ci0 .. ci0+31 of the tile at (img0, h0): the waves take
  // halo rows in turn. A row inside the image is loaded (the pads stay
  // zero), a row outside is zeroed if `first` and left alone otherwise.
  auto stage_halo = [&](int img0, int h0, int ci0, bool first) {
    int seg = 0, hr = wave;  // hrow = seg * hrows_seg + hr
    for (int hrow = wave; hrow < hrows; hrow += SWAVES, hr += SWAVES) {
      while (hr >= hrows_seg) {
        hr -= hrows_seg;
        ++seg;
      }
      const int img = img0 + seg, ih = 2 * h0 - 1 + hr;
      if (img >= g.n) break;  // the tile has fewer images
      const int pix0 = hrow * HW;
      if (ih >= 0 && ih < g.h) {
        const short* src =
            x + (((long long)img * g.h + ih) * g.w) * g.cin + ci0;
        for (int j0 = 0; j0 < row_chunks; j0 += 64) {
          const int j = j0 + lane, pr = j >> 2;  // pixel of the halo row
          const int col = pr <= g.wo ? 2 * pr - 1 : 2 * (pr - g.wo - 1);
          const bool on = j < row_chunks && col >= 0 && col < g.w;
          const int kc = (j & 3) ^ swz64(pix0 + pr);
          // a valid address in any lane
          const short* gp = src + (long long)(on ? col : 0) * g.cin + kc * 8;
          if (on) global_load_lds16(gp, lH + (pix0 * 4 + j0) * 8);
        }
      } else if (first) {
        for (int j = lane; j < row_chunks; j += 64)
          *(bf16x8*)(lH + (pix0 * 4 + j) * 8) = zero8;
      }
    }
  };
  // weight slice: 9 tap tiles, pre-permuted source, whole waves
  auto stage_w = [&](int ci0) {
    for (int q = tid; q < 9 * SBN * 4; q += STHREADS) {
      const int t = q >> 8, row = (q >> 2) & 63;
      const int kc = (q & 3) ^ swz64(row);
      global_load_lds16(
          wt + ((long long)(nb * SBN + row) * 9 + t) * g.cin + ci0 + kc * 8,
          lW + (q - lane) * 8);  // wave-uniform base
    }
  };

  const int nslices = g.cin / FBK;
  short* myC = lC + wave * (16 * SBN);
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
      stage_halo(img0, h0, s * FBK, s == 0);
      stage_w(s * FBK);
      __builtin_amdgcn_s_waitcnt(0);
      __syncthreads();

#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int toff = (t / 3) * HW + tapd[t % 3];
        bf16x8 a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int pix = hb[i] + toff;
          a[i] = *(const bf16x8*)((const char*)lH + pix * (FBK * 2) +
                                  (((fl.frag_k >> 3) ^ swz64(pix)) << 4));
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
          b[j] = *(const bf16x8*)((const char*)(lW + t * kFTapElems) +
                                  boff[j]);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = mfma_bf16(a[i], b[j], acc[i][j]);
        __builtin_amdgcn_s_setprio(0);
      }
    }

    // the tile's pixels are contiguous in y: slot p is pixel base_px + p
    const int vimgs = g.n - img0 < g.imgs ? g.n - img0 : g.imgs;
    const int vrows = g.ho - h0 < g.rows ? g.ho - h0 : g.rows;
    const int nvalid = (vimgs - 1) * seg_px + vrows * g.wo;
    const long long base_px = ((long long)img0 * g.ho + h0) * g.wo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      wave_lds_sync();  // the previous read-back is done
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
          myC[(fl.c_sub_row + rr) * SBN + j * 16 + fl.c_col] =
              f2bf(acc[i][j][rr]);
      wave_lds_sync();
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int r = u * 8 + lane / 8;
        const int c = (lane % 8) * 8;
        const int p = wave * 64 + i * 16 + r;
        if (p < nvalid) {
          const bf16x8 v = *(const bf16x8*)&myC[r * SBN + c];
          *(bf16x8*)&y[(base_px + p) * g.cout + nb * SBN + c] = v;
        }
      }
    }
  }
}

__global__ __launch_bounds__(STHREADS) void conv3x3_s2_dgrad_k(
    const short* __restrict__ dy, const short* __restrict__ wd,
    short* __restrict__ dx, const GeomS2 g) {
  extern __shared__ __attribute__((aligned(16))) short lds[];
  short* lH = lds;
  short* lW = lds + kDHaloElems;
  short* lC = lW + kDWElems;

  const int nnb = g.cin / SBN;
  const int nb = blockIdx.x % nnb;    // block of dx channels
  const int widx = blockIdx.x / nnb;  // worker of the block
  const int nworkers = gridDim.x / nnb;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const FragLane fl(lane);
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

  const int W1 = g.wo + 1;            // pixels of a halo row
  const int hrows_seg = g.rows + 1;
  const int seg_px = g.rows * g.wo;   // cells of a segment
  const int seg_hp = hrows_seg * W1;  // halo pixels of a segment
  const int tile_px = g.imgs * seg_px;
  const int hrows = g.imgs * hrows_seg;
  const int row_chunks = g.wo * 8;    // 16 B chunks of dy in a halo row

  // column Wo of every halo row: zero for the whole launch
  for (int q = tid; q < hrows * 8; q += STHREADS)
    *(bf16x8*)(lH + ((q >> 3) * W1 + g.wo) * DBK + (q & 7) * 8) = zero8;

  // halo index of the lane's cell in each of the 2 M fragments
  int hb[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    int p = wave * 32 + m * 16 + fl.frag_row;
    if (p >= tile_px) p = 0;  // no such cell: any slot, never stored
    const int seg = p / seg_px;
    const int r = (p - seg * seg_px) / g.wo;
    hb[m] = seg * seg_hp + r * W1 + (p - seg * seg_px - r * g.wo);
  }
  // (segment, row, column) of the cells whose dx pixels the lane stores:
  // bounce row u*8 + lane/8 of M fragment m. No such cell: segment = imgs.
  int sseg[2][2], srow[2][2], scol[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int p = wave * 32 + m * 16 + u * 8 + lane / 8;
      const int seg = p < tile_px ? p / seg_px : g.imgs;
      const int q = p < tile_px ? p - seg * seg_px : 0;
      sseg[m][u] = seg;
      srow[m][u] = q / g.wo;
      scol[m][u] = q - (q / g.wo) * g.wo;
    }
  // byte offsets of the lane's B fragments inside a tap tile
  int boff[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      boff[j][ks] = tile_swz128(
          ((j * 16 + fl.frag_row) * DBK + ks * 32 + fl.frag_k) * 2);

  // dy halo slice co0 .. co0+63 of the tile at (img0, i0): the waves take
  // halo rows in turn; a row at or below Ho is zeroed if `first`.
  auto stage_halo = [&](int img0, int i0, int co0, bool first) {
    int seg = 0, hr = wave;  // hrow = seg * hrows_seg + hr
    for (int hrow = wave; hrow < hrows; hrow += SWAVES, hr += SWAVES) {
      while (hr >= hrows_seg) {
        hr -= hrows_seg;
        ++seg;
      }
      const int img = img0 + seg, ih = i0 + hr;
      if (img >= g.n) break;  // the tile has fewer images
      const int pix0 = hrow * W1;
      if (ih < g.ho) {
        const short* src =
            dy + (((long long)img * g.ho + ih) * g.wo) * g.cout + co0;
        for (int j0 = 0; j0 < row_chunks; j0 += 64) {
          const bool on = j0 + lane < row_chunks;
          const int j = on ? j0 + lane : 0;  // a valid address in any lane
          const int kc = (j & 7) ^ ((pix0 + (j >> 3)) & 7);
          const short* gp = src + (long long)(j >> 3) * g.cout + kc * 8;
          if (on) global_load_lds16(gp, lH + (pix0 * 8 + j0) * 8);
        }
      } else if (first) {
        for (int j = lane; j < row_chunks; j += 64)
          *(bf16x8*)(lH + (pix0 * 8 + j) * 8) = zero8;
      }
    }
  };
  // weight slice: 9 tap tiles [64 ci][64 co], pre-permuted source
  auto stage_w = [&](int co0) {
    for (int q = tid; q < 9 * SBN * 8; q += STHREADS) {
      const int t = q >> 9, row = (q >> 3) & 63;
      const int kc = (q & 7) ^ (row & 7);
      global_load_lds16(
          wd + ((long long)(nb * SBN + row) * 9 + t) * g.cout + co0 + kc * 8,
          lW + (q - lane) * 8);  // wave-uniform base
    }
  };

  const int nslices = g.cout / DBK;
  if (nslices == 1) stage_w(0);  // the whole panel: resident

  short* myC = lC + wave * (16 * SBN);
  for (int tile = widx; tile < g.tiles; tile += nworkers) {
    const int ti = tile / g.nbands;
    const int img0 = ti * g.imgs;
    const int i0 = (tile - ti * g.nbands) * g.rows;

    f32x4 acc[2][4][4];  // [M fragment][class 2*dr+dc][N fragment]
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int cl = 0; cl < 4; ++cl)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[m][cl][j] = {0.f, 0.f, 0.f, 0.f};

    for (int s = 0; s < nslices; ++s) {
      __syncthreads();  // the previous slice's fragment reads are done
      stage_halo(img0, i0, s * DBK, s == 0);
      if (nslices > 1) stage_w(s * DBK);
      __builtin_amdgcn_s_waitcnt(0);
      __syncthreads();

#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        // dy at (i + di, j + dj), position 2*di + dj
        bf16x8 a[2][4];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int pos = 0; pos < 4; ++pos) {
            const int pix = hb[m] + (pos >> 1) * W1 + (pos & 1);
            const int off = pix * 128 + (((fl.frag_k >> 3) ^ (pix & 7)) << 4);
            // K-step 1 is chunk + 4: bit 6 of the byte offset
            a[m][pos] = *(const bf16x8*)((const char*)lH + (off ^ (ks << 6)));
          }
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const int kh = t / 3, kw = t % 3;
          const int cl = (kh != 1) * 2 + (kw != 1);
          const int pos = (kh == 0) * 2 + (kw == 0);
          bf16x8 b[4];
#pragma unroll
          for (int j = 0; j < 4; ++j)
            b[j] = *(const bf16x8*)((const char*)(lW + t * kDTapElems) +
                                    boff[j][ks]);
          __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              acc[m][cl][j] = mfma_bf16(a[m][pos], b[j], acc[m][cl][j]);
          __builtin_amdgcn_s_setprio(0);
        }
      }
    }

    const int vimgs = g.n - img0 < g.imgs ? g.n - img0 : g.imgs;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int cl = 0; cl < 4; ++cl) {
        wave_lds_sync();  // the previous read-back is done
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int rr = 0; rr < 4; ++rr)
            myC[(fl.c_sub_row + rr) * SBN + j * 16 + fl.c_col] =
                f2bf(acc[m][cl][j][rr]);
        wave_lds_sync();
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int r = u * 8 + lane / 8;
          const int c = (lane % 8) * 8;
          const int ci = i0 + srow[m][u];  // the cell's row in the image
          const int oh = 2 * ci + (cl >> 1), ow = 2 * scol[m][u] + (cl & 1);
          if (sseg[m][u] < vimgs && ci < g.ho && oh < g.h && ow < g.w) {
            const bf16x8 v = *(const bf16x8*)&myC[r * SBN + c];
            const long long px =
                ((long long)(img0 + sseg[m][u]) * g.h + oh) * g.w + ow;
            *(bf16x8*)&dx[px * g.cin + nb * SBN + c] = v;
          }
        }
      }
  }
}

int ceil_div(int a, int b) { return (a + b - 1) / b; }

// rows, imgs, nbands and tiles of g (header), and the workers per block of
// the `blocks` channel blocks that share the CUs. Halo pixels of r rows:
// (2r+1)(2Wo+1) forward, (r+1)(Wo+1) for the data gradient.
int plan(GeomS2* g, bool dgrad, int blocks, int max_workers) {
  const int mt = dgrad ? DMT : FMT, cap = dgrad ? DHALO : FHALO;
  const int hw = dgrad ? g->wo + 1 : 2 * g->wo + 1;
  const long long px = (long long)g->ho * g->wo;
  const long long hp = (long long)(dgrad ? g->ho + 1 : 2 * g->ho + 1) * hw;
  if (px <= mt && hp <= cap) {
    const int by_px = mt / (int)px, by_hp = cap / (int)hp;
    g->rows = g->ho;
    g->imgs = by_px < by_hp ? by_px : by_hp;
    g->nbands = 1;
    g->tiles = ceil_div(g->n, g->imgs);
  } else {
    int maxr = mt / g->wo;
    const int by_hp = dgrad ? cap / hw - 1 : (cap / hw - 1) / 2;
    if (maxr > by_hp) maxr = by_hp;
    if (maxr > g->ho) maxr = g->ho;
    g->nbands = ceil_div(g->ho, maxr);
    g->rows = ceil_div(g->ho, g->nbands);
    g->imgs = 1;
    g->tiles = g->n * g->nbands;
  }
  int workers = kCUs / blocks;
  if (workers < 1) workers = 1;
  if (workers > g->tiles) workers = g->tiles;
  if (max_workers > 0 && workers > max_workers) workers = max_workers;
  return workers;
}

GeomS2 geom(int n, int h, int w, int cin, int cout) {
  return GeomS2{n, h, w, (h - 1) / 2 + 1, (w - 1) / 2 + 1, cin, cout,
                0, 0, 0, 0};
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

bool conv3x3_s2_supported(long long n, long long h, long long w, int cin,
                          int cout) {
  return cin >= 64 && cin % 64 == 0 && cout >= SBN && cout % SBN == 0 &&
         n >= 1 && h >= 1 && w >= 1 && w <= 56 &&
         n * h < (1LL << 31) && n * h * w < (1LL << 31);
}

// Launch plans: rows and imgs of the tile of the Ho x Wo grid (header; one
// of them is 1 unless a whole image fits a tile), tiles per channel block,
// persistent workers per block: one workgroup per CU over all blocks, at
// most one per tile; max_workers > 0 lowers it further.
void conv3x3_s2_plan(int n, int h, int w, int cin, int cout, int max_workers,
                     int* rows, int* imgs, int* tiles, int* workers) {
  GeomS2 g = geom(n, h, w, cin, cout);
  *workers = plan(&g, false, cout / SBN, max_workers);
  *rows = g.rows;
  *imgs = g.imgs;
  *tiles = g.tiles;
}

void conv3x3_s2_dgrad_plan(int n, int h, int w, int cin, int cout,
                           int max_workers, int* rows, int* imgs, int* tiles,
                           int* workers) {
  GeomS2 g = geom(n, h, w, cin, cout);
  *workers = plan(&g, true, cin / SBN, max_workers);
  *rows = g.rows;
  *imgs = g.imgs;
  *tiles = g.tiles;
}

void launch_conv3x3_s2(const short* x, const short* wt, short* y, int n,
                       int h, int w, int cin, int cout, int max_workers,
                       hipStream_t stream) {
  static const hipError_t lds_set = hipFuncSetAttribute(
      (const void*)&conv3x3_s2_k, hipFuncAttributeMaxDynamicSharedMemorySize,
      kFLds);
  (void)lds_set;
  GeomS2 g = geom(n, h, w, cin, cout);
  const int workers = plan(&g, false, cout / SBN, max_workers);
  hipLaunchKernelGGL(conv3x3_s2_k, dim3((cout / SBN) * workers),
                     dim3(STHREADS), kFLds, stream, x, wt, y, g);
}

void launch_conv3x3_s2_dgrad(const short* dy, const short* wd, short* dx,
                             int n, int h, int w, int cin, int cout,
                             int max_workers, hipStream_t stream) {
  static const hipError_t lds_set = hipFuncSetAttribute(
      (const void*)&conv3x3_s2_dgrad_k,
      hipFuncAttributeMaxDynamicSharedMemorySize, kDLds);
  (void)lds_set;
  GeomS2 g = geom(n, h, w, cin, cout);
  const int workers = plan(&g, true, cin / SBN, max_workers);
  hipLaunchKernelGGL(conv3x3_s2_dgrad_k, dim3((cin / SBN) * workers),
                     dim3(STHREADS), kDLds, stream, dy, wd, dx, g);
}
