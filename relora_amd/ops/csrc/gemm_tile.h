// Shared device pieces of the 2-buffer fused GEMM kernels of fused_gemm.hip
// (dense, NF4, int8): 512 threads = 8 waves as 2M x 4N over a 256x256 output
// tile, [256][64] bf16 operand tiles staged by global_load_lds into swizzled
// LDS images, 16x16x32 MFMA fragments, the rank-r LoRA update on the resident
// accumulators and the LDS-staged b128 store epilogue.  The 3-buffer and
// bk32x4 research kernels, fp8_gemm.hip and mxfp4_gemm.hip keep copies of
// their own (docs/KERNELS.md "Shared GEMM tile header" says why).
//
// This header sets no function attribute of its own.  A file that compiles
// its code under `#pragma clang attribute push(target("no-packed-fp32-ops"))`
// has to include it INSIDE the pushed region: a helper without that attribute
// is not inlined into a kernel that has it.
#pragma once

#include "hip/hip_runtime.h"

#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// XCD-aware blockIdx remap (guide T1, bijective form): consecutive launch ids
// land on the same XCD's L2 as neighbors in tile space, so the B tile reused
// across M-blocks stays resident (+L2 locality on the K>=2048 shapes)
DEV_INLINE int xcd_remap() {
  const int nwg = gridDim.x;
  const int q8 = nwg >> 3, r8 = nwg & 7;
  int wgid = blockIdx.x;
  if (nwg >= 8) {
    const int xcd = wgid & 7, pos = wgid >> 3;
    wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + pos;
  }
  return wgid;
}

struct WaveCoord {
  int lane, wave;
  int wr;  // 0..1: wave m-position (128 rows)
  int wc;  // 0..3: wave n-position (64 cols)
  int fr;  // fragment row / C column
  int fq;  // fragment k-group / C row group
};

DEV_INLINE WaveCoord wave_coord() {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  return {lane, wave, wave >> 2, wave & 3, lane & 15, lane >> 4};
}

DEV_INLINE void zero_acc(f32x4 (&acc)[8][4]) {
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// st_16x32 swizzle on a byte offset within a [rows][64] bf16 image (128-B
// rows): byte bit5 ^= bit9 -- spreads each ds_read_b128 lane group over four
// 16-B slots (guide: bank-conflict 141x down, +35%).  It keeps the row and is
// an involution, so it maps LDS byte -> source byte when staging and logical
// byte -> LDS byte when reading.
DEV_INLINE unsigned swz(unsigned o) { return o ^ (((o >> 9) & 1u) << 5); }

// Stage one [256][64] bf16 tile (32 KB) into `image` via glds: 32 wave-level
// 1-KiB pieces (8 full rows each), 4 per wave.  The LDS image is lane-linear
// as glds requires; the per-lane GLOBAL source address carries the swizzle.
// `ld` (row pitch) and `k0` count bf16 elements.
DEV_INLINE void stage_glds(void* image, const __hip_bfloat16* gbase, long row0, long ld, long k0,
                           const WaveCoord& w) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int piece = w.wave * 4 + p;
    const unsigned s = swz(piece * 1024u + w.lane * 16u);  // source byte in tile
    const __hip_bfloat16* src = gbase + (row0 + (s >> 7)) * ld + k0 + ((s & 127u) >> 1);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)(image) + (piece * 1024u) / 4,
        16, 0, 0);
  }
}

// bf16 fragment (16x16x32 layout: lane -> row l&15, 8 k at ks*32 + (l>>4)*8)
DEV_INLINE bf16x8 frag_bf16(const void* image, int row, int ks, int fq) {
  const unsigned o = (unsigned)row * 128u + (unsigned)ks * 64u + (unsigned)fq * 16u;
  return *reinterpret_cast<const bf16x8*>((const char*)image + swz(o));
}

// 32 dequantised bf16 of image row `row`, k = half*32 .. +31, as 4 swizzled
// b128 LDS writes (the tail of the NF4 and int8 B stagers)
DEV_INLINE void write_dequant32(void* image, int row, int half, const __bf16 (&vals)[32]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const unsigned o = (unsigned)row * 128u + (unsigned)half * 64u + c * 16u;
    *reinterpret_cast<bf16x8*>((char*)image + swz(o)) =
        *reinterpret_cast<const bf16x8*>(vals + c * 8);
  }
}

// acc += A-image[128 rows of this wave][64 k] · B-image[64 rows][64 k]^T,
// between an s_setprio pair.
DEV_INLINE void mma_bf16_chunk(f32x4 (&acc)[8][4], const void* A, const void* B,
                               const WaveCoord& w) {
  __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    // the 4 B fragments stay resident; A fragments stream through
    bf16x8 bf[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bf[j] = frag_bf16(B, w.wc * 64 + j * 16 + w.fr, ks, w.fq);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bf16x8 af = frag_bf16(A, w.wr * 128 + i * 16 + w.fr, ks, w.fq);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf[j], acc[i][j], 0, 0, 0);
    }
  }
  __builtin_amdgcn_s_setprio(0);
}

// LoRA rank-r update: acc += t-tile @ Bw-tile^T in [256][64] chunks.  The host
// pre-scales t by lora_scale (scaling here would scale the main GEMM too).
// Chunk c lands at A and B, `alt` bytes further on for odd c (r <= 128: both
// operands fit the 4 buffer slots at once), serialized: vmcnt(0) + barrier,
// MFMAs, barrier.
DEV_INLINE void lora_update(f32x4 (&acc)[8][4], const __hip_bfloat16* t, const __hip_bfloat16* bw,
                            long m0, long n0, int r, char* A, char* B, unsigned alt,
                            const WaveCoord& w) {
  if (r <= 0) return;
  const int RC = r >> 6;
#pragma unroll 1
  for (int c = 0; c < RC; ++c) {
    char* Ac = A + (c & 1) * alt;
    char* Bc = B + (c & 1) * alt;
    stage_glds(Ac, t, m0, r, (long)c * 64, w);
    stage_glds(Bc, bw, n0, r, (long)c * 64, w);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    mma_bf16_chunk(acc, Ac, Bc, w);
    __syncthreads();  // all waves done reading before the next chunk lands
  }
}

// Epilogue: bias, ONE rounding to bf16, the wave's 128x64 tile into its own
// LDS region `mine` (16 KiB, row-major), then b128 row stores of it into the
// block at y[m0][n0] (pitch ld).  Per-element global stores are
// store-issue-bound; the LDS re-read gives b128 row stores (DESIGN.md rule
// 6).  Writes are 2-way (col pairs share a dword), the b128 reads
// conflict-free.  No barrier in between: each wave reads only its own region.
// bias and y are __restrict__ as in the kernels' signatures: without it every
// row store recomputes its 64-bit address.
DEV_INLINE void store_wave_tile(__bf16* mine, const f32x4 (&acc)[8][4],
                                const __hip_bfloat16* __restrict__ bias,
                                __hip_bfloat16* __restrict__ y, long m0, long ld, long n0,
                                const WaveCoord& w) {
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = i * 16 + w.fq * 4 + reg;  // within wave tile
        const int col = j * 16 + w.fr;
        float v = acc[i][j][reg];
        if (bias) v += (float)bias[n0 + w.wc * 64 + col];
        mine[row * 64 + col] = (__bf16)v;
      }
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const int row = rr * 8 + (w.lane >> 3);  // 0..127
    const int cb = (w.lane & 7) * 8;         // 8-col chunk
    const bf16x8 vv = *reinterpret_cast<const bf16x8*>(mine + row * 64 + cb);
    *reinterpret_cast<bf16x8*>(y + (m0 + w.wr * 128 + row) * ld + n0 + w.wc * 64 + cb) = vv;
  }
}
